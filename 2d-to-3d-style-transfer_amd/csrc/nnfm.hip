// nnfm.hip -- the nearest-neighbour feature matching style loss (Zhang et al., "ARF", ECCV 2022): every feature
// vector of a render tap looks up its nearest style feature by cosine distance, the loss is the weighted mean distance.
//   nnfm_normalise   (C, M) features -> the unit-norm copy and the norms; lanes run along the positions (the channel stride is
//                    M), the squares are added in ascending channel order in fp32; a zero vector stays zero
//   nnfm_search      the hot kernel: sim = S^ F^ on v_mfma_f32_32x32x2_f32, K = the channels, both operands k-major as they lie
//                    in memory.  Style positions on the accumulator's rows, queries on its columns: a lane owns one query
//                    column of each 32x32 block and keeps a running (max, index) over its rows in registers; lanes and waves
//                    are merged once per workgroup.  The N x M similarities are never written.  The style range is cut into
//                    `segments` runs along grid.y; query tiles without an active position end at once
//   nnfm_merge       maximum over the runs in ascending order with the same strict >; the distance written is recomputed from
//                    the two unit vectors as one ascending fmaf chain (what the matrix pipe computes, bit for bit)
//   nnfm_sum / bwd   ordered fp64 sums of w d and w per image; the gradient, one writer per element, exact zeros where inactive
// Every similarity is ONE k-ordered fp32 fma chain over all channels (no split over K), so its value does not depend on the
// tile or run it fell into: equal style vectors tie bit for bit and the lowest index wins under any tiling.
// No float atomics: two runs are bit-equal.  Built with -ffp-contract=off: the roundings of the norm are the ones written here.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TQ = 128;             // queries per workgroup (accumulator columns)
constexpr int TS = 128;             // style positions per tile (accumulator rows)
constexpr int KCH = 32;             // channels per LDS chunk: K is streamed, so C = 512 needs no more LDS than C = 64
constexpr int THREADS = 256;        // 4 waves as 2 (style) x 2 (query), each 64 x 64 = four 32x32 accumulators
constexpr int TARGET_WG = 1024;     // workgroups wanted per image: two on every CU, twice over
constexpr int MAX_POS = 1 << 20;
constexpr int MAX_C = 512;
constexpr int MAX_B = 65535;        // grid.z
constexpr int SUM_BLOCK = 1024;

inline bool sizes_ok(int N, int M, int C) { return N >= 1 && N <= MAX_POS && M >= 1 && M <= MAX_POS && C >= 1 && C <= MAX_C; }

inline int nnfm_segments(int N, int M, int *seg_tiles) {
    const int qtiles = st3d::cdiv(N, TQ), stiles = st3d::cdiv(M, TS);
    int want = TARGET_WG / qtiles;
    if (want < 1) want = 1;
    if (want > stiles) want = stiles;
    *seg_tiles = st3d::cdiv(stiles, want);                 // run length = seg_tiles * TS style positions
    return st3d::cdiv(stiles, *seg_tiles);
}

// 4 consecutive elements along the position axis, zero from `remain` on
__device__ __forceinline__ float4 load4(const float *p, long remain, bool aligned) {
    if (remain >= 4 && aligned) return *reinterpret_cast<const float4 *>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (remain > 0) v.x = p[0];
    if (remain > 1) v.y = p[1];
    if (remain > 2) v.z = p[2];
    if (remain > 3) v.w = p[3];
    return v;
}

// grid (cdiv(M, 256), B).  x (B, C, M) -> xhat (B, C, M) (may be NULL), norm (B, M)
__global__ __launch_bounds__(256) void nnfm_normalise_kernel(const float *__restrict__ x, int C, int M, float *__restrict__ xhat,
                                                             float *__restrict__ norm) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const float *xb = x + (size_t)blockIdx.y * C * M + j;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = xb[(size_t)c * M];
        acc = acc + v * v;
    }
    const float n = sqrtf(acc);
    norm[(size_t)blockIdx.y * M + j] = n;
    if (!xhat) return;
    float *hb = xhat + (size_t)blockIdx.y * C * M + j;
    for (int c = 0; c < C; ++c) hb[(size_t)c * M] = n == 0.f ? 0.f : xb[(size_t)c * M] / n;
}

// grid (cdiv(N, TQ), segments, B).  fhat (B, C, N), shat (Bs, C, M) with image stride s_stride (0 when Bs = 1), w (B, N) or
// NULL.  seg_best / seg_idx: (segments, B, N).  A NaN similarity never passes v > best: a NaN style vector is never chosen
// and a NaN query keeps (-Inf, 0).
__global__ __launch_bounds__(THREADS, 2) void nnfm_search_kernel(const float *__restrict__ fhat, const float *__restrict__ shat,
                                                                 size_t s_stride, const float *__restrict__ w, int C, int N, int M,
                                                                 int seg_tiles, float *__restrict__ seg_best,
                                                                 int32_t *__restrict__ seg_idx) {
    __shared__ __attribute__((aligned(16))) float Ss[KCH * TS];
    __shared__ __attribute__((aligned(16))) float Qs[KCH * TQ];
    __shared__ float mbest[4 * TQ];
    __shared__ int32_t midx[4 * TQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int ws = wave >> 1, wq = wave & 1;
    const int b = blockIdx.z, nb = gridDim.z;
    const int q0 = blockIdx.x * TQ;

    if (w) {                                                        // a query tile with no active position costs no search
        int active = 0;
        if (tid < TQ && q0 + tid < N) active = w[(size_t)b * N + q0 + tid] != 0.f;
        if (!__syncthreads_or(active)) return;
    }

    const float *Fb = fhat + (size_t)b * C * N;
    const float *Sb = shat + (size_t)b * s_stride;
    const bool f_al = ((N & 3) == 0) && ((((uintptr_t)Fb) & 15) == 0);
    const bool s_al = ((M & 3) == 0) && ((((uintptr_t)Sb) & 15) == 0);

    const long seg_lo = (long)blockIdx.y * seg_tiles * TS;
    long seg_hi = seg_lo + (long)seg_tiles * TS;
    if (seg_hi > M) seg_hi = M;
    const int ntiles = seg_lo < seg_hi ? (int)((seg_hi - seg_lo + TS - 1) / TS) : 0;
    const int ksteps = (C + KCH - 1) / KCH;
    const int total = ntiles * ksteps;

    // staging: a chunk is KCH channel rows of 128 positions = 1024 float4 per operand, four per thread
    float4 sv[4], qv[4];
    auto load_tiles = [&](int step) {
        const int t = step / ksteps, k0 = (step - t * ksteps) * KCH;
        const long j0 = seg_lo + (long)t * TS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * THREADS, kr = e >> 5, p4 = (e & 31) * 4;
            const int gk = k0 + kr;
            const long gj = j0 + p4;
            const int gq = q0 + p4;
            sv[i] = gk < C ? load4(Sb + (size_t)gk * M + gj, (long)M - gj, s_al) : make_float4(0.f, 0.f, 0.f, 0.f);
            qv[i] = gk < C ? load4(Fb + (size_t)gk * N + gq, (long)N - gq, f_al) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * THREADS, kr = e >> 5, p4 = (e & 31) * 4;
            *reinterpret_cast<float4 *>(&Ss[kr * TS + p4]) = sv[i];
            *reinterpret_cast<float4 *>(&Qs[kr * TQ + p4]) = qv[i];
        }
    };

    float best[2] = {-__builtin_inff(), -__builtin_inff()};
    int bi[2] = {0, 0};
    f32x16 acc[2][2];

    if (total > 0) load_tiles(0);
    for (int step = 0; step < total; ++step) {
        const int t = step / ksteps, kc = step - t * ksteps;
        if (kc == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;
        }
        __syncthreads();                                            // the previous chunk's reads are done
        store_tiles();
        __syncthreads();
        if (step + 1 < total) load_tiles(step + 1);                 // in flight under the MFMAs below
        const float *pa = Ss + lhi * TS + ws * 64 + l31;
        const float *pb = Qs + lhi * TQ + wq * 64 + l31;
#pragma unroll
        for (int kk = 0; kk < KCH / 2; ++kk) {
            float a[2], bb[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) a[m] = pa[(kk * 2) * TS + m * 32];
#pragma unroll
            for (int q = 0; q < 2; ++q) bb[q] = pb[(kk * 2) * TQ + q * 32];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bb[q], acc[m][q], 0, 0, 0);
        }
        if (kc == ksteps - 1) {
            // this lane's rows of the tile in ascending order: the strict > keeps the lowest index among its equals
            const long j0 = seg_lo + (long)t * TS;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long row = j0 + ws * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    const bool in = row < seg_hi;                   // rows past M are padding, not candidates
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const float v = acc[m][q][r];
                        if (in && v > best[q]) { best[q] = v; bi[q] = (int)row; }
                    }
                }
        }
    }

    // one query column is held by four lanes (2 style waves x 2 lane halves) whose rows interleave: the maximum, and the
    // lowest index among equal maxima
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = wq * 64 + q * 32 + l31;
        mbest[(ws * 2 + lhi) * TQ + col] = best[q];
        midx[(ws * 2 + lhi) * TQ + col] = bi[q];
    }
    __syncthreads();
    if (tid < TQ && q0 + tid < N) {
        float v = mbest[tid];
        int id = midx[tid];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float vk = mbest[k * TQ + tid];
            const int ik = midx[k * TQ + tid];
            if (vk > v || (vk == v && ik < id)) { v = vk; id = ik; }
        }
        const size_t o = ((size_t)blockIdx.y * nb + b) * N + q0 + tid;
        seg_best[o] = v;
        seg_idx[o] = id;
    }
}

// grid (cdiv(N, 256), B)
__global__ __launch_bounds__(256) void nnfm_merge_kernel(const float *__restrict__ fhat, const float *__restrict__ fnorm,
                                                         const float *__restrict__ shat, size_t s_stride,
                                                         const float *__restrict__ w, int C, int N, int M, int segments,
                                                         const float *__restrict__ seg_best, const int32_t *__restrict__ seg_idx,
                                                         int32_t *__restrict__ idx, float *__restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int b = blockIdx.y, nb = gridDim.y;
    const size_t o = (size_t)b * N + i;
    if (w && w[o] == 0.f) { idx[o] = -1; dist[o] = 0.f; return; }  // inactive: its tile may not have been searched at all
    if (fnorm[o] == 0.f) { idx[o] = -1; dist[o] = 1.f; return; }   // a zero query
    float best = -__builtin_inff();
    int bi = 0;
    for (int s = 0; s < segments; ++s) {
        const size_t k = ((size_t)s * nb + b) * N + i;
        const float v = seg_best[k];
        if (v > best) { best = v; bi = seg_idx[k]; }
    }
    if ((unsigned)bi >= (unsigned)M) bi = 0;                        // cannot happen; keeps the gather below in bounds
    const float *f = fhat + (size_t)b * C * N + i;
    const float *s = shat + (size_t)b * s_stride + bi;
    float sim = 0.f;
    for (int c = 0; c < C; ++c) sim = __builtin_fmaf(s[(size_t)c * M], f[(size_t)c * N], sim);
    idx[o] = bi;
    dist[o] = 1.0f - sim;
}

// one workgroup.  Per image b: num = sum_i w_i d_i, den = sum_i w_i (w == NULL: 1), thread t sums i = t, t + 1024, ... then
// a fixed tree, in fp64; wsum[b] = den; loss = (float)(inv_denom * sum_b (den > 0 ? num / den : 0)), the images in order.
// An inactive position (w_i = 0) adds an exact 0 whatever d_i holds.
__global__ __launch_bounds__(SUM_BLOCK) void nnfm_sum_kernel(const float *__restrict__ d, const float *__restrict__ w, int B, int N,
                                                             double inv_denom, float *__restrict__ loss, double *__restrict__ wsum) {
    __shared__ double sn[SUM_BLOCK], sd[SUM_BLOCK];
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double num = 0.0, den = 0.0;
        for (int i = threadIdx.x; i < N; i += SUM_BLOCK) {
            const size_t o = (size_t)b * N + i;
            const double wi = w ? (double)w[o] : 1.0;
            if (wi != 0.0) num += wi * (double)d[o];
            den += wi;
        }
        sn[threadIdx.x] = num;
        sd[threadIdx.x] = den;
        __syncthreads();
        for (int s = SUM_BLOCK / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) { sn[threadIdx.x] += sn[threadIdx.x + s]; sd[threadIdx.x] += sd[threadIdx.x + s]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            wsum[b] = sd[0];
            if (sd[0] > 0.0) total += sn[0] / sd[0];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(inv_denom * total);
}

// grid (cdiv(N, 256), B).  grad[b, c, i] = -(g w_i inv_denom / (W_b n_i)) (s^_jc - sim f^_ic), j = idx_i, sim = 1 - d_i,
// n_i recomputed from the tap in fp64 (ascending c), f^_ic = f_ic / n_i, all in fp64, rounded once; exact zeros where
// idx_i < 0 (inactive or zero query) or W_b = 0.
__global__ __launch_bounds__(256) void nnfm_bwd_kernel(const float *__restrict__ feat,
                                                       const float *__restrict__ shat, size_t s_stride,
                                                       const int32_t *__restrict__ idx, const float *__restrict__ dist,
                                                       const float *__restrict__ w, const double *__restrict__ wsum,
                                                       const float *__restrict__ gout, int C, int N, int M, double inv_denom,
                                                       float *__restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int b = blockIdx.y;
    const size_t o = (size_t)b * N + i;
    const int j = idx[o];
    const double Wb = wsum[b];
    float *g = grad + (size_t)b * C * N + i;
    if (j < 0 || j >= M || !(Wb > 0.0) || (w && w[o] == 0.f)) {
        for (int c = 0; c < C; ++c) g[(size_t)c * N] = 0.f;
        return;
    }
    const float *f = feat + (size_t)b * C * N + i;
    double n2 = 0.0;
    for (int c = 0; c < C; ++c) n2 += (double)f[(size_t)c * N] * (double)f[(size_t)c * N];
    const double n = sqrt(n2), sim = 1.0 - (double)dist[o];
    const double wi = w ? (double)w[o] : 1.0;
    const double cf = -((gout ? (double)gout[0] : 1.0) * wi * inv_denom) / (Wb * n);
    const float *s = shat + (size_t)b * s_stride + j;
    for (int c = 0; c < C; ++c) g[(size_t)c * N] = (float)(cf * ((double)s[(size_t)c * M] - sim * ((double)f[(size_t)c * N] / n)));
}

}  // namespace

extern "C" int st3d_nnfm_geometry(int N, int M, int C, int *tile_q, int *tile_s, int *segments) {
    ST3D_CHECK_ARG(tile_q && tile_s && segments);
    ST3D_CHECK_ARG(sizes_ok(N, M, C));
    int seg_tiles;
    *segments = nnfm_segments(N, M, &seg_tiles);
    *tile_q = TQ;
    *tile_s = TS;
    return ST3D_OK;
}

extern "C" size_t st3d_nnfm_workspace_bytes(int B, int N, int M, int C) {
    if (!sizes_ok(N, M, C) || B < 1 || B > MAX_B) return 0;
    int seg_tiles;
    return (size_t)nnfm_segments(N, M, &seg_tiles) * (size_t)B * (size_t)N * 8;
}

extern "C" int st3d_nnfm_normalise(const float *x, int B, int C, int M, float *xhat, float *norm, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && norm);
    ST3D_CHECK_ARG(B >= 1 && B <= MAX_B && sizes_ok(M, M, C));
    nnfm_normalise_kernel<<<dim3(st3d::cdiv(M, 256), B), 256, 0, st3d::as_stream(stream)>>>(x, C, M, xhat, norm);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_nnfm_search(const float *feat_hat, const float *feat_norm, const float *style_hat, const float *weights, int B,
                                int Bs, int C, int N, int M, void *workspace, size_t workspace_bytes, int32_t *idx, float *dist,
                                st3d_stream_t stream) {
    ST3D_CHECK_ARG(feat_hat && feat_norm && style_hat && workspace && idx && dist);
    ST3D_CHECK_ARG(B >= 1 && B <= MAX_B && (Bs == 1 || Bs == B) && sizes_ok(N, M, C));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_nnfm_workspace_bytes(B, N, M, C) && ((uintptr_t)workspace & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    int seg_tiles;
    const int segments = nnfm_segments(N, M, &seg_tiles);
    const size_t s_stride = Bs == 1 ? 0 : (size_t)C * M;
    float *seg_best = static_cast<float *>(workspace);
    int32_t *seg_idx = reinterpret_cast<int32_t *>(seg_best + (size_t)segments * B * N);
    nnfm_search_kernel<<<dim3(st3d::cdiv(N, TQ), segments, B), THREADS, 0, s>>>(feat_hat, style_hat, s_stride, weights, C, N, M,
                                                                               seg_tiles, seg_best, seg_idx);
    ST3D_LAUNCH_CHECK();
    nnfm_merge_kernel<<<dim3(st3d::cdiv(N, 256), B), 256, 0, s>>>(feat_hat, feat_norm, style_hat, s_stride, weights, C, N, M, segments,
                                                                 seg_best, seg_idx, idx, dist);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_nnfm_sum(const float *dist, const float *weights, int B, int N, double inv_denom, float *loss, double *wsum,
                             st3d_stream_t stream) {
    ST3D_CHECK_ARG(dist && loss && wsum);
    ST3D_CHECK_ARG(B >= 1 && B <= MAX_B && N >= 1 && N <= MAX_POS && ((uintptr_t)wsum & 7) == 0);
    nnfm_sum_kernel<<<1, SUM_BLOCK, 0, st3d::as_stream(stream)>>>(dist, weights, B, N, inv_denom, loss, wsum);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_nnfm_bwd(const float *feat, const float *style_hat, const int32_t *idx, const float *dist,
                             const float *weights, const double *wsum, const float *grad_out, int B, int Bs, int C, int N, int M,
                             double inv_denom, float *grad_feat, st3d_stream_t stream) {
    ST3D_CHECK_ARG(feat && style_hat && idx && dist && wsum && grad_feat);
    ST3D_CHECK_ARG(B >= 1 && B <= MAX_B && (Bs == 1 || Bs == B) && sizes_ok(N, M, C) && ((uintptr_t)wsum & 7) == 0);
    const size_t s_stride = Bs == 1 ? 0 : (size_t)C * M;
    nnfm_bwd_kernel<<<dim3(st3d::cdiv(N, 256), B), 256, 0, st3d::as_stream(stream)>>>(feat, style_hat, s_stride, idx, dist,
                                                                                     weights, wsum, grad_out, C, N, M, inv_denom,
                                                                                     grad_feat);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
