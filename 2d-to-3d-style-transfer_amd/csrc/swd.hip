// swd.hip -- the sliced Wasserstein style loss (Heitz, Vanhoey, Chambon, Belcour, "A Sliced Wasserstein Loss for Neural
// Texture Synthesis", CVPR 2021): the features of a render tap and of the style tap are projected onto K random
// directions, every projected row is sorted, and the loss is the mean squared difference of matching quantiles.
//   swd_project      out = a x on v_mfma_f32_32x32x2_f32: the rows of `a` on the accumulator's rows, the positions on its
//                    columns, the summed index streamed through LDS in chunks and never split, so each value is ONE ascending
//                    fp32 fma chain from +0 whatever tile it fell into (a chain from +0 is never -0, so the zero padding of the
//                    last chunk changes nothing).  Forward: a = V; backward: a = V^T on the gradient of the projections
//   swd_sort         a bitonic network on one 64-bit word per position, (inactive, key, index) from the top bit down: the words
//                    of a row are distinct, so ANY correct sort gives the one result the total order fixes.  Rows are padded to
//                    a power of two with all-ones words, which sort behind every position and are never written out.  All
//                    strides below the block run in LDS (8192 words = 64 KB per workgroup, two workgroups per CU).  A row
//                    longer than a block takes TWO passes per level of the network, whatever the level: the strides at or above
//                    the block all at once on tiles that are strided in memory (2^h slabs of the block apart, 8192 / 2^h
//                    contiguous words from each, which holds every partner of every such stride), then the strides below it
//   swd_loss / bwd   one ordered fp64 sum per row, the rows of an image and the images in order by one workgroup; the gradient
//                    scattered through perm, one writer per element, exact +0 where inactive
// No float atomics: two runs are bit-equal.
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR = 128;             // rows of `a` per workgroup (accumulator rows)
constexpr int TN = 128;             // positions per workgroup (accumulator columns)
constexpr int KCH = 32;             // summed indices per LDS chunk
constexpr int AST = TR + 1;         // row stride of the `a` chunk: its transposing writes then hit 32 banks
constexpr int THREADS = 256;        // 4 waves as 2 (rows) x 2 (positions), each 64 x 64 = four 32x32 accumulators
constexpr int MAX_POS = 1 << 20;
constexpr int MAX_C = 512;
constexpr int MAX_B = 65535;
constexpr int SORT_BLOCK = 8192;    // words per workgroup in LDS
constexpr int SORT_BLOCK_LOG2 = 13;
constexpr int SORT_THREADS = 1024;
constexpr int IDX_BITS = 20;        // MAX_POS = 2^20 indices
constexpr long MAX_GRID = 2147483647L;

inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// strided launches of a row of N positions: one per level of the network above the block
inline int sort_passes(int N) {
    const int P = pow2_at_least(N);
    int passes = 0;
    for (long k = 2L * SORT_BLOCK; k <= P; k <<= 1) ++passes;
    return passes;
}

inline size_t sort_workspace(long rows, int N) { return N <= SORT_BLOCK ? 0 : (size_t)rows * (size_t)pow2_at_least(N) * 8; }

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

// grid (cdiv(N, TN), cdiv(R, TR), B).  x (B, Q, N), a (R, Q) -> out (B, R, N)
__global__ __launch_bounds__(THREADS, 2) void swd_project_kernel(const float *__restrict__ x, const float *__restrict__ a, int Q,
                                                                 int R, int N, float *__restrict__ out) {
    __shared__ float As[KCH * AST];
    __shared__ __attribute__((aligned(16))) float Xs[KCH * TN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int wr = wave >> 1, wn = wave & 1;
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * TR, n0 = blockIdx.x * TN;
    const float *Xb = x + (size_t)b * Q * N;
    const bool x_al = ((N & 3) == 0) && ((((uintptr_t)Xb) & 15) == 0);
    const int ksteps = (Q + KCH - 1) / KCH;

    // staging: a chunk is KCH rows of 128 positions of x (four float4 per thread) and KCH columns of 128 rows of `a`, read
    // along its contiguous axis and transposed on the way into LDS
    float4 xv[4];
    float av[16];
    auto load_tiles = [&](int step) {
        const int k0 = step * KCH;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * THREADS, kr = e >> 5, p4 = (e & 31) * 4;
            const int gk = k0 + kr, gn = n0 + p4;
            xv[i] = gk < Q ? load4(Xb + (size_t)gk * N + gn, (long)N - gn, x_al) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * THREADS, kr = e & 31, r = e >> 5;
            const int gk = k0 + kr, gr = r0 + r;
            av[i] = (gk < Q && gr < R) ? a[(size_t)gr * Q + gk] : 0.f;
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + i * THREADS, kr = e >> 5, p4 = (e & 31) * 4;
            *reinterpret_cast<float4 *>(&Xs[kr * TN + p4]) = xv[i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = tid + i * THREADS, kr = e & 31, r = e >> 5;
            As[kr * AST + r] = av[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;
    const bool rows_live = r0 + wr * 64 < R;                        // wave-uniform: a wave whose rows are all padding idles

    load_tiles(0);
    for (int step = 0; step < ksteps; ++step) {
        __syncthreads();                                            // the previous chunk's reads are done
        store_tiles();
        __syncthreads();
        if (step + 1 < ksteps) load_tiles(step + 1);                // in flight under the MFMAs below
        if (rows_live) {
            const float *pa = As + lhi * AST + wr * 64 + l31;
            const float *pb = Xs + lhi * TN + wn * 64 + l31;
#pragma unroll
            for (int kk = 0; kk < KCH / 2; ++kk) {
                float fa[2], fb[2];
#pragma unroll
                for (int m = 0; m < 2; ++m) fa[m] = pa[(kk * 2) * AST + m * 32];
#pragma unroll
                for (int q = 0; q < 2; ++q) fb[q] = pb[(kk * 2) * TN + q * 32];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[m], fb[q], acc[m][q], 0, 0, 0);
            }
        }
    }

    float *Ob = out + (size_t)b * R * N;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = r0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int col = n0 + wn * 64 + q * 32 + l31;
                if (row < R && col < N) Ob[(size_t)row * N + col] = acc[m][q][r];
            }
        }
}

// the sort word of a position: bit 52 = inactive, bits 51..20 = the order-preserving key of the value, bits 19..0 = its index
__device__ __forceinline__ uint64_t sort_word(float v, bool inactive, uint32_t idx) {
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;           // every NaN sorts as the canonical one, after +Inf
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)(inactive ? 1u : 0u) << (32 + IDX_BITS)) | ((uint64_t)key << IDX_BITS) | (uint64_t)idx;
}

// where word i of a tile lies in LDS: bits 5..7 of i folded into its lowest three.  A thread that takes 8 consecutive words
// (the strides 4, 2, 1) then meets 32 different bank pairs across a half-wave instead of 4; runs of 32 consecutive words
// stay on 32 different ones.
__device__ __forceinline__ int sw(int i) { return i ^ ((i >> 5) & 7); }

// G consecutive steps of one level -- strides low 2^(G-1) ... low -- in one round trip through LDS: a thread takes the 2^G
// words i0 + m low, which hold every partner of each other under these strides, into registers.  They lie in one run of the
// level (their indices differ below k only), so they sort one way: up iff bit k of their row position is clear.
template <int G>
__device__ __forceinline__ void lds_group(uint64_t *s, int n, long base, long k, int low) {
    for (int p = threadIdx.x; p < (n >> G); p += SORT_THREADS) {
        const int i0 = ((p & ~(low - 1)) << G) | (p & (low - 1));
        const bool asc = ((base + i0) & k) == 0;
        uint64_t v[1 << G];
#pragma unroll
        for (int m = 0; m < (1 << G); ++m) v[m] = s[sw(i0 + m * low)];
#pragma unroll
        for (int t = G - 1; t >= 0; --t)
#pragma unroll
            for (int m = 0; m < (1 << G); ++m)
                if (!(m & (1 << t))) {
                    const uint64_t lo = v[m], hi = v[m | (1 << t)];
                    const bool swap = (lo > hi) == asc;
                    v[m] = swap ? hi : lo;
                    v[m | (1 << t)] = swap ? lo : hi;
                }
#pragma unroll
        for (int m = 0; m < (1 << G); ++m) s[sw(i0 + m * low)] = v[m];
    }
    __syncthreads();
}

// the bitonic steps j = jstart, jstart / 2, ... jstop of level k on the `n` words in LDS whose word i stands at position
// base + i of the row as far as bit k goes; three steps at a time, the one or two left over first, so that the last three
// (down to jstop) always go together
__device__ __forceinline__ void lds_steps(uint64_t *s, int n, long base, long k, int jstart, int jstop) {
    int j = jstart, steps = 0;
    for (int t = jstart; t >= jstop; t >>= 1) ++steps;
    if (steps % 3 == 2) { lds_group<2>(s, n, base, k, j >> 1); j >>= 2; }
    else if (steps % 3 == 1) { lds_group<1>(s, n, base, k, j); j >>= 1; }
    for (; j >= jstop; j >>= 3) lds_group<3>(s, n, base, k, j >> 2);
}

// grid (rows * P / n), n = min(P, SORT_BLOCK) words per workgroup.  first: the words are built from proj (and weights) and the
// levels k = 2 .. n run; else the words come from `words` and the steps below the block of level k run.  last: the row is
// sorted after this launch and sorted / perm are written; else the words go (back) to `words`.
__global__ __launch_bounds__(SORT_THREADS) void swd_sort_local_kernel(const float *__restrict__ proj, const float *__restrict__ w,
                                                                      uint64_t *__restrict__ words, int K, int N, int P, long k,
                                                                      int first, int last, float *__restrict__ sorted,
                                                                      int32_t *__restrict__ perm) {
    __shared__ uint64_t s[SORT_BLOCK];
    const int n = P < SORT_BLOCK ? P : SORT_BLOCK;
    const int per_row = P / n;
    const long row = blockIdx.x / per_row;
    const long base = (long)(blockIdx.x - row * per_row) * n;
    const float *prow = proj + (size_t)row * N;
    uint64_t *wrow = words ? words + (size_t)row * P : nullptr;

    if (first) {
        const float *wimg = w ? w + (size_t)(row / K) * N : nullptr;
        for (int i = threadIdx.x; i < n; i += SORT_THREADS) {
            const long gi = base + i;
            s[sw(i)] = gi < N ? sort_word(prow[gi], wimg ? !(wimg[gi] > 0.f) : false, (uint32_t)gi) : ~(uint64_t)0;
        }
        __syncthreads();
        for (int kk = 2; kk <= n; kk <<= 1) lds_steps(s, n, base, kk, kk >> 1, 1);
    } else {
        for (int i = threadIdx.x; i < n; i += SORT_THREADS) s[sw(i)] = wrow[base + i];
        __syncthreads();
        lds_steps(s, n, base, k, n >> 1, 1);
    }

    if (!last) {
        for (int i = threadIdx.x; i < n; i += SORT_THREADS) wrow[base + i] = s[sw(i)];
        return;
    }
    for (int i = threadIdx.x; i < n; i += SORT_THREADS) {
        const long gi = base + i;
        if (gi >= N) continue;                                      // the padding sorts behind every position
        const uint64_t c = s[sw(i)];
        uint32_t idx = (uint32_t)(c & ((1u << IDX_BITS) - 1));
        if (idx >= (uint32_t)N) idx = 0;                            // cannot happen; keeps the gather below in bounds
        const uint32_t key = (uint32_t)(c >> IDX_BITS);
        const uint32_t u = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
        sorted[(size_t)row * N + gi] = u == 0x7fc00000u ? prow[idx] : __uint_as_float(u);      // a NaN as it came
        if (perm) perm[(size_t)row * N + gi] = (int32_t)idx;
    }
}

// grid (rows * P / SORT_BLOCK): the steps j = k / 2 ... SORT_BLOCK of level k = SORT_BLOCK 2^h, in place.  A run of k words is
// 2^h slabs of SORT_BLOCK; a tile takes the same `wdt` = SORT_BLOCK / 2^h contiguous words of every slab of one run (h <= 7:
// at least 64 words, 512 bytes, at a time), so word (r, q) of the tile sits at r wdt + q in LDS and stride SORT_BLOCK 2^s in
// memory is stride wdt 2^s there.  The whole run sorts one way.
__global__ __launch_bounds__(SORT_THREADS) void swd_sort_strided_kernel(uint64_t *__restrict__ words, int P, long k, int h) {
    __shared__ uint64_t s[SORT_BLOCK];
    const int per_row = P / SORT_BLOCK, per_run = 1 << h;
    const int wdt = SORT_BLOCK >> h, wlog = SORT_BLOCK_LOG2 - h;
    const long row = blockIdx.x / per_row;
    const int t = (int)(blockIdx.x - row * per_row);
    const int run = t >> h, c = t & (per_run - 1);
    uint64_t *base = words + (size_t)row * P + (size_t)run * k + (size_t)c * wdt;
    for (int e = threadIdx.x; e < SORT_BLOCK; e += SORT_THREADS) s[sw(e)] = base[(size_t)(e >> wlog) * SORT_BLOCK + (e & (wdt - 1))];
    __syncthreads();
    // every word of the tile belongs to the run: `base` = the run's start stands for all of them (LDS indices stay below k)
    lds_steps(s, SORT_BLOCK, (long)run * k, k, SORT_BLOCK >> 1, wdt);
    for (int e = threadIdx.x; e < SORT_BLOCK; e += SORT_THREADS) base[(size_t)(e >> wlog) * SORT_BLOCK + (e & (wdt - 1))] = s[sw(e)];
}

// grid (B): count[b] = the positions with w > 0 (integers: any order gives the same sum)
__global__ __launch_bounds__(256) void swd_count_kernel(const float *__restrict__ w, int N, int32_t *__restrict__ count) {
    __shared__ int sc[256];
    const float *wb = w + (size_t)blockIdx.x * N;
    int c = 0;
    for (int i = threadIdx.x; i < N; i += 256) c += wb[i] > 0.f;
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sc[threadIdx.x] += sc[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[blockIdx.x] = sc[0];
}

__global__ void swd_count_all_kernel(int B, int N, int32_t *__restrict__ count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) count[b] = N;
}

__device__ __forceinline__ int clamp_count(int n, int N) { return n < 0 ? 0 : (n > N ? N : n); }

// grid (B K).  partial[row] = sum_{r < n_b} (sorted_r - tsorted_{j(r)})^2: thread t adds r = t, t + 256, ... then a fixed tree
__global__ __launch_bounds__(256) void swd_loss_rows_kernel(const float *__restrict__ sorted, const int32_t *__restrict__ count,
                                                            const float *__restrict__ tsorted, size_t t_stride, int K, int N, int M,
                                                            double *__restrict__ partial) {
    __shared__ double sd[256];
    const size_t row = blockIdx.x;
    const int b = (int)(row / K), k = (int)(row - (size_t)b * K);
    const int n = clamp_count(count[b], N);
    const float *s = sorted + row * N;
    const float *t = tsorted + (size_t)b * t_stride + (size_t)k * M;
    double acc = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) {
        const long j = ((2L * r + 1) * M) / (2L * n);
        const double d = (double)s[r] - (double)t[j];
        acc += d * d;
    }
    sd[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sd[threadIdx.x] += sd[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[row] = sd[0];
}

// one workgroup: per image the K row sums (thread t adds k = t, t + 256, ... then the tree) over K n_b, the images in order
__global__ __launch_bounds__(256) void swd_loss_finish_kernel(const double *__restrict__ partial, const int32_t *__restrict__ count,
                                                              int B, int K, int N, double inv_denom, float *__restrict__ loss) {
    __shared__ double sd[256];
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double acc = 0.0;
        for (int k = threadIdx.x; k < K; k += 256) acc += partial[(size_t)b * K + k];
        sd[threadIdx.x] = acc;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if ((int)threadIdx.x < h) sd[threadIdx.x] += sd[threadIdx.x + h];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const int n = clamp_count(count[b], N);
            if (n > 0) total += sd[0] / ((double)K * (double)n);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(inv_denom * total);
}

// grid (B K cdiv(N, 256)): rank r of a row writes element perm[r] of it -- perm is a permutation, so every element is
// written exactly once
__global__ __launch_bounds__(256) void swd_bwd_kernel(const float *__restrict__ sorted, const int32_t *__restrict__ perm,
                                                      const int32_t *__restrict__ count, const float *__restrict__ tsorted,
                                                      size_t t_stride, const float *__restrict__ gout, int K, int N, int M,
                                                      int nblk, double inv_denom, float *__restrict__ gproj) {
    const size_t row = blockIdx.x / nblk;
    const int r = (int)(blockIdx.x - row * nblk) * 256 + threadIdx.x;
    if (r >= N) return;
    const int b = (int)(row / K), k = (int)(row - (size_t)b * K);
    const int n = clamp_count(count[b], N);
    const int i = perm[row * N + r];
    if ((unsigned)i >= (unsigned)N) return;                         // cannot happen with the perm of st3d_swd_sort
    float g = 0.f;
    if (r < n) {
        const long j = ((2L * r + 1) * M) / (2L * n);
        const double d = (double)sorted[row * N + r] - (double)tsorted[(size_t)b * t_stride + (size_t)k * M + j];
        const double cf = ((gout ? (double)gout[0] : 1.0) * 2.0 * inv_denom) / ((double)K * (double)n);
        g = (float)(cf * d);
    }
    gproj[row * N + i] = g;
}

inline bool dims_ok(int B, int K, int N) { return B >= 1 && B <= MAX_B && K >= 1 && K <= MAX_C && N >= 1 && N <= MAX_POS; }

}  // namespace

extern "C" int st3d_swd_project(const float *x, const float *a, int B, int Q, int R, int N, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && a && out);
    ST3D_CHECK_ARG(B >= 1 && B <= MAX_B && Q >= 1 && Q <= MAX_C && R >= 1 && R <= MAX_C && N >= 1 && N <= MAX_POS);
    swd_project_kernel<<<dim3(st3d::cdiv(N, TN), st3d::cdiv(R, TR), B), THREADS, 0, st3d::as_stream(stream)>>>(x, a, Q, R, N, out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_swd_geometry(int N, int *block, int *passes) {
    ST3D_CHECK_ARG(block && passes);
    ST3D_CHECK_ARG(N >= 1 && N <= MAX_POS);
    *block = SORT_BLOCK;
    *passes = sort_passes(N);
    return ST3D_OK;
}

extern "C" size_t st3d_swd_workspace_bytes(int B, int K, int N) {
    if (!dims_ok(B, K, N)) return 0;
    return sort_workspace((long)B * K, N);
}

extern "C" int st3d_swd_sort(const float *proj, const float *weights, int B, int K, int N, void *workspace, size_t workspace_bytes,
                             float *sorted, int32_t *perm, int32_t *count, st3d_stream_t stream) {
    ST3D_CHECK_ARG(proj && sorted);
    ST3D_CHECK_ARG(dims_ok(B, K, N));
    const long rows = (long)B * K;
    const size_t need = sort_workspace(rows, N);
    ST3D_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0));
    const int P = pow2_at_least(N);
    const int n = P < SORT_BLOCK ? P : SORT_BLOCK;
    const long local_blocks = rows * (P / n);
    ST3D_CHECK_ARG(local_blocks <= MAX_GRID);
    hipStream_t s = st3d::as_stream(stream);
    uint64_t *words = need ? static_cast<uint64_t *>(workspace) : nullptr;

    if (count) {
        if (weights) swd_count_kernel<<<B, 256, 0, s>>>(weights, N, count);
        else swd_count_all_kernel<<<st3d::cdiv(B, 256), 256, 0, s>>>(B, N, count);
        ST3D_LAUNCH_CHECK();
    }
    swd_sort_local_kernel<<<(unsigned)local_blocks, SORT_THREADS, 0, s>>>(proj, weights, words, K, N, P, 0, 1, P <= SORT_BLOCK,
                                                                          sorted, perm);
    ST3D_LAUNCH_CHECK();
    int h = 1;
    for (long k = 2L * SORT_BLOCK; k <= P; k <<= 1, ++h) {
        swd_sort_strided_kernel<<<(unsigned)local_blocks, SORT_THREADS, 0, s>>>(words, P, k, h);
        ST3D_LAUNCH_CHECK();
        swd_sort_local_kernel<<<(unsigned)local_blocks, SORT_THREADS, 0, s>>>(proj, weights, words, K, N, P, k, 0, k == P, sorted,
                                                                              perm);
        ST3D_LAUNCH_CHECK();
    }
    return ST3D_OK;
}

extern "C" int st3d_swd_loss(const float *sorted, const int32_t *count, const float *tsorted, int B, int Bs, int K, int N, int M,
                             double inv_denom, void *workspace, size_t workspace_bytes, float *loss, st3d_stream_t stream) {
    ST3D_CHECK_ARG(sorted && count && tsorted && loss && workspace);
    ST3D_CHECK_ARG(dims_ok(B, K, N) && M >= 1 && M <= MAX_POS && (Bs == 1 || Bs == B));
    ST3D_CHECK_ARG(workspace_bytes >= (size_t)B * K * 8 && ((uintptr_t)workspace & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    double *partial = static_cast<double *>(workspace);
    const size_t t_stride = Bs == 1 ? 0 : (size_t)K * M;
    swd_loss_rows_kernel<<<(unsigned)((long)B * K), 256, 0, s>>>(sorted, count, tsorted, t_stride, K, N, M, partial);
    ST3D_LAUNCH_CHECK();
    swd_loss_finish_kernel<<<1, 256, 0, s>>>(partial, count, B, K, N, inv_denom, loss);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_swd_bwd(const float *sorted, const int32_t *perm, const int32_t *count, const float *tsorted,
                            const float *grad_out, int B, int Bs, int K, int N, int M, double inv_denom, float *gproj,
                            st3d_stream_t stream) {
    ST3D_CHECK_ARG(sorted && perm && count && tsorted && gproj);
    ST3D_CHECK_ARG(dims_ok(B, K, N) && M >= 1 && M <= MAX_POS && (Bs == 1 || Bs == B));
    const int nblk = st3d::cdiv(N, 256);
    const long blocks = (long)B * K * nblk;
    ST3D_CHECK_ARG(blocks <= MAX_GRID);
    const size_t t_stride = Bs == 1 ? 0 : (size_t)K * M;
    swd_bwd_kernel<<<(unsigned)blocks, 256, 0, st3d::as_stream(stream)>>>(sorted, perm, count, tsorted, t_stride, grad_out, K, N, M,
                                                                         nblk, inv_denom, gproj);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
