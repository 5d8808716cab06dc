// cover.hip -- which texels of a T x T map each view touches, and a greedy choice of views by what each adds (DESIGN 7,
// "Coverage-driven view selection").  Integer work throughout: bit masks, population counts and an integer atomic OR, so
// every result is the same bits from run to run and equal to its numpy restatement (tests/_coverref.py).
//
// A mask is W = (T*T + 31) / 32 words per view; texel (row r, column x) of the map as stored is bit (r*T + x) & 31 of word
// (r*T + x) >> 5.  A texel is marked when shade_bwd of a positive gradient would add a non-zero weight to it: the four
// texels of the pixel's bilinear footprint (shadek1.h) that are inside the map and whose two weights are both > 0.
//   cover_mark:   24 B of fragments read per pixel, at most four atomic ORs per covered pixel into 4 W bytes per view
//                 (neighbouring pixels hit the same words: the word is read first and the atomic issued only for a clear bit)
//   cover_gain:   one workgroup per candidate reads its W words and the W covered words once (16-byte loads when W % 4 == 0)
//   cover_pick:   one workgroup: arg-max over <= 4096 gains, then covered |= the picked row
//   cover_count:  one thread per texel walks the C rows (the 32 texels of a word share one broadcast load)
// Built with -ffp-contract=off and the correctly rounded division: the footprint is shade.hip's, bit for bit.
#include "common.h"
#include "shadek1.h"

namespace {

using namespace st3d_k1;

constexpr int kMaxCandidates = 4096;
constexpr int kMaxSide = 16384;             // T*T <= 2^28: a texel index and a gain fit an int32 with room to spare
constexpr int kThreads = 256, kWaves = kThreads / st3d::kWave;

__device__ __forceinline__ void mark_texel(uint32_t *__restrict__ row, int T, int r, int x) {
    const uint32_t t = (uint32_t)r * (uint32_t)T + (uint32_t)x;
    uint32_t *w = row + (t >> 5);
    const uint32_t bit = 1u << (t & 31);
    if (!(*w & bit)) atomicOr(w, bit);      // bits are only ever set: a stale read costs one redundant atomic, never a bit
}

__global__ __launch_bounds__(kThreads) void cover_mark_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                              const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                                              int B, int S, int T, int W, uint32_t *__restrict__ masks) {
    const size_t HW = (size_t)S * S;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const int f = p2f[i];
    if (f < 0) return;
    const FragUV t = frag_uv(uvs, fuv, f, bary[3 * i], bary[3 * i + 1], bary[3 * i + 2]);
    const Footprint q = uv_footprint(t.u, t.v, T);
    uint32_t *row = masks + (i / HW) * (size_t)W;
    const bool x0 = q.vx0 && q.wx0 > 0.f, x1 = q.vx1 && q.wx1 > 0.f;
    const bool y0 = q.vy0 && q.wy0 > 0.f, y1 = q.vy1 && q.wy1 > 0.f;
    if (y0 && x0) mark_texel(row, T, q.r0, q.x0);
    if (y0 && x1) mark_texel(row, T, q.r0, q.x1);
    if (y1 && x0) mark_texel(row, T, q.r1, q.x0);
    if (y1 && x1) mark_texel(row, T, q.r1, q.x1);
}

// sum of `v` over the workgroup, valid in thread 0: xor-shuffles inside each wave of 64, the waves through LDS
__device__ __forceinline__ int block_sum(int v, int *lds) {
#pragma unroll
    for (int o = st3d::kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & (st3d::kWave - 1), wave = threadIdx.x / st3d::kWave;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    int s = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kWaves; ++k) s += lds[k];
    }
    return s;
}

// gain[c] = sum_w popcount(masks[c][w] & ~covered[w]); a taken candidate is skipped (cover_pick never reads its gain)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void cover_gain_kernel(const uint32_t *__restrict__ masks, const uint32_t *__restrict__ covered,
                                                              int W, const int32_t *__restrict__ taken, int32_t *__restrict__ gain) {
    __shared__ int lds[kWaves];
    const int c = blockIdx.x;
    if (taken[c]) return;
    const uint32_t *row = masks + (size_t)c * W;
    int n = 0;
    if (VEC) {                  // W % 4 == 0 and both bases 16-byte aligned: every row starts on a 16-byte boundary
        const uint4 *r4 = reinterpret_cast<const uint4 *>(row), *c4 = reinterpret_cast<const uint4 *>(covered);
        for (int w = threadIdx.x; w < W / 4; w += kThreads) {
            const uint4 m = r4[w], k = c4[w];
            n += __popc(m.x & ~k.x) + __popc(m.y & ~k.y) + __popc(m.z & ~k.z) + __popc(m.w & ~k.w);
        }
    } else {
        for (int w = threadIdx.x; w < W; w += kThreads) n += __popc(row[w] & ~covered[w]);
    }
    n = block_sum(n, lds);
    if (threadIdx.x == 0) gain[c] = n;
}

// round k: the untaken candidate of the largest gain, the lowest index among equals -> picks[k], gains[k]; covered |= its row
__global__ __launch_bounds__(kThreads) void cover_pick_kernel(const uint32_t *__restrict__ masks, int C, int W, int k,
                                                              const int32_t *__restrict__ gain, int32_t *__restrict__ taken,
                                                              uint32_t *__restrict__ covered, int32_t *__restrict__ picks,
                                                              int32_t *__restrict__ gains) {
    __shared__ int lds_g[kWaves], lds_c[kWaves], best;
    int g = -1, at = C;         // (-1, C): no candidate; every real gain is >= 0
    for (int c = threadIdx.x; c < C; c += kThreads) {       // ascending c: a later equal gain does not replace an earlier one
        if (taken[c]) continue;
        const int gc = gain[c];
        if (gc > g) { g = gc; at = c; }
    }
#pragma unroll
    for (int o = st3d::kWave / 2; o > 0; o >>= 1) {
        const int og = __shfl_xor(g, o), oc = __shfl_xor(at, o);
        if (og > g || (og == g && oc < at)) { g = og; at = oc; }
    }
    const int lane = threadIdx.x & (st3d::kWave - 1), wave = threadIdx.x / st3d::kWave;
    if (lane == 0) { lds_g[wave] = g; lds_c[wave] = at; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kWaves; ++j)
            if (lds_g[j] > g || (lds_g[j] == g && lds_c[j] < at)) { g = lds_g[j]; at = lds_c[j]; }
        best = at;              // n <= C: an untaken candidate always exists
        picks[k] = at;
        gains[k] = g;
        taken[at] = 1;
    }
    __syncthreads();
    const uint32_t *row = masks + (size_t)best * W;
    for (int w = threadIdx.x; w < W; w += kThreads) covered[w] |= row[w];
}

__global__ __launch_bounds__(kThreads) void cover_count_kernel(const uint32_t *__restrict__ masks, int C, int W, int TT,
                                                               int32_t *__restrict__ counts) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= TT) return;
    const uint32_t *col = masks + (t >> 5);
    const int sh = t & 31;
    int n = 0;
    for (int c = 0; c < C; ++c) n += (int)((col[(size_t)c * W] >> sh) & 1u);
    counts[t] = n;
}

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int words_of(int T) { return (int)(((long)T * T + 31) / 32); }

}  // namespace

extern "C" int st3d_cover_mark(const int32_t *pix_to_face, const float *bary, const float *verts_uvs, const int32_t *faces_uvs,
                               int B, int S, int T, void *masks, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && verts_uvs && faces_uvs && masks);
    ST3D_CHECK_ARG(B >= 1 && S >= 1 && S <= 4096 && T >= 1 && T <= kMaxSide);
    ST3D_CHECK_ARG(aligned(masks, 4));
    const size_t n = (size_t)B * S * S;
    ST3D_CHECK_ARG(n <= (size_t)0x7fffffff * kThreads);
    cover_mark_kernel<<<st3d::cdiv((long)n, kThreads), kThreads, 0, st3d::as_stream(stream)>>>(
        pix_to_face, bary, verts_uvs, faces_uvs, B, S, T, words_of(T), static_cast<uint32_t *>(masks));
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_cover_workspace_bytes(int C) {
    return (C >= 1 && C <= kMaxCandidates) ? (size_t)C * 2 * sizeof(int32_t) : 0;
}

extern "C" int st3d_cover_greedy(const void *masks, int C, int W, int n, void *covered, int32_t *picks, int32_t *gains,
                                 void *workspace, st3d_stream_t stream) {
    ST3D_CHECK_ARG(masks && covered && picks && gains && workspace);
    ST3D_CHECK_ARG(C >= 1 && C <= kMaxCandidates && n >= 1 && n <= C);
    ST3D_CHECK_ARG(W >= 1 && W <= (1 << 26));           // 32 W: the largest gain, an int32
    ST3D_CHECK_ARG(aligned(masks, 4) && aligned(covered, 4) && aligned(workspace, 4));
    ST3D_CHECK_ARG(masks != covered);
    hipStream_t s = st3d::as_stream(stream);
    int32_t *gain = static_cast<int32_t *>(workspace), *taken = gain + C;
    const uint32_t *m = static_cast<const uint32_t *>(masks);
    uint32_t *cov = static_cast<uint32_t *>(covered);
    const bool vec = W % 4 == 0 && aligned(masks, 16) && aligned(covered, 16);
    ST3D_HIP(hipMemsetAsync(taken, 0, (size_t)C * sizeof(int32_t), s));
    for (int k = 0; k < n; ++k) {
        if (vec) cover_gain_kernel<true><<<C, kThreads, 0, s>>>(m, cov, W, taken, gain);
        else cover_gain_kernel<false><<<C, kThreads, 0, s>>>(m, cov, W, taken, gain);
        cover_pick_kernel<<<1, kThreads, 0, s>>>(m, C, W, k, gain, taken, cov, picks, gains);
    }
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_cover_count(const void *masks, int C, int W, int T, int32_t *counts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(masks && counts);
    ST3D_CHECK_ARG(C >= 1 && T >= 1 && T <= kMaxSide && W == words_of(T));
    ST3D_CHECK_ARG(aligned(masks, 4));
    const int TT = T * T;
    cover_count_kernel<<<st3d::cdiv(TT, kThreads), kThreads, 0, st3d::as_stream(stream)>>>(
        static_cast<const uint32_t *>(masks), C, W, TT, counts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
