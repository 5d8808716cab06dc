// fill.hip -- pull-push fill of a texture map (Gortler et al. 1996; DESIGN 7, "Filling the texels no view moved"): every
// texel that is not `valid` takes a colour interpolated from the valid ones, from as far away as it has to.  A gather with
// fixed-order sums, one integer atomicAdd per wave for the count and no float atomic: two runs give the same bits;
// tests/_fillref.py restates the contract of include/st3d.h in fp64.
//
// Levels: level 0 is the H x W map, level l + 1 has sides ceil(h / 2), ceil(w / 2), down to 1 x 1.  A level entry is one
// float4 (rgb, w).  Level 0 is never stored: it is the select (valid ? (tex, 1) : (0, 0)) of the inputs, formed where it is
// read.  Levels 1...n lie packed in the workspace in that order, 16 B per texel, about H W 16 / 3 bytes in all.
//   fill_pull0:  level 1 from (tex, valid), one thread per coarse texel, up to four (tex, valid) pairs each (13 B) -> 16 B
//   fill_pull:   level l + 1 from level l, while level l + 1 has a side above kTailSide            4 x 16 B -> 16 B
//   fill_tail:   one workgroup takes the first level whose sides are both <= kTailSide = 64 and everything coarser into LDS
//                (at most 64^2 + 32^2 + ... + 1 = 5461 entries = 87376 of the CU's 163840 bytes), runs the remaining pulls
//                and all their pushes there and writes the entries back: one launch where a 1024^2 map would otherwise
//                spend twelve on levels of 64^2 texels and fewer
//   fill_push:   level l completed in place from the completed level l + 1, one thread per fine texel
//   fill_push0:  the last push, fused with the valid / domain select, the write of `out` and the count
// ST3D_FILL_TAIL=0 (read per call) leaves fill_tail out and launches every level on its own; both routes call the same
// pull_texel / push_texel, so they give the same bits.
// Built with -ffp-contract=off and the correctly rounded division, like bake.hip: the roundings are the ones written here.
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int kMaxSide = 16384;             // H W <= 2^28: a texel index fits an int32 with room to spare
constexpr int kMaxLevels = 16;              // 16384 -> 1 takes 14 halvings
constexpr int kThreads = 256;
constexpr int kTailSide = 64;
constexpr int kTailEntries = 5461;          // sum of 4^k, k = 0...6

struct Levels {
    int n;                                  // levels above the map: level n is 1 x 1; 0 for a 1 x 1 map
    int h[kMaxLevels], w[kMaxLevels];       // [0] = the map
    long off[kMaxLevels];                   // entries in front of level l >= 1 in the workspace; off[n + 1] = all of them
};

Levels make_levels(int H, int W) {
    Levels L;
    memset(&L, 0, sizeof(L));
    L.h[0] = H; L.w[0] = W;
    int l = 0;
    while (L.h[l] > 1 || L.w[l] > 1) {
        L.h[l + 1] = (L.h[l] + 1) / 2; L.w[l + 1] = (L.w[l] + 1) / 2;
        L.off[l + 2] = L.off[l + 1] + (long)L.h[l + 1] * L.w[l + 1];
        ++l;
    }
    L.n = l;
    return L;
}

// ---- the two rules, shared by every kernel

// level 0 at (y, x): a select, never a product -- what an invalid texel holds reaches nothing
struct MapSource {
    const float *tex; const uint8_t *valid; int w;
    __device__ __forceinline__ float4 operator()(int y, int x) const {
        const size_t t = (size_t)y * w + x;
        if (!valid[t]) return make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(tex[3 * t], tex[3 * t + 1], tex[3 * t + 2], 1.f);
    }
};

struct LevelSource {
    const float4 *p; int w;
    __device__ __forceinline__ float4 operator()(int y, int x) const { return p[y * w + x]; }
};

// coarse texel (y, x) from the children (2y + dy, 2x + dx) that exist, in the order (0,0), (0,1), (1,0), (1,1):
// W = sum w, C = sum w c; (C / W, min(W, 1)) where W > 0, else (0, 0)
template <class Source>
__device__ __forceinline__ float4 pull_texel(const Source &src, int hs, int ws, int y, int x) {
    float r = 0.f, g = 0.f, b = 0.f, wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = 2 * y + (k >> 1), xx = 2 * x + (k & 1);
        if (yy < hs && xx < ws) {
            const float4 c = src(yy, xx);
            wsum += c.w; r += c.w * c.x; g += c.w * c.y; b += c.w * c.z;
        }
    }
    if (!(wsum > 0.f)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(r / wsum, g / wsum, b / wsum, fminf(wsum, 1.f));
}

// the two taps of the 2x bilinear upsample along one axis for fine index i, clamped to the n coarse texels
__device__ __forceinline__ void axis_taps(int i, int n, int &i0, int &i1, float &a0, float &a1) {
    if (i & 1) { i0 = (i - 1) / 2; i1 = (i + 1) / 2; a0 = 0.75f; a1 = 0.25f; }
    else       { i0 = i / 2 - 1;   i1 = i / 2;       a0 = 0.25f; a1 = 0.75f; }
    i0 = min(max(i0, 0), n - 1); i1 = min(max(i1, 0), n - 1);
}

// fine texel (y, x) holding `own` = (c, w) of the pull: its colour once the coarser level is complete.  w >= 1 keeps c; any
// other takes w c + (1 - w) up, up = the four taps summed in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1)
__device__ __forceinline__ float4 push_texel(const float4 own, const float4 *coarse, int hc, int wc, int y, int x) {
    if (own.w >= 1.f) return own;
    int y0, y1, x0, x1;
    float b0, b1, a0, a1;
    axis_taps(y, hc, y0, y1, b0, b1);
    axis_taps(x, wc, x0, x1, a0, a1);
    const float4 c00 = coarse[y0 * wc + x0], c01 = coarse[y0 * wc + x1], c10 = coarse[y1 * wc + x0], c11 = coarse[y1 * wc + x1];
    const float w00 = b0 * a0, w01 = b0 * a1, w10 = b1 * a0, w11 = b1 * a1;         // sixteenths: exact
    const float ur = w00 * c00.x + w01 * c01.x + w10 * c10.x + w11 * c11.x;
    const float ug = w00 * c00.y + w01 * c01.y + w10 * c10.y + w11 * c11.y;
    const float ub = w00 * c00.z + w01 * c01.z + w10 * c10.z + w11 * c11.z;
    const float keep = own.w, take = 1.f - own.w;
    return make_float4(keep * own.x + take * ur, keep * own.y + take * ug, keep * own.z + take * ub, own.w);
}

// ---- kernels

__global__ __launch_bounds__(kThreads) void fill_pull0_kernel(const float *__restrict__ tex, const uint8_t *__restrict__ valid, int H,
                                                              int W, float4 *__restrict__ dst, int hd, int wd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= hd * wd) return;
    dst[t] = pull_texel(MapSource{tex, valid, W}, H, W, t / wd, t % wd);
}

__global__ __launch_bounds__(kThreads) void fill_pull_kernel(const float4 *__restrict__ src, int hs, int ws, float4 *__restrict__ dst,
                                                             int hd, int wd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= hd * wd) return;
    dst[t] = pull_texel(LevelSource{src, ws}, hs, ws, t / wd, t % wd);
}

__global__ __launch_bounds__(kThreads) void fill_push_kernel(const float4 *__restrict__ coarse, int hc, int wc,
                                                             float4 *__restrict__ fine, int hf, int wf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= hf * wf) return;
    const float4 own = fine[t];
    if (own.w >= 1.f) return;
    fine[t] = push_texel(own, coarse, hc, wc, t / wf, t % wf);
}

// levels first...n of the workspace (entries base[0 .. total)): the pulls above `first`, then every push down to it, in LDS
__global__ __launch_bounds__(kThreads) void fill_tail_kernel(float4 *__restrict__ base, Levels L, int first, int total) {
    __shared__ float4 lds[kTailEntries];
    if (total > kTailEntries) return;           // the host never asks for it
    const long origin = L.off[first];
    const int have = L.h[first] * L.w[first];   // what the pull launches left: level `first` alone
    for (int i = threadIdx.x; i < have; i += kThreads) lds[i] = base[i];
    __syncthreads();
    for (int l = first; l < L.n; ++l) {
        const float4 *src = lds + (L.off[l] - origin);
        float4 *dst = lds + (L.off[l + 1] - origin);
        const int hd = L.h[l + 1], wd = L.w[l + 1];
        for (int i = threadIdx.x; i < hd * wd; i += kThreads) dst[i] = pull_texel(LevelSource{src, L.w[l]}, L.h[l], L.w[l], i / wd, i % wd);
        __syncthreads();
    }
    for (int l = L.n - 1; l >= first; --l) {
        const float4 *coarse = lds + (L.off[l + 1] - origin);
        float4 *fine = lds + (L.off[l] - origin);
        const int hf = L.h[l], wf = L.w[l];
        for (int i = threadIdx.x; i < hf * wf; i += kThreads) fine[i] = push_texel(fine[i], coarse, L.h[l + 1], L.w[l + 1], i / wf, i % wf);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < total; i += kThreads) base[i] = lds[i];
}

// the last push: out = tex bit for bit where valid, outside the domain, or when the map has no valid texel at all (the
// 1 x 1 level `top` has w = 0); the pushed level-0 colour elsewhere, counted once per wave
__global__ __launch_bounds__(kThreads) void fill_push0_kernel(const float *__restrict__ tex, const uint8_t *__restrict__ valid,
                                                              const uint8_t *__restrict__ domain, int H, int W,
                                                              const float4 *__restrict__ coarse, int hc, int wc,
                                                              const float4 *__restrict__ top, float *__restrict__ out,
                                                              unsigned long long *__restrict__ count) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = t < H * W;
    bool take = false;
    if (inside) {
        take = top->w > 0.f && !valid[t] && (domain == nullptr || domain[t]);
        if (take) {
            const float4 c = push_texel(make_float4(0.f, 0.f, 0.f, 0.f), coarse, hc, wc, t / W, t % W);
            out[3 * (size_t)t] = c.x; out[3 * (size_t)t + 1] = c.y; out[3 * (size_t)t + 2] = c.z;
        } else {
            const uint32_t *in = reinterpret_cast<const uint32_t *>(tex);
            uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
            for (int k = 0; k < 3; ++k) o[3 * (size_t)t + k] = in[3 * (size_t)t + k];
        }
    }
    const unsigned long long votes = __ballot(take);
    if ((threadIdx.x & (st3d::kWave - 1)) == 0 && votes) atomicAdd(count, (unsigned long long)__popcll(votes));
}

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool tail_enabled() {
    const char *e = getenv("ST3D_FILL_TAIL");
    return !(e && e[0] == '0' && e[1] == '\0');
}

}  // namespace

extern "C" size_t st3d_fill_workspace_bytes(int H, int W) {
    if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide) return 0;
    const Levels L = make_levels(H, W);
    const long entries = L.off[L.n + 1];
    return sizeof(float4) * (size_t)(entries > 0 ? entries : 1);      // a 1 x 1 map has no level above it: never 0 in range
}

extern "C" int st3d_fill_pushpull(const float *tex, const uint8_t *valid, const uint8_t *domain, int H, int W, void *workspace,
                                  size_t workspace_bytes, float *out, int64_t *count, st3d_stream_t stream) {
    ST3D_CHECK_ARG(tex && valid && workspace && out && count);
    ST3D_CHECK_ARG(H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide);
    ST3D_CHECK_ARG(aligned(workspace, 16) && workspace_bytes >= st3d_fill_workspace_bytes(H, W));
    ST3D_CHECK_ARG(aligned(count, 8) && out != tex);
    hipStream_t s = st3d::as_stream(stream);
    const Levels L = make_levels(H, W);
    ST3D_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    if (L.n == 0) {                             // one texel: valid or not, it is its own answer
        ST3D_HIP(hipMemcpyAsync(out, tex, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
        return ST3D_OK;
    }
    float4 *ws = static_cast<float4 *>(workspace);
    auto level = [&](int l) { return ws + L.off[l]; };
    // the tail takes the first level whose sides both fit kTailSide, and everything above it
    int first = L.n + 1;
    if (tail_enabled())
        for (first = 1; L.h[first] > kTailSide || L.w[first] > kTailSide; ++first) {}
    const int last_pull = first <= L.n ? first : L.n;       // the pull launches build levels 1...last_pull
    fill_pull0_kernel<<<st3d::cdiv((long)L.h[1] * L.w[1], kThreads), kThreads, 0, s>>>(tex, valid, H, W, level(1), L.h[1], L.w[1]);
    for (int l = 2; l <= last_pull; ++l)
        fill_pull_kernel<<<st3d::cdiv((long)L.h[l] * L.w[l], kThreads), kThreads, 0, s>>>(level(l - 1), L.h[l - 1], L.w[l - 1], level(l),
                                                                                         L.h[l], L.w[l]);
    if (first < L.n)                            // (first == n: the 1 x 1 level alone, complete as pulled)
        fill_tail_kernel<<<1, kThreads, 0, s>>>(level(first), L, first, (int)(L.off[L.n + 1] - L.off[first]));
    for (int l = last_pull - 1; l >= 1; --l)    // levels last_pull...n are complete: the tail's, or the 1 x 1 level as pulled
        fill_push_kernel<<<st3d::cdiv((long)L.h[l] * L.w[l], kThreads), kThreads, 0, s>>>(level(l + 1), L.h[l + 1], L.w[l + 1], level(l),
                                                                                         L.h[l], L.w[l]);
    fill_push0_kernel<<<st3d::cdiv((long)H * W, kThreads), kThreads, 0, s>>>(tex, valid, domain, H, W, level(1), L.h[1], L.w[1],
                                                                            level(L.n), out,
                                                                            reinterpret_cast<unsigned long long *>(count));
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
