// guide.hip -- the guidance planes of the guided style loss (Gatys et al. 2017, "Controlling Perceptual Factors in
// Neural Style Transfer": the Gram of a tap is taken over the guided region only).  From a coverage mask (n, 1, S, S) in
// [0, 1] to the five planes the weighted Gram kernels read, one per style tap:
//   sides    H_0 = S, H_{l+1} = H_l / 2 (floor, as MaxPool2d: a trailing odd row / column is dropped)
//   a_0 = mask,  a_{l+1}[y][x] = 0.25f * ((a_l[2y][2x] + a_l[2y][2x+1]) + (a_l[2y+1][2x] + a_l[2y+1][2x+1]))
//   Sigma_l  = sum of a_l over the image        (ordered two-stage reduction: bitwise reproducible, no atomics)
//   r_l      = (float)(H_l^2) / Sigma_l, or 0 where Sigma_l is not > 0
//   q_l      = sqrtf(a_l * r_l)                 (the device keeps q: both Gram operands are multiplied by it)
// Division and square root are the correctly rounded ones (the build does not relax them for this file).
// Because the pools floor, pixel (y, x) of level l depends on the aligned 2^l x 2^l block of the mask only: a workgroup
// takes one 16 x 16 tile of the mask through all five levels in LDS, in exactly the pairing written above.
// Two launches: (1) the a_l planes and one partial sum per (level, image, tile); (2) every workgroup sums the partials
// of its (level, image) in one fixed order and turns its share of the plane into q.
#include "common.h"

namespace {

constexpr int kLevels = 5;
constexpr int kTile = 16;

struct GuideArgs {
    const float *mask; float *q; float *sums; float *partials;
    int n, S, tiles;                     // tiles per side of the mask
    int H[kLevels];
    size_t off[kLevels];                 // start of level l in q (elements)
};

// sum of v[0..m) (m a power of two <= 256) in a fixed tree; every thread of the workgroup calls it
__device__ __forceinline__ float tree_sum(float *red, float mine, int m) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = t < m ? mine : 0.f;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void guide_pyramid_kernel(const GuideArgs g) {
    __shared__ float lv[2][kTile * kTile];
    __shared__ float red[256];
    const int t = threadIdx.x, b = blockIdx.y;
    const int ty = blockIdx.x / g.tiles, tx = blockIdx.x % g.tiles;
    float *partials = g.partials + ((size_t)b * g.tiles * g.tiles + blockIdx.x);
    const size_t pstride = (size_t)g.n * g.tiles * g.tiles;         // partials: [level][image][tile]
    float v = 0.f;
    {
        const int y = ty * kTile + (t >> 4), x = tx * kTile + (t & 15);
        if (y < g.S && x < g.S) {
            v = g.mask[((size_t)b * g.S + y) * g.S + x];
            g.q[g.off[0] + ((size_t)b * g.S + y) * g.S + x] = v;
        }
    }
    lv[0][t] = v;
    const float s0 = tree_sum(red, v, 256);
    if (t == 0) partials[0] = s0;
#pragma unroll
    for (int l = 1; l < kLevels; ++l) {
        const int side = kTile >> l, H = g.H[l];
        const float *src = lv[(l - 1) & 1];
        float *dst = lv[l & 1];
        v = 0.f;
        if (t < side * side) {
            const int yy = t / side, xx = t % side;
            const int y = ty * side + yy, x = tx * side + xx;
            // a pixel inside level l has all four children inside level l - 1 (2 H_l <= H_{l-1})
            if (y < H && x < H) {
                const int ps = side * 2;
                v = 0.25f * ((src[(2 * yy) * ps + 2 * xx] + src[(2 * yy) * ps + 2 * xx + 1]) +
                             (src[(2 * yy + 1) * ps + 2 * xx] + src[(2 * yy + 1) * ps + 2 * xx + 1]));
                g.q[g.off[l] + ((size_t)b * H + y) * H + x] = v;
            }
            dst[t] = v;
        }
        const float sl = tree_sum(red, v, side * side);        // (its barriers also order dst's writes before the next level's reads)
        if (t == 0) partials[l * pstride] = sl;
    }
}

constexpr int kChunk = 4096;            // plane elements per workgroup of the second launch

__global__ __launch_bounds__(256) void guide_scale_kernel(const GuideArgs g) {
    __shared__ float red[256];
    const int t = threadIdx.x, b = blockIdx.y, l = blockIdx.z;
    const int H = g.H[l];
    const size_t HH = (size_t)H * H, first = (size_t)blockIdx.x * kChunk;
    if (first >= HH && !(blockIdx.x == 0)) return;       // (uniform per workgroup; a level of side 0 still reports its sum)
    const int T = g.tiles * g.tiles;
    const float *p = g.partials + ((size_t)l * g.n + b) * T;
    float s = 0.f;
    for (int i = t; i < T; i += 256) s += p[i];          // ascending, then the fixed tree: the same bits in every workgroup
    const float sigma = tree_sum(red, s, 256);
    const float r = sigma > 0.f ? (float)HH / sigma : 0.f;
    if (blockIdx.x == 0 && t == 0) g.sums[l * g.n + b] = sigma;
    float *q = g.q + g.off[l] + (size_t)b * HH;
    for (int k = 0; k < kChunk / 256; ++k) {
        const size_t i = first + (size_t)k * 256 + t;
        if (i < HH) q[i] = sqrtf(q[i] * r);
    }
}

int fill_args(GuideArgs &g, int n, int S) {
    memset(&g, 0, sizeof(g));
    g.n = n; g.S = S; g.tiles = st3d::cdiv(S, kTile);
    size_t off = 0;
    int H = S;
    for (int l = 0; l < kLevels; ++l) {
        g.H[l] = H; g.off[l] = off;
        off += (size_t)n * H * H;
        H /= 2;
    }
    return 0;
}

}  // namespace

extern "C" size_t st3d_guidance_floats(int n, int S) {
    if (n <= 0 || S < kTile) return 0;
    size_t tot = 0;
    for (int l = 0, H = S; l < kLevels; ++l, H /= 2) tot += (size_t)n * H * H;
    return tot;
}

extern "C" size_t st3d_guidance_partials(int n, int S) {
    if (n <= 0 || S < kTile) return 0;
    const size_t t = (size_t)st3d::cdiv(S, kTile);
    return (size_t)kLevels * n * t * t;
}

extern "C" int st3d_guidance_build(const float *mask, int n, int S, float *q_out, float *sums_out, float *partials,
                                   st3d_stream_t stream) {
    ST3D_CHECK_ARG(mask && q_out && sums_out && partials);
    ST3D_CHECK_ARG(n > 0 && n <= 65535);
    ST3D_CHECK_ARG(S >= 16 && S <= 16384);
    GuideArgs g;
    fill_args(g, n, S);
    g.mask = mask; g.q = q_out; g.sums = sums_out; g.partials = partials;
    hipStream_t s = st3d::as_stream(stream);
    guide_pyramid_kernel<<<dim3(g.tiles * g.tiles, n), 256, 0, s>>>(g);
    ST3D_LAUNCH_CHECK();
    guide_scale_kernel<<<dim3(st3d::cdiv((long)S * S, kChunk), n, kLevels), 256, 0, s>>>(g);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
