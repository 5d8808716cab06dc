// regions.hip -- the guidance planes of several mesh regions at once (--style_regions: Gatys et al. 2017, spatial control
// with one style per region).  From the fragments of a render, pix_to_face (n, S, S), and one label per face to the planes
// guide.hip builds for the R one-hot masks
//   a_0[r][p] = 1 where pix_to_face[p] >= 0 and face_region[pix_to_face[p]] == r, else 0
// without any (n, R, S, S) mask in memory.  Everything behind a_0 is guide.hip's arithmetic in its pairing and order -- the
// floor 2 x 2 means, the tree over the 256 values of a tile, the ascending sum of the tile partials and the same tree, the
// correctly rounded division and square root (the build gives this file guide.hip's flags) -- so region r's block of q_out
// holds bit for bit what st3d_guidance_build writes for that mask.
// A workgroup takes one 16 x 16 tile of one image: it reads pix_to_face once, gathers the labels and carries all R regions
// through the five levels in LDS side by side (one barrier sequence for all of them).  Two launches, no atomics.
#include "common.h"

namespace {

constexpr int kLevels = 5;
constexpr int kTile = 16;
constexpr int kMaxRegions = 8;
constexpr int kNone = 255;               // the label of a pixel without a face (no region has it: R <= 8)

struct RegionArgs {
    const int32_t *p2f; const uint8_t *labels; float *q; float *sums; float *partials;
    int n, S, F, R, tiles;               // tiles per side of the image
    int H[kLevels];
    size_t off[kLevels];                 // start of level l inside a region's block of q (elements)
    size_t qstride, pstride;             // a region's block of q / of partials (elements)
};

// guide.hip's tree_sum for R rows at once: row r sums v[r][0..m) (m a power of two <= 256) in the same fixed tree;
// every thread of the workgroup calls it.  The sums are left in red[r][0].
__device__ __forceinline__ void tree_sums(float (*red)[256], const float *mine, int m, int R) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kMaxRegions; ++r)      // (unrolled: `mine` stays in registers)
        if (r < R) red[r][t] = t < m ? mine[r] : 0.f;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            for (int r = 0; r < R; ++r) red[r][t] += red[r][t + o];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void region_pyramid_kernel(const RegionArgs g) {
    __shared__ float lv[2][kMaxRegions][kTile * kTile];
    __shared__ float red[kMaxRegions][256];
    const int t = threadIdx.x, b = blockIdx.y, R = g.R;
    const int ty = blockIdx.x / g.tiles, tx = blockIdx.x % g.tiles;
    const size_t lstride = (size_t)g.n * g.tiles * g.tiles;         // a region's partials: [level][image][tile]
    float *partials = g.partials + ((size_t)b * g.tiles * g.tiles + blockIdx.x);
    float v[kMaxRegions];
    {
        const int y = ty * kTile + (t >> 4), x = tx * kTile + (t & 15);
        const bool in = y < g.S && x < g.S;
        int label = kNone;
        if (in) {
            const int f = g.p2f[((size_t)b * g.S + y) * g.S + x];
            if (f >= 0 && f < g.F) label = g.labels[f];
        }
#pragma unroll
        for (int r = 0; r < kMaxRegions; ++r) {
            v[r] = label == r ? 1.f : 0.f;
            if (r < R) {
                if (in) g.q[r * g.qstride + g.off[0] + ((size_t)b * g.S + y) * g.S + x] = v[r];
                lv[0][r][t] = v[r];
            }
        }
    }
    tree_sums(red, v, 256, R);
    if (t < R) partials[t * g.pstride] = red[t][0];
#pragma unroll
    for (int l = 1; l < kLevels; ++l) {
        const int side = kTile >> l, H = g.H[l];
        const int yy = t / side, xx = t % side;
        const int y = ty * side + yy, x = tx * side + xx;
        // a pixel inside level l has all four children inside level l - 1 (2 H_l <= H_{l-1})
        const bool mine = t < side * side, in = mine && y < H && x < H;
#pragma unroll
        for (int r = 0; r < kMaxRegions; ++r) {
            v[r] = 0.f;
            if (r < R && mine) {
                const float *src = lv[(l - 1) & 1][r];
                if (in) {
                    const int ps = side * 2;
                    v[r] = 0.25f * ((src[(2 * yy) * ps + 2 * xx] + src[(2 * yy) * ps + 2 * xx + 1]) +
                                    (src[(2 * yy + 1) * ps + 2 * xx] + src[(2 * yy + 1) * ps + 2 * xx + 1]));
                    g.q[r * g.qstride + g.off[l] + ((size_t)b * H + y) * H + x] = v[r];
                }
                lv[l & 1][r][t] = v[r];
            }
        }
        tree_sums(red, v, side * side, R);      // (its barriers also order this level's writes before the next level's reads)
        if (t < R) partials[t * g.pstride + l * lstride] = red[t][0];
    }
}

constexpr int kChunk = 4096;            // plane elements per workgroup of the second launch

// guide.hip's guide_scale_kernel with the region in blockIdx.z: z = r * kLevels + l
__global__ __launch_bounds__(256) void region_scale_kernel(const RegionArgs g) {
    __shared__ float red[256];
    const int t = threadIdx.x, b = blockIdx.y, l = blockIdx.z % kLevels, r = blockIdx.z / kLevels;
    const int H = g.H[l];
    const size_t HH = (size_t)H * H, first = (size_t)blockIdx.x * kChunk;
    if (first >= HH && !(blockIdx.x == 0)) return;       // (uniform per workgroup; a level of side 0 still reports its sum)
    const int T = g.tiles * g.tiles;
    const float *p = g.partials + r * g.pstride + ((size_t)l * g.n + b) * T;
    float s = 0.f;
    for (int i = t; i < T; i += 256) s += p[i];          // ascending, then the fixed tree: the same bits in every workgroup
    __syncthreads();
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const float sigma = red[0];
    const float ratio = sigma > 0.f ? (float)HH / sigma : 0.f;
    if (blockIdx.x == 0 && t == 0) g.sums[((size_t)r * kLevels + l) * g.n + b] = sigma;
    float *q = g.q + r * g.qstride + g.off[l] + (size_t)b * HH;
    for (int k = 0; k < kChunk / 256; ++k) {
        const size_t i = first + (size_t)k * 256 + t;
        if (i < HH) q[i] = sqrtf(q[i] * ratio);
    }
}

}  // namespace

extern "C" size_t st3d_region_planes_floats(int n, int S, int R) {
    if (R < 1 || R > kMaxRegions) return 0;
    return (size_t)R * st3d_guidance_floats(n, S);
}

extern "C" size_t st3d_region_planes_partials(int n, int S, int R) {
    if (R < 1 || R > kMaxRegions) return 0;
    return (size_t)R * st3d_guidance_partials(n, S);
}

extern "C" int st3d_region_planes(const int32_t *pix_to_face, const uint8_t *face_region, int n, int S, int F, int R,
                                  float *q_out, float *sums_out, float *partials, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && face_region && q_out && sums_out && partials);
    ST3D_CHECK_ARG(n > 0 && n <= 65535);
    ST3D_CHECK_ARG(S >= 16 && S <= 16384);
    ST3D_CHECK_ARG(F > 0);
    ST3D_CHECK_ARG(R >= 1 && R <= kMaxRegions);
    RegionArgs g;
    memset(&g, 0, sizeof(g));
    g.p2f = pix_to_face; g.labels = face_region; g.q = q_out; g.sums = sums_out; g.partials = partials;
    g.n = n; g.S = S; g.F = F; g.R = R; g.tiles = st3d::cdiv(S, kTile);
    size_t off = 0;
    for (int l = 0, H = S; l < kLevels; ++l, H /= 2) {
        g.H[l] = H; g.off[l] = off;
        off += (size_t)n * H * H;
    }
    g.qstride = st3d_guidance_floats(n, S);
    g.pstride = st3d_guidance_partials(n, S);
    hipStream_t s = st3d::as_stream(stream);
    region_pyramid_kernel<<<dim3(g.tiles * g.tiles, n), 256, 0, s>>>(g);
    ST3D_LAUNCH_CHECK();
    region_scale_kernel<<<dim3(st3d::cdiv((long)S * S, kChunk), n, kLevels * R), 256, 0, s>>>(g);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
