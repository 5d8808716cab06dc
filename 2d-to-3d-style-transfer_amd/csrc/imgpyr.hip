// imgpyr.hip -- one step of an image pyramid ("Multi-scale style loss"): a (N,H,W) stack of planes halved with the
// separable tent filter [1 3 3 1] / 8, its exact transpose, and the need mask that travels with it.  For sides >= 4 the
// filter is that of an anti-aliased bilinear resize by 1/2: centred on every 2 x 2 block, no half-pixel shift.
//
//   coarse (i, j) reads fine rows 2i-1 ... 2i+2 and columns 2j-1 ... 2j+2, indices clamped to the plane (replicate border):
//     per row   h = (x[-1] + x[2]) + 3 (x[0] + x[1])
//     then      v = (h[-1] + h[2]) + 3 (h[0] + h[1]),  out = v * (1 / 64)
//   The transpose is a gather: along an axis fine index y has the near coarse index y >> 1 with weight 3 and the far one
//   (y odd: near + 1, y even: near - 1) with weight 1; where the far one falls off the plane the clamp had doubled the
//   border row, and the near weight is 4.  A fine pixel sums its <= 2 x 2 coarse pixels in the order (near, near),
//   (near, far), (far, near), (far, far) over (row, column), each times (wy wx) / 64 (exact in fp32); taps that do not exist
//   are skipped, never multiplied by zero.  No atomics: two runs give the same bits.
//   A coarse pixel is needed iff any pixel of its clamped 4 x 4 footprint is -- so every coarse pixel a needed fine pixel
//   gathers from is needed, and a gradient that is exact at the needed coarse pixels is exact at the needed fine ones.
//
// Tile: one workgroup of 256 threads owns kTileH x kTileW = 8 x 64 coarse pixels, i.e. 16 x 128 fine ones.
//   forward:   the 18 x 130 fine pixels (tile plus a halo of one) go to LDS once, rows read along W; the horizontal pass
//              reads them as float2 pairs (no bank conflicts) into an 18 x 64 LDS plane, the vertical pass reads that by
//              rows and stores 64 consecutive floats per row                                     (9360 + 4608 bytes of LDS)
//   transpose: the 10 x 66 coarse pixels (tile plus halo) go to LDS once; every thread writes eight fine pixels, 128
//              consecutive floats per row                                                                    (2640 bytes)
// Planes whose sides are no multiple of the tile: loads clamp to the plane, stores are guarded.
// Built with -ffp-contract=off: the roundings are the ones written here (tests/_imgpyrref.py restates them in numpy).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileH = 8, kTileW = 64;              // coarse pixels per workgroup
constexpr int kFineH = 2 * kTileH + 2;              // 18 staged fine rows
constexpr int kFineW = 2 * kTileW + 2;              // 130 staged fine columns (even: float2 rows stay aligned)
constexpr int kMaxSide = 32768;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the grid is one-dimensional: block -> (plane, tile row, tile column)
__device__ __forceinline__ void tile_of(int tiles_y, int tiles_x, int &n, int &ty, int &tx) {
    const int b = blockIdx.x;
    tx = b % tiles_x;
    ty = (b / tiles_x) % tiles_y;
    n = b / (tiles_x * tiles_y);
}

__global__ __launch_bounds__(kThreads) void pyr_down_fwd_kernel(const float *__restrict__ in, int H, int W, float *__restrict__ out,
                                                                int tiles_y, int tiles_x) {
    __shared__ __align__(8) float raw[kFineH][kFineW];
    __shared__ float hsum[kFineH][kTileW];
    int n, ty, tx;
    tile_of(tiles_y, tiles_x, n, ty, tx);
    const int Ho = H / 2, Wo = W / 2;
    const int i0 = ty * kTileH, j0 = tx * kTileW;
    const float *plane = in + (size_t)n * H * W;

    // raw[r][c] = fine (2 i0 - 1 + r, 2 j0 - 1 + c), clamped
    for (int t = threadIdx.x; t < kFineH * kFineW; t += kThreads) {
        const int r = t / kFineW, c = t % kFineW;
        const int y = clampi(2 * i0 - 1 + r, 0, H - 1), x = clampi(2 * j0 - 1 + c, 0, W - 1);
        raw[r][c] = plane[(size_t)y * W + x];
    }
    __syncthreads();
    // coarse column j0 + j reads raw columns 2j ... 2j+3: two float2
    for (int t = threadIdx.x; t < kFineH * kTileW; t += kThreads) {
        const int r = t / kTileW, j = t % kTileW;
        const float2 *row = reinterpret_cast<const float2 *>(&raw[r][0]);
        const float2 ab = row[j], cd = row[j + 1];
        hsum[r][j] = (ab.x + cd.y) + 3.f * (ab.y + cd.x);
    }
    __syncthreads();
    // coarse row i0 + i reads hsum rows 2i ... 2i+3
    for (int t = threadIdx.x; t < kTileH * kTileW; t += kThreads) {
        const int i = t / kTileW, j = t % kTileW;
        if (i0 + i < Ho && j0 + j < Wo) {
            const float v = (hsum[2 * i][j] + hsum[2 * i + 3][j]) + 3.f * (hsum[2 * i + 1][j] + hsum[2 * i + 2][j]);
            out[((size_t)n * Ho + (i0 + i)) * Wo + (j0 + j)] = v * 0.015625f;
        }
    }
}

// along one axis: the near coarse index and its weight, the far one and whether it exists (n coarse indices)
__device__ __forceinline__ void axis_taps(int y, int n, int &near, int &far, float &wnear, bool &has_far) {
    near = y >> 1;
    far = (y & 1) ? near + 1 : near - 1;
    has_far = far >= 0 && far < n;
    wnear = has_far ? 3.f : 4.f;
}

__global__ __launch_bounds__(kThreads) void pyr_down_bwd_kernel(const float *__restrict__ gout, int H, int W, float *__restrict__ gin,
                                                                int tiles_y, int tiles_x) {
    __shared__ float g[kTileH + 2][kTileW + 2];
    int n, ty, tx;
    tile_of(tiles_y, tiles_x, n, ty, tx);
    const int Ho = H / 2, Wo = W / 2;
    const int i0 = ty * kTileH, j0 = tx * kTileW;
    const float *plane = gout + (size_t)n * Ho * Wo;

    // g[r][c] = coarse (i0 - 1 + r, j0 - 1 + c); what lies off the plane is loaded clamped and never used
    for (int t = threadIdx.x; t < (kTileH + 2) * (kTileW + 2); t += kThreads) {
        const int r = t / (kTileW + 2), c = t % (kTileW + 2);
        const int i = clampi(i0 - 1 + r, 0, Ho - 1), j = clampi(j0 - 1 + c, 0, Wo - 1);
        g[r][c] = plane[(size_t)i * Wo + j];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 4 * kTileH * kTileW; t += kThreads) {
        const int y = 2 * i0 + t / (2 * kTileW), x = 2 * j0 + t % (2 * kTileW);
        if (y >= H || x >= W) continue;
        int yn, yf, xn, xf;
        float wy, wx;
        bool hy, hx;
        axis_taps(y, Ho, yn, yf, wy, hy);
        axis_taps(x, Wo, xn, xf, wx, hx);
        const int rn = yn - i0 + 1, rf = yf - i0 + 1, cn = xn - j0 + 1, cf = xf - j0 + 1;
        float s = (wy * wx * 0.015625f) * g[rn][cn];
        if (hx) s += (wy * 0.015625f) * g[rn][cf];
        if (hy) s += (wx * 0.015625f) * g[rf][cn];
        if (hy && hx) s += 0.015625f * g[rf][cf];
        gin[((size_t)n * H + y) * W + x] = s;
    }
}

__global__ __launch_bounds__(kThreads) void pyr_down_need_kernel(const uint8_t *__restrict__ need_in, int H, int W,
                                                                 uint8_t *__restrict__ need_out, size_t total) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total) return;
    const int Ho = H / 2, Wo = W / 2;
    const int j = (int)(t % Wo), i = (int)((t / Wo) % Ho);
    const uint8_t *plane = need_in + (t / ((size_t)Wo * Ho)) * (size_t)H * W;
    const int y0 = max(2 * i - 1, 0), y1 = min(2 * i + 2, H - 1), x0 = max(2 * j - 1, 0), x1 = min(2 * j + 2, W - 1);
    bool any = false;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) any |= plane[(size_t)y * W + x] != 0;
    need_out[t] = any ? 1 : 0;
}

inline bool sides_ok(int H, int W) { return H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && H <= kMaxSide && W <= kMaxSide; }

// tiles of all planes, or 0 when they do not fit the one-dimensional grid
inline long grid_blocks(int N, int H, int W, int &tiles_y, int &tiles_x) {
    tiles_y = st3d::cdiv(H / 2, kTileH);
    tiles_x = st3d::cdiv(W / 2, kTileW);
    const long blocks = (long)N * tiles_y * tiles_x;
    return blocks <= 0x7fffffffL ? blocks : 0;
}

}  // namespace

extern "C" int st3d_pyr_down_tile(int *tile_h, int *tile_w) {
    ST3D_CHECK_ARG(tile_h && tile_w);
    *tile_h = 2 * kTileH;
    *tile_w = 2 * kTileW;
    return ST3D_OK;
}

extern "C" int st3d_pyr_down_fwd(const float *in, int N, int H, int W, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(in && out && in != out);
    ST3D_CHECK_ARG(N > 0 && sides_ok(H, W));
    int tiles_y, tiles_x;
    const long blocks = grid_blocks(N, H, W, tiles_y, tiles_x);
    ST3D_CHECK_ARG(blocks > 0);
    pyr_down_fwd_kernel<<<(unsigned)blocks, kThreads, 0, st3d::as_stream(stream)>>>(in, H, W, out, tiles_y, tiles_x);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_pyr_down_bwd(const float *grad_out, int N, int H, int W, float *grad_in, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_out && grad_in && grad_out != grad_in);
    ST3D_CHECK_ARG(N > 0 && sides_ok(H, W));
    int tiles_y, tiles_x;
    const long blocks = grid_blocks(N, H, W, tiles_y, tiles_x);
    ST3D_CHECK_ARG(blocks > 0);
    pyr_down_bwd_kernel<<<(unsigned)blocks, kThreads, 0, st3d::as_stream(stream)>>>(grad_out, H, W, grad_in, tiles_y, tiles_x);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_pyr_down_need(const uint8_t *need_in, int Bn, int H, int W, uint8_t *need_out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(need_in && need_out && need_in != need_out);
    ST3D_CHECK_ARG(Bn > 0 && sides_ok(H, W));
    const size_t total = (size_t)Bn * (H / 2) * (W / 2);
    ST3D_CHECK_ARG(total <= (size_t)0x7fffffff * kThreads);
    pyr_down_need_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, st3d::as_stream(stream)>>>(need_in, H, W, need_out,
                                                                                                             total);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
