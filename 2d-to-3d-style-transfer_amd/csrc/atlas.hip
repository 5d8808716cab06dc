// atlas.hip -- per-face texel atlas (PyTorch3D TexturesAtlas) on the hard renderer: nearest-texel lookup in the R x R block
// of the fragment's face + unlit white-ambient shading + the K = 1 softmax blend, forward and backward: the device work of
// TexturesAtlas.sample_textures under SoftPhongShader(AmbientLights) and of its autograd backward.  No UV chart: the colour
// of a covered pixel is
//     texel = atlas[f][wy][wx]                              ((wy, wx) = atlas_texel_index(b0, b1, R), atlas.h)
//     rgb_c = (wnum texel_c + delta 1.0f) / denom           (shadek1.h's blend_k1, the mask as in vcolor.hip's forward)
// and white with mask 0 where there is no face.  Backward, with k = wnum / denom:
//     datlas[f][wy][wx][c] += g_c k   (one deposit per covered pixel);
// the lookup is piecewise constant in the barycentrics and nothing flows through dists / zbuf, so there is no
// gradient towards the vertices.
// HBM-bound like the shade kernels: 24 B of fragments + 16 B written per pixel forward and one 12-byte texel gather per
// covered pixel; 24 + 12 B read backward.
// Built with vcolor.hip's flags (-ffp-contract=off, correctly rounded division): blend and mask are its bits.
#include <type_traits>

#include "atlas.h"
#include "common.h"
#include "det.h"
#include "shadek1.h"
#include "tilebins.h"

namespace {

using namespace st3d_k1;

// one thread per pixel, coalesced per colour plane
__global__ __launch_bounds__(256) void shade_atlas_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                              const float *__restrict__ zbuf, const float *__restrict__ dists,
                                                              const float *__restrict__ atlas, int B, int S, int R,
                                                              float *__restrict__ rgb, float *__restrict__ mask) {
    const size_t HW = (size_t)S * S;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const size_t b = i / HW, p = i - b * HW;
    float *o = rgb + b * 3 * HW + p;
    const int f = p2f[i];
    if (f < 0) {
        o[0] = 1.f; o[HW] = 1.f; o[2 * HW] = 1.f; mask[i] = 0.f;
        return;
    }
    int wy, wx;
    atlas_texel_index(bary[3 * i], bary[3 * i + 1], R, wy, wx);
    const float *t = atlas + (((size_t)f * R + wy) * R + wx) * 3;
    const Blend bl = blend_k1(dists[i], zbuf[i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * HW] = (bl.wnum * t[c] + bl.delta * 1.0f) / bl.denom;
    mask[i] = ((1.0f - (1.0f - bl.prob)) > 0.f) ? 1.f : 0.f;
}

// Atlas backward.  One workgroup per 16x16-pixel tile of one view, the structure of vcolor.hip's shade_vc_bwd_kernel with
// the texel's flat index (f R + wy) R + wx in the vertex's place and one deposit of weight 1 per lane: the contributions of
// a tile are summed per texel in LDS first (the atlas table below: 9 KB + 4 B of LDS in fixed point, 6 KB + 4 B in float)
// and each distinct texel of the tile then costs three global atomics.  A tile in which no pixel has a face leaves after
// one workgroup-wide OR.
// DET 0: float table + float global atomics into gatlas (F,R,R,3).  DET 1: the same binning in 64-bit fixed point (det.h):
// gatlas is the int64 accumulator array and `det` holds the power-of-two scale.
#define ST3D_ATLAS_BINS(name, acc_t) ST3D_TILEBINS(name, acc_t, 1, 512, 256)

template <int DET>
__global__ __launch_bounds__(256) void shade_atlas_bwd_kernel(const float *__restrict__ grad_rgb, const int32_t *__restrict__ p2f,
                                                              const float *__restrict__ bary, const float *__restrict__ zbuf,
                                                              const float *__restrict__ dists, int B, int S, int R, int tiles_x,
                                                              float *__restrict__ gatlas,
                                                              const st3d_det::DetHeader *__restrict__ det) {
    typedef typename std::conditional<DET != 0, unsigned long long, float>::type acc_t;
    ST3D_ATLAS_BINS(bins, acc_t);
    const int tid = threadIdx.x;
    const double dscale = DET ? det->scale : 1.0;
    const size_t HW = (size_t)S * S;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int yi = ty * 16 + (tid >> 4), xi = tx * 16 + (tid & 15);
    const bool in_img = yi < S && xi < S;
    const size_t p = (size_t)yi * S + xi, i = (size_t)b * HW + p;
    const int f = in_img ? p2f[i] : -1;
    if (!__syncthreads_or(f >= 0)) return;           // the same answer in every lane: the whole workgroup leaves
    bins.reset();
    int dep_key[1] = {0};               // this pixel's texel, weight 1, and g k per channel
    const float dep_w[1] = {1.f};
    float dep_g[3] = {0.f, 0.f, 0.f};
    if (f >= 0) {
        int wy, wx;
        atlas_texel_index(bary[3 * i], bary[3 * i + 1], R, wy, wx);
        dep_key[0] = (f * R + wy) * R + wx;          // < F R^2 <= 2^31 - 1 (checked on the host)
        const Blend bl = blend_k1(dists[i], zbuf[i]);
        const float k = bl.wnum / bl.denom;
        const float *g = grad_rgb + (size_t)b * 3 * HW + p;
        dep_g[0] = g[0] * k; dep_g[1] = g[HW] * k; dep_g[2] = g[2 * HW] * k;
    }
    bins.scatter(dep_key, dep_w, dep_g, f >= 0 ? 1u : 0u, dscale, gatlas);
}

// The fixed-point bound of the atlas scatter: partials[block] = sum over the block's grid-stride share of the B*S^2 pixels
// of |g_0| + |g_1| + |g_2| on covered pixels -- every deposit is g_c k with 0 <= k <= 1 and weight 1.  A pixel without a
// face deposits nothing, so its values enter with weight 0, not a skip: finite ones leave the bound -- and with it the
// power-of-two scale -- independent of what a loss wrote on the background, a NaN or an infinity there still poisons it
// (x * 0 = NaN), as in vcolor.hip's vc_abs_sum_kernel.  Fixed order.
__global__ __launch_bounds__(256) void atlas_abs_sum_kernel(const float *__restrict__ g, const int32_t *__restrict__ p2f, int B,
                                                            int S, float *__restrict__ partials) {
    __shared__ float s4[4];
    float acc = 0.f;
    const size_t HW = (size_t)S * S, n = (size_t)B * HW;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / HW, p = i - b * HW;
        const float *gp = g + b * 3 * HW + p;
        const float w = p2f[i] >= 0 ? 1.f : 0.f;
        acc += fabsf(gp[0]) * w;
        acc += fabsf(gp[HW]) * w;
        acc += fabsf(gp[2 * HW]) * w;
    }
    const float t = st3d_det::det_block_sum(acc, s4);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

constexpr int kMaxSide = 4096;      // the rasteriser's limit: fragments exist up to this side
constexpr int kMaxR = 64;
using st3d_det::kPixelPartials;

// 1 <= R <= 64 and F R^2 within the int keys of the tile table
inline bool atlas_dims_ok(int F, int R) {
    return F > 0 && R >= 1 && R <= kMaxR && (long long)F * R * R <= 2147483647ll;
}

}  // namespace

extern "C" int st3d_atlas_texel_index(float b0, float b1, int R, int *wy, int *wx) {
    ST3D_CHECK_ARG(wy && wx);
    ST3D_CHECK_ARG(R >= 1 && R <= kMaxR);
    atlas_texel_index(b0, b1, R, *wy, *wx);
    return ST3D_OK;
}

extern "C" int st3d_shade_atlas_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                    const float *atlas, int B, int S, int F, int R, float *rgb, float *mask,
                                    st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && atlas && rgb && mask);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && atlas_dims_ok(F, R));
    const size_t n = (size_t)B * S * S;
    shade_atlas_fwd_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(pix_to_face, bary, zbuf, dists, atlas,
                                                                                         B, S, R, rgb, mask);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_atlas_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                    const float *dists, int B, int S, int F, int R, float *grad_atlas, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && grad_atlas);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && atlas_dims_ok(F, R));
    const int tiles = (S + 15) / 16;
    shade_atlas_bwd_kernel<0><<<dim3(tiles * tiles, B), 256, 0, st3d::as_stream(stream)>>>(
        grad_rgb, pix_to_face, bary, zbuf, dists, B, S, R, tiles, grad_atlas, nullptr);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_shade_atlas_bwd_det_workspace_bytes(int F, int R) {
    return atlas_dims_ok(F, R) ? st3d_det::workspace_bytes((size_t)F * R * R * 3, kPixelPartials) : 0;
}

extern "C" int st3d_shade_atlas_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                        const float *dists, int B, int S, int F, int R, float *grad_atlas, void *workspace,
                                        size_t workspace_bytes, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && grad_atlas && workspace);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && atlas_dims_ok(F, R));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_shade_atlas_bwd_det_workspace_bytes(F, R) && ((uintptr_t)workspace & 15) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const size_t n_accum = (size_t)F * R * R * 3;
    const st3d_det::DetRun det(workspace, kPixelPartials, n_accum);
    atlas_abs_sum_kernel<<<kPixelPartials, 256, 0, s>>>(grad_rgb, pix_to_face, B, S, det.partials);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    const int tiles = (S + 15) / 16;
    shade_atlas_bwd_kernel<1><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_rgb, pix_to_face, bary, zbuf, dists, B, S, R, tiles,
                                                                     reinterpret_cast<float *>(det.acc), det.hdr);
    ST3D_LAUNCH_CHECK();
    return det.convert(1, grad_atlas, s);
}
