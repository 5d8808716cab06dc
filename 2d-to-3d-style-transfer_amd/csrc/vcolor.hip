// vcolor.hip -- per-vertex colours (PyTorch3D TexturesVertex) on the hard renderer: barycentric interpolation of a (V,3)
// colour array + unlit white-ambient shading + the K = 1 softmax blend, forward and backward: the device work of
// TexturesVertex.sample_textures / interpolate_face_attributes under SoftPhongShader(AmbientLights) and of their autograd
// backward.  No UV atlas and no texture map: the colour of a covered pixel is
//     t_c = b0 C[v0][c] + b1 C[v1][c] + b2 C[v2][c]        (v_i = faces[f][i], left to right, no contraction)
//     rgb_c = (wnum t_c + delta 1.0f) / denom               (shadek1.h's blend_k1, the mask as in shade.hip's shade_fwd_kernel)
// and white with mask 0 where there is no face.  Backward, with k = wnum / denom and gk_c = g_c k:
//     dC[v_i][c] += b_i gk_c  (nine deposits per covered pixel),   db_i = sum_c gk_c C[v_i][c]  (0 on uncovered pixels);
// nothing flows through dists / zbuf (as on the UV path).
// HBM-bound like the shade kernels: 24 B of fragments + 16 B written per pixel forward (the three face indices and nine
// colour floats of a covered pixel come from L2: 35 KB of colours for the cow), 24 + 12 B read backward.
// Built with shade.hip's flags (-ffp-contract=off, correctly rounded division): blend and mask are its bits.
#include <type_traits>

#include "common.h"
#include "det.h"
#include "shadek1.h"
#include "tilebins.h"

namespace {

using namespace st3d_k1;

// one thread per pixel, coalesced per colour plane
__global__ __launch_bounds__(256) void shade_vc_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                           const float *__restrict__ zbuf, const float *__restrict__ dists,
                                                           const int32_t *__restrict__ faces, const float *__restrict__ col,
                                                           int B, int S, float *__restrict__ rgb, float *__restrict__ mask) {
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
    const float b0 = bary[3 * i], b1 = bary[3 * i + 1], b2 = bary[3 * i + 2];
    const float *c0 = col + (size_t)faces[3 * f] * 3, *c1 = col + (size_t)faces[3 * f + 1] * 3;
    const float *c2 = col + (size_t)faces[3 * f + 2] * 3;
    const Blend bl = blend_k1(dists[i], zbuf[i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = b0 * c0[c] + b1 * c1[c] + b2 * c2[c];
        o[c * HW] = (bl.wnum * t + bl.delta * 1.0f) / bl.denom;
    }
    mask[i] = ((1.0f - (1.0f - bl.prob)) > 0.f) ? 1.f : 0.f;
}

// Colour backward.  One workgroup per 16x16-pixel tile of one view, the structure of shade.hip's shade_bwd_kernel with the
// vertex index in the texel's place: the nine contributions of a pixel are summed per vertex in LDS first (the vertex table
// of tilebins.h: 29 KB + 4 B of LDS in fixed point, 20 KB + 4 B in float) and each distinct vertex of the tile then costs
// three global atomics.  A tile in which no pixel has a face writes its zero rows of gbary and leaves (one workgroup-wide OR).
// DET 0: float table + float global atomics into gcol (V,3).  DET 1: the same binning in 64-bit fixed point (det.h): gcol is
// the int64 accumulator array and `det` holds the power-of-two scale.  gcol == nullptr (the vertices alone are optimised):
// no table, gbary only.
template <int DET>
__global__ __launch_bounds__(256) void shade_vc_bwd_kernel(const float *__restrict__ grad_rgb, const int32_t *__restrict__ p2f,
                                                           const float *__restrict__ bary, const float *__restrict__ zbuf,
                                                           const float *__restrict__ dists, const int32_t *__restrict__ faces,
                                                           const float *__restrict__ col, int B, int S, int tiles_x,
                                                           float *__restrict__ gcol, float *__restrict__ gbary,
                                                           const st3d_det::DetHeader *__restrict__ det) {
    typedef typename std::conditional<DET != 0, unsigned long long, float>::type acc_t;
    ST3D_VERTEX_BINS(bins, acc_t);
    const int tid = threadIdx.x;
    const double dscale = DET ? det->scale : 1.0;
    const size_t HW = (size_t)S * S;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int yi = ty * 16 + (tid >> 4), xi = tx * 16 + (tid & 15);
    const bool in_img = yi < S && xi < S;
    const size_t p = (size_t)yi * S + xi, i = (size_t)b * HW + p;
    const int f = in_img ? p2f[i] : -1;
    if (in_img && f < 0 && gbary) { gbary[3 * i] = 0.f; gbary[3 * i + 1] = 0.f; gbary[3 * i + 2] = 0.f; }
    if (gcol) {
        if (!__syncthreads_or(f >= 0)) return;           // the same answer in every lane: the whole workgroup leaves
        bins.reset();
    }
    int dep_vert[3] = {0, 0, 0};        // this pixel's three vertices, their barycentric weights and g k per channel
    float dep_w[3] = {0.f, 0.f, 0.f}, dep_g[3] = {0.f, 0.f, 0.f};
    if (f >= 0) {
        const float bw[3] = {bary[3 * i], bary[3 * i + 1], bary[3 * i + 2]};
        const Blend bl = blend_k1(dists[i], zbuf[i]);
        const float k = bl.wnum / bl.denom;
        const float *g = grad_rgb + (size_t)b * 3 * HW + p;
        const float gk[3] = {g[0] * k, g[HW] * k, g[2 * HW] * k};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int v = faces[3 * f + j];
            dep_vert[j] = v; dep_w[j] = bw[j];
            if (gbary) {
                const float *c = col + (size_t)v * 3;
                gbary[3 * i + j] = gk[0] * c[0] + gk[1] * c[1] + gk[2] * c[2];
            }
        }
        dep_g[0] = gk[0]; dep_g[1] = gk[1]; dep_g[2] = gk[2];
    }
    if (gcol) bins.scatter(dep_vert, dep_w, dep_g, f >= 0 ? 7u : 0u, dscale, gcol);
}

// The fixed-point bound of the colour scatter: partials[block] = sum over the block's grid-stride share of the B*S^2 pixels
// of (|g_0| + |g_1| + |g_2|) max(1, max_i |b_i|) -- every deposit is g_c k b_i with 0 <= k <= 1, and the fragment buffers
// may hold barycentrics outside (0,1), so the weight bound of the texel scatter (<= 1) is not assumed.  (A vertex that is
// two or three corners of one face takes up to three deposits of a pixel; the scale leaves 2^3 of headroom above the bound.)
// A pixel without a face deposits nothing, so its values enter with weight 0: finite ones leave the bound -- and with it the
// power-of-two scale -- independent of what a loss wrote on the background, a NaN or an infinity there still poisons it
// (x * 0 = NaN), as in shade.hip's ss_abs_sum_kernel.  Fixed order.
__global__ __launch_bounds__(256) void vc_abs_sum_kernel(const float *__restrict__ g, const int32_t *__restrict__ p2f,
                                                         const float *__restrict__ bary, int B, int S,
                                                         float *__restrict__ partials) {
    __shared__ float s4[4];
    float acc = 0.f;
    const size_t HW = (size_t)S * S, n = (size_t)B * HW;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / HW, p = i - b * HW;
        const float *gp = g + b * 3 * HW + p;
        float w = 0.f;
        if (p2f[i] >= 0) {
            w = 1.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float a = fabsf(bary[3 * i + j]);
                if (a > w || a != a) w = a;          // (a NaN barycentric poisons the bound too)
            }
        }
        acc += fabsf(gp[0]) * w;
        acc += fabsf(gp[HW]) * w;
        acc += fabsf(gp[2 * HW]) * w;
    }
    const float t = st3d_det::det_block_sum(acc, s4);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

constexpr int kMaxSide = 4096;      // the rasteriser's limit: fragments exist up to this side
using st3d_det::kPixelPartials;

}  // namespace

extern "C" int st3d_shade_vc_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                 const int32_t *faces, const float *verts_colors, int B, int S, int F, int V, float *rgb,
                                 float *mask, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && faces && verts_colors && rgb && mask);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && F > 0 && V > 0);
    const size_t n = (size_t)B * S * S;
    shade_vc_fwd_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(pix_to_face, bary, zbuf, dists, faces,
                                                                                      verts_colors, B, S, rgb, mask);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_vc_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                 const float *dists, const int32_t *faces, const float *verts_colors, int B, int S, int F,
                                 int V, float *grad_colors, float *grad_bary, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && faces && verts_colors);
    ST3D_CHECK_ARG(grad_colors || grad_bary);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && F > 0 && V > 0);
    const int tiles = (S + 15) / 16;
    shade_vc_bwd_kernel<0><<<dim3(tiles * tiles, B), 256, 0, st3d::as_stream(stream)>>>(
        grad_rgb, pix_to_face, bary, zbuf, dists, faces, verts_colors, B, S, tiles, grad_colors, grad_bary, nullptr);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_shade_vc_bwd_det_workspace_bytes(int V) {
    return V > 0 ? st3d_det::workspace_bytes((size_t)V * 3, kPixelPartials) : 0;
}

extern "C" int st3d_shade_vc_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                     const float *dists, const int32_t *faces, const float *verts_colors, int B, int S, int F,
                                     int V, float *grad_colors, float *grad_bary, void *workspace, size_t workspace_bytes,
                                     st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && faces && verts_colors && workspace);
    ST3D_CHECK_ARG(grad_colors);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxSide && F > 0 && V > 0);
    ST3D_CHECK_ARG(workspace_bytes >= st3d_shade_vc_bwd_det_workspace_bytes(V) && ((uintptr_t)workspace & 15) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const st3d_det::DetRun det(workspace, kPixelPartials, (size_t)V * 3);
    vc_abs_sum_kernel<<<kPixelPartials, 256, 0, s>>>(grad_rgb, pix_to_face, bary, B, S, det.partials);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    const int tiles = (S + 15) / 16;
    shade_vc_bwd_kernel<1><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_rgb, pix_to_face, bary, zbuf, dists, faces, verts_colors, B,
                                                                  S, tiles, reinterpret_cast<float *>(det.acc), grad_bary, det.hdr);
    ST3D_LAUNCH_CHECK();
    return det.convert(1, grad_colors, s);
}
