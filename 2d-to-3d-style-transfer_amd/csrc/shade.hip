// shade.hip -- fused texture sampling + ambient shading + K=1 softmax blend, forward and
// backward: the device work of PyTorch3D SoftPhongShader(AmbientLights) +
// TexturesUV.sample_textures as configured at first_approach.py:108-113 /
// second_approach.py:102-108, plus the RGB / mask extraction of utils.py:70-72.
//
// The reference runs ~15 elementwise/gather launches per view here and materialises
// (1,S,S,1,3) texels, (1,S,S,4) RGBA, permutes and stacks; these kernels read the fragments
// once and write NCHW RGB + mask directly (coalesced per colour plane).
// HBM-bound: algorithmic bytes per pixel = 24 B fragments + 16 B written (fwd),
// 24 + 12 B read (bwd) + <= 12 float atomics per covered pixel into the 3*T*T*4-byte map.
// Built with -ffp-contract=off (same operation sequence as oracle/raster_ref.c).
// Supersampling (st3d_shade_ss_*, st3d_box_down_*): the same kernels over fragments at side a*S with the a x a box filter
// fused in -- 24 a^2 B of fragments + 16 B written per output pixel; neither the a*S image nor an a*S gradient exists.
#include <type_traits>

#include "common.h"
#include "det.h"
#include "phong.h"
#include "shadek1.h"
#include "tilebins.h"

namespace {

using namespace st3d_k1;

// LIT 1: the texel is lit first (phong.h): colour = ad * texel + sp replaces it in the blend
template <int LIT = 0>
__global__ __launch_bounds__(256) void shade_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                        const float *__restrict__ zbuf, const float *__restrict__ dists,
                                                        const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                                        const float *__restrict__ tex, int B, int S, int T,
                                                        float *__restrict__ rgb, float *__restrict__ mask,
                                                        const st3d_phong::LitArgs la = {}) {
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
    const FragUV fu = frag_uv(uvs, fuv, f, b0, b1, b2);
    const float u = fu.u, v = fu.v;
    const Footprint q = uv_footprint(u, v, T);
    const Blend bl = blend_k1(dists[i], zbuf[i]);
    const float w00 = q.wx0 * q.wy0, w01 = q.wx1 * q.wy0, w10 = q.wx0 * q.wy1, w11 = q.wx1 * q.wy1;
    const float *t00 = tex + ((size_t)q.r0 * T + q.x0) * 3, *t01 = tex + ((size_t)q.r0 * T + q.x1) * 3;
    const float *t10 = tex + ((size_t)q.r1 * T + q.x0) * 3, *t11 = tex + ((size_t)q.r1 * T + q.x1) * 3;
    float ad[3] = {1.f, 1.f, 1.f}, sp[3] = {0.f, 0.f, 0.f};
    if (LIT) st3d_phong::phong_fwd(la, (int)b, f, b0, b1, b2, ad, sp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = 0.f;
        if (q.vy0 && q.vx0) t += t00[c] * w00;
        if (q.vy0 && q.vx1) t += t01[c] * w01;
        if (q.vy1 && q.vx0) t += t10[c] * w10;
        if (q.vy1 && q.vx1) t += t11[c] * w11;
        if (LIT) t = ad[c] * t + sp[c];
        o[c * HW] = (bl.wnum * t + bl.delta * 1.0f) / bl.denom;
    }
    mask[i] = ((1.0f - (1.0f - bl.prob)) > 0.f) ? 1.f : 0.f;
}

// shade_fwd_kernel's pixel as a function: colour (3) and 0/1 mask of fragment i (view b), white and 0 where there is no
// face.  The same expressions in the same order (the plain kernel keeps its own copy: calling this from it moves its
// registers and branches, and its code is pinned instruction for instruction).
template <int LIT>
__device__ __forceinline__ float shade_px(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                          const float *__restrict__ zbuf, const float *__restrict__ dists,
                                          const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                          const float *__restrict__ tex, int T, size_t i, int b,
                                          const st3d_phong::LitArgs &la, float col[3]) {
    const int f = p2f[i];
    if (f < 0) {
        col[0] = 1.f; col[1] = 1.f; col[2] = 1.f;
        return 0.f;
    }
    const float b0 = bary[3 * i], b1 = bary[3 * i + 1], b2 = bary[3 * i + 2];
    const FragUV fu = frag_uv(uvs, fuv, f, b0, b1, b2);
    const float u = fu.u, v = fu.v;
    const Footprint q = uv_footprint(u, v, T);
    const Blend bl = blend_k1(dists[i], zbuf[i]);
    const float w00 = q.wx0 * q.wy0, w01 = q.wx1 * q.wy0, w10 = q.wx0 * q.wy1, w11 = q.wx1 * q.wy1;
    const float *t00 = tex + ((size_t)q.r0 * T + q.x0) * 3, *t01 = tex + ((size_t)q.r0 * T + q.x1) * 3;
    const float *t10 = tex + ((size_t)q.r1 * T + q.x0) * 3, *t11 = tex + ((size_t)q.r1 * T + q.x1) * 3;
    float ad[3] = {1.f, 1.f, 1.f}, sp[3] = {0.f, 0.f, 0.f};
    if (LIT) st3d_phong::phong_fwd(la, b, f, b0, b1, b2, ad, sp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = 0.f;
        if (q.vy0 && q.vx0) t += t00[c] * w00;
        if (q.vy0 && q.vx1) t += t01[c] * w01;
        if (q.vy1 && q.vx0) t += t10[c] * w10;
        if (q.vy1 && q.vx1) t += t11[c] * w11;
        if (LIT) t = ad[c] * t + sp[c];
        col[c] = (bl.wnum * t + bl.delta * 1.0f) / bl.denom;
    }
    return ((1.0f - (1.0f - bl.prob)) > 0.f) ? 1.f : 0.f;
}

// Supersampled forward: the fragments are at side A*S, one thread per OUTPUT pixel shades its A x A sub-pixels (the A of a
// row are contiguous: lanes stay coalesced) and writes their ordered sum / A^2 -- the A*S image never exists.  Sum order
// and division are those of box_down_fwd_kernel, so the result is bitwise shade_fwd_kernel at A*S followed by that filter.
// coverage = the same expression over the 0/1 mask (exact: a count over A^2).
template <int A, int LIT>
__global__ __launch_bounds__(256) void shade_ss_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                           const float *__restrict__ zbuf, const float *__restrict__ dists,
                                                           const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                                           const float *__restrict__ tex, int B, int S, int T,
                                                           float *__restrict__ rgb, float *__restrict__ coverage,
                                                           const st3d_phong::LitArgs la = {}) {
    const size_t HW = (size_t)S * S;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const size_t b = i / HW, p = i - b * HW;
    const int y = (int)(p / S), x = (int)(p - (size_t)y * S);
    const size_t SS = (size_t)A * S;
    const size_t base = b * SS * SS + (size_t)(A * y) * SS + (size_t)A * x;
    float s[3], sm;
#pragma unroll
    for (int j = 0; j < A; ++j) {
#pragma unroll
        for (int k = 0; k < A; ++k) {
            float col[3];
            const float m = shade_px<LIT>(p2f, bary, zbuf, dists, uvs, fuv, tex, T, base + (size_t)j * SS + k, (int)b, la, col);
            if (j == 0 && k == 0) { s[0] = col[0]; s[1] = col[1]; s[2] = col[2]; sm = m; }
            else { s[0] = s[0] + col[0]; s[1] = s[1] + col[1]; s[2] = s[2] + col[2]; sm = sm + m; }
        }
    }
    float *o = rgb + b * 3 * HW + p;
    o[0] = s[0] / (float)(A * A); o[HW] = s[1] / (float)(A * A); o[2 * HW] = s[2] / (float)(A * A);
    coverage[i] = sm / (float)(A * A);
}

// Texture-sampling backward.  One workgroup per 16x16-pixel tile of one view.  The <= 12 bilinear contributions of a
// pixel are not sent to HBM one float atomic each (neighbouring pixels hit the same texels: ~6 M contended L2 atomics
// per step at config 2): they are first summed per texel in LDS and each distinct texel of the tile then costs three
// global atomics.  d/d(u,v) and d/d(bary) (vertex path) are per-pixel outputs written directly.
// A tile in which no pixel has a face writes its zero rows and leaves (one workgroup-wide OR): three quarters of the tiles
// of a typical view.  The others sum through the texel table of tilebins.h: 36 KB + 4 B of LDS in fixed point, 24 KB + 4 B
// in float: four and six workgroups per CU (the one 56 KB table it replaced allowed two).
//
// DET 0: float LDS table + float global atomics (fast default).  DET 1: the same binning in 64-bit fixed point (LDS and
// global integer atomics; `gtex` is then the int64 accumulator array and `det` holds the power-of-two scale): bitwise
// reproducible whatever the order (det.h).
// LIT 1: colour = ad * texel + sp (phong.h) -- the texture / uv factor of a channel becomes g k ad_c, and with la.grad_np the
// lighting's own d/dN, d/dP go to grad_np (per pixel) and, through N = sum b_i n_i and P = sum b_i v_i, into gbary.
// A > 1 (supersampling): S and every per-pixel array are at the SUB-PIXEL side; grad_rgb is (B,3,S/A,S/A) and sub-pixel
// (yi, xi) takes grad_rgb(yi / A, xi / A) / A^2 -- the backward of the ordered box sum of shade_ss_fwd_kernel.  The tile is
// still 16 x 16 sub-pixels = 256 footprints, so the table's sizes stay.
template <int DET, int LIT = 0, int A = 1>
__global__ __launch_bounds__(256) void shade_bwd_kernel(const float *__restrict__ grad_rgb, const int32_t *__restrict__ p2f,
                                                        const float *__restrict__ bary, const float *__restrict__ zbuf,
                                                        const float *__restrict__ dists, const float *__restrict__ uvs,
                                                        const int32_t *__restrict__ fuv, const float *__restrict__ tex,
                                                        int B, int S, int T, int tiles_x, float *__restrict__ gtex,
                                                        float *__restrict__ guv, float *__restrict__ gbary,
                                                        const st3d_det::DetHeader *__restrict__ det,
                                                        const st3d_phong::LitArgs la = {}) {
    typedef typename std::conditional<DET != 0, unsigned long long, float>::type acc_t;
    ST3D_TEXEL_BINS(bins, acc_t);
    const int tid = threadIdx.x;
    const double dscale = DET ? det->scale : 1.0;
    const size_t HW = (size_t)S * S;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int yi = ty * 16 + (tid >> 4), xi = tx * 16 + (tid & 15);
    const bool in_img = yi < S && xi < S;
    const size_t p = (size_t)yi * S + xi, i = (size_t)b * HW + p;
    const int f = in_img ? p2f[i] : -1;
    if (in_img && f < 0) {
        if (guv) { guv[2 * i] = 0.f; guv[2 * i + 1] = 0.f; }
        if (gbary) { gbary[3 * i] = 0.f; gbary[3 * i + 1] = 0.f; gbary[3 * i + 2] = 0.f; }
    }
    if (gtex) {
        if (!__syncthreads_or(f >= 0)) return;           // the same answer in every lane: the whole workgroup leaves
        bins.reset();                                    // here, so that its barrier is long past when the deposits arrive
    }
    int dep_texel[4];            // this pixel's footprint corners: texel, weight; dep_valid: bit c = corner c deposits
    float dep_w[4], dep_g[3] = {0.f, 0.f, 0.f};
    unsigned dep_valid = 0;
    if (f >= 0) {
        const bool want_uv = guv || gbary;
        const float b0 = bary[3 * i], b1 = bary[3 * i + 1], b2 = bary[3 * i + 2];
        const FragUV fu = frag_uv(uvs, fuv, f, b0, b1, b2);
        const int u0 = fu.u0, u1 = fu.u1, u2 = fu.u2;
        const float u = fu.u, v = fu.v;
        const Footprint q = uv_footprint(u, v, T);
        const Blend bl = blend_k1(dists[i], zbuf[i]);
        const float k = bl.wnum / bl.denom;
        const float w00 = q.wx0 * q.wy0, w01 = q.wx1 * q.wy0, w10 = q.wx0 * q.wy1, w11 = q.wx1 * q.wy1;
        const int e00 = q.r0 * T + q.x0, e01 = q.r0 * T + q.x1, e10 = q.r1 * T + q.x0, e11 = q.r1 * T + q.x1;
        const size_t gHW = A == 1 ? HW : (size_t)(S / A) * (S / A);
        const float *g = grad_rgb + (size_t)b * 3 * gHW + (A == 1 ? p : (size_t)(yi / A) * (S / A) + xi / A);
        const float gs[3] = {A == 1 ? g[0] : g[0] / (float)(A * A), A == 1 ? g[gHW] : g[gHW] / (float)(A * A),
                             A == 1 ? g[2 * gHW] : g[2 * gHW] / (float)(A * A)};
        const float gk0[3] = {gs[0] * k, gs[1] * k, gs[2] * k};
        float ad[3] = {1.f, 1.f, 1.f}, sp[3] = {0.f, 0.f, 0.f};
        if (LIT) st3d_phong::phong_fwd(la, b, f, b0, b1, b2, ad, sp);
        const float gk[3] = {LIT ? gk0[0] * ad[0] : gk0[0], LIT ? gk0[1] * ad[1] : gk0[1], LIT ? gk0[2] * ad[2] : gk0[2]};
        if (LIT && la.grad_np) {
            // d colour_c / d ad_c = texel_c, d colour_c / d sp_c = 1
            float g_ad[3], g_sp[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = 0.f;
                if (q.vy0 && q.vx0) t += tex[(size_t)e00 * 3 + c] * w00;
                if (q.vy0 && q.vx1) t += tex[(size_t)e01 * 3 + c] * w01;
                if (q.vy1 && q.vx0) t += tex[(size_t)e10 * 3 + c] * w10;
                if (q.vy1 && q.vx1) t += tex[(size_t)e11 * 3 + c] * w11;
                g_ad[c] = gk0[c] * t;
                g_sp[c] = gk0[c];
            }
            st3d_phong::F3 gN = {0.f, 0.f, 0.f}, gP = {0.f, 0.f, 0.f};
            if (la.kind != st3d_phong::kAmbient) st3d_phong::phong_bwd(la, b, f, b0, b1, b2, g_ad, g_sp, gN, gP);
            float *o = la.grad_np + 6 * i;
            o[0] = gN.x; o[1] = gN.y; o[2] = gN.z; o[3] = gP.x; o[4] = gP.y; o[5] = gP.z;
        }
        if (want_uv) {
            float gix = 0.f, giy = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t00 = (q.vy0 && q.vx0) ? tex[(size_t)e00 * 3 + c] : 0.f, t01 = (q.vy0 && q.vx1) ? tex[(size_t)e01 * 3 + c] : 0.f;
                const float t10 = (q.vy1 && q.vx0) ? tex[(size_t)e10 * 3 + c] : 0.f, t11 = (q.vy1 && q.vx1) ? tex[(size_t)e11 * 3 + c] : 0.f;
                gix += gk[c] * ((t01 - t00) * q.wy0 + (t11 - t10) * q.wy1);
                giy += gk[c] * ((t10 - t00) * q.wx0 + (t11 - t01) * q.wx1);
            }
            const float gu = q.cx ? 0.f : gix * (float)(T - 1);
            const float gv = q.cy ? 0.f : giy * (float)(T - 1);
            if (guv) { guv[2 * i] = gu; guv[2 * i + 1] = gv; }
            if (gbary) {      // uv = sum_i b_i * uv_i
                gbary[3 * i] = gu * uvs[2 * u0] + gv * uvs[2 * u0 + 1];
                gbary[3 * i + 1] = gu * uvs[2 * u1] + gv * uvs[2 * u1 + 1];
                gbary[3 * i + 2] = gu * uvs[2 * u2] + gv * uvs[2 * u2 + 1];
                if (LIT && la.grad_np && la.kind != st3d_phong::kAmbient) {     // + dN/db_i = n_i, dP/db_i = v_i
                    const float *gnp = la.grad_np + 6 * i;
                    const st3d_phong::F3 gN = st3d_phong::f3(gnp), gP = st3d_phong::f3(gnp + 3);
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int vj = la.faces[3 * f + j];
                        gbary[3 * i + j] += st3d_phong::dot3(gN, st3d_phong::f3(la.normals + 3 * vj)) +
                                            st3d_phong::dot3(gP, st3d_phong::f3(la.verts + 3 * vj));
                    }
                }
            }
        }
        dep_texel[0] = e00; dep_texel[1] = e01; dep_texel[2] = e10; dep_texel[3] = e11;
        dep_w[0] = w00; dep_w[1] = w01; dep_w[2] = w10; dep_w[3] = w11;
        dep_g[0] = gk[0]; dep_g[1] = gk[1]; dep_g[2] = gk[2];
        dep_valid = (q.vy0 && q.vx0 ? 1u : 0u) | (q.vy0 && q.vx1 ? 2u : 0u) | (q.vy1 && q.vx0 ? 4u : 0u) | (q.vy1 && q.vx1 ? 8u : 0u);
    }
    if (gtex) bins.scatter(dep_texel, dep_w, dep_g, dep_valid, dscale, gtex);
}

// out = img*mask + bg*(1-mask)   (utils.py:23,27); bg == nullptr: out = img*mask
__global__ __launch_bounds__(256) void background_kernel(const float *__restrict__ img, const float *__restrict__ mask,
                                                         const float *__restrict__ bg, int bg_batch, int B, size_t HW,
                                                         float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * 3 * HW) return;
    const size_t b = i / (3 * HW), r = i - b * 3 * HW, p = r % HW;
    const float m = mask[b * HW + p];
    float v = img[i] * m;
    if (bg) v = v + bg[(bg_batch == 1 ? 0 : b * 3 * HW) + r] * (1.0f - m);
    out[i] = v;
}

// a x a box filter (B*C planes of side A*S -> side S): out = (ordered row-major sum of the block) / A^2, the sum order and
// the division of shade_ss_fwd_kernel.  VEC: four outputs per thread, A float4 loads per block row and one float4 store
// (S % 4 == 0 and 16-byte aligned pointers); else one output per thread.
template <int A, int VEC>
__global__ __launch_bounds__(256) void box_down_fwd_kernel(const float *__restrict__ in, size_t N, int S, float *__restrict__ out) {
    constexpr int V = VEC ? 4 : 1;
    const size_t W = (size_t)(S / V), per = W * S;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * per) return;
    const size_t n = t / per, r = t - n * per;
    const int y = (int)(r / W), x = (int)(r - (size_t)y * W) * V;
    const size_t SS = (size_t)A * S;
    const float *src = in + n * SS * SS + (size_t)(A * y) * SS + (size_t)A * x;
    float s[V];
#pragma unroll
    for (int j = 0; j < A; ++j) {
        float row[A * V];
        if constexpr (VEC != 0) {
#pragma unroll
            for (int q = 0; q < A; ++q) {
                const float4 v4 = *reinterpret_cast<const float4 *>(src + (size_t)j * SS + 4 * q);
                row[4 * q] = v4.x; row[4 * q + 1] = v4.y; row[4 * q + 2] = v4.z; row[4 * q + 3] = v4.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < A; ++q) row[q] = src[(size_t)j * SS + q];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int k = 0; k < A; ++k) {
                if (j == 0 && k == 0) s[v] = row[A * v];
                else s[v] = s[v] + row[A * v + k];
            }
        }
    }
    float *dst = out + n * (size_t)S * S + (size_t)y * S + x;
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = s[v] / (float)(A * A);
    if constexpr (VEC != 0) *reinterpret_cast<float4 *>(dst) = make_float4(s[0], s[1], s[2], s[3]);
    else dst[0] = s[0];
}

// its transpose: every sub-pixel of a block gets grad_out / A^2 (one division per output value)
template <int A, int VEC>
__global__ __launch_bounds__(256) void box_down_bwd_kernel(const float *__restrict__ gout, size_t N, int S, float *__restrict__ gin) {
    constexpr int V = VEC ? 4 : 1;
    const size_t W = (size_t)(S / V), per = W * S;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * per) return;
    const size_t n = t / per, r = t - n * per;
    const int y = (int)(r / W), x = (int)(r - (size_t)y * W) * V;
    const size_t SS = (size_t)A * S;
    const float *src = gout + n * (size_t)S * S + (size_t)y * S + x;
    float g[V];
    if constexpr (VEC != 0) {
        const float4 v4 = *reinterpret_cast<const float4 *>(src);
        g[0] = v4.x; g[1] = v4.y; g[2] = v4.z; g[3] = v4.w;
    } else {
        g[0] = src[0];
    }
    float row[A * V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float gs = g[v] / (float)(A * A);
#pragma unroll
        for (int k = 0; k < A; ++k) row[A * v + k] = gs;
    }
    float *dst = gin + n * SS * SS + (size_t)(A * y) * SS + (size_t)A * x;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        if constexpr (VEC != 0) {
#pragma unroll
            for (int q = 0; q < A; ++q)
                *reinterpret_cast<float4 *>(dst + (size_t)j * SS + 4 * q) = make_float4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < A; ++q) dst[(size_t)j * SS + q] = row[q];
        }
    }
}

// The fixed-point bound of the supersampled texture scatter: partials[block] = scale * sum |grad_rgb| over the block's
// grid-stride share of the B*3*S^2 values (fixed order, like st3d_det::det_abs_sum_kernel).  A pixel none of whose A x A
// sub-pixels holds a face deposits nothing, so its values enter with weight 0: finite ones leave the bound -- and with it
// the power-of-two scale -- independent of what a loss wrote on the background (a loss that skips the background's
// gradient gets the bits of one that does not), a NaN or an infinity there still poisons it (x * 0 = NaN).
template <int A>
__global__ __launch_bounds__(256) void ss_abs_sum_kernel(const float *__restrict__ g, const int32_t *__restrict__ p2f, int B, int S,
                                                         float scale, float *__restrict__ partials) {
    __shared__ float s4[4];
    float acc = 0.f;
    const size_t HW = (size_t)S * S, n = (size_t)B * HW, SS = (size_t)A * S;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const size_t b = i / HW, p = i - b * HW;
        const int y = (int)(p / S), x = (int)(p - (size_t)y * S);
        const int32_t *f = p2f + b * SS * SS + (size_t)(A * y) * SS + (size_t)A * x;
        bool covered = false;
#pragma unroll
        for (int j = 0; j < A; ++j)
#pragma unroll
            for (int k = 0; k < A; ++k) covered = covered || f[(size_t)j * SS + k] >= 0;
        const float *gp = g + b * 3 * HW + p;
        const float w = covered ? 1.f : 0.f;
        acc += fabsf(gp[0]) * w;
        acc += fabsf(gp[HW]) * w;
        acc += fabsf(gp[2 * HW]) * w;
    }
    const float t = st3d_det::det_block_sum(acc, s4);
    if (threadIdx.x == 0) partials[blockIdx.x] = t * scale;
}

constexpr int kMaxSide = 4096;      // the rasteriser's limit: fragments exist up to this side

// a = 1..4 -> the template argument
#define ST3D_SS_DISPATCH(a, CALL) \
    switch (a) {                  \
    case 1: { constexpr int A_ = 1; CALL; } break; \
    case 2: { constexpr int A_ = 2; CALL; } break; \
    case 3: { constexpr int A_ = 3; CALL; } break; \
    default: { constexpr int A_ = 4; CALL; } break; \
    }

}  // namespace

extern "C" int st3d_shade_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                              const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int T,
                              int F, int VT, float *rgb, float *mask, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture && rgb && mask);
    ST3D_CHECK_ARG(B > 0 && S > 0 && T > 1 && F > 0 && VT > 0);
    const size_t n = (size_t)B * S * S;
    shade_fwd_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(pix_to_face, bary, zbuf, dists, verts_uvs,
                                                                                   faces_uvs, texture, B, S, T, rgb, mask);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_ss_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                 const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int a,
                                 int T, int F, int VT, float *rgb, float *coverage, st3d_stream_t stream) {
    ST3D_CHECK_ARG(a >= 1 && a <= 4 && S > 0 && S <= kMaxSide / a);
    if (a == 1) return st3d_shade_fwd(pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, T, F, VT, rgb, coverage, stream);
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture && rgb && coverage);
    ST3D_CHECK_ARG(B > 0 && T > 1 && F > 0 && VT > 0);
    const size_t n = (size_t)B * S * S;
    ST3D_SS_DISPATCH(a, (shade_ss_fwd_kernel<A_, 0><<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(
                            pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, T, rgb, coverage)));
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

namespace {
int box_args_ok(const void *in, const void *out, int B, int C, int S, int a) {
    return in && out && B > 0 && C > 0 && a >= 1 && a <= 4 && S > 0 && S <= kMaxSide / a;
}
bool box_vec(const void *p, const void *q, int S) { return S % 4 == 0 && (((uintptr_t)p | (uintptr_t)q) & 15) == 0; }
}  // namespace

extern "C" int st3d_box_down_fwd(const float *in, int B, int C, int S, int a, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(box_args_ok(in, out, B, C, S, a));
    const size_t N = (size_t)B * C;
    hipStream_t s = st3d::as_stream(stream);
    if (box_vec(in, out, S)) {
        ST3D_SS_DISPATCH(a, (box_down_fwd_kernel<A_, 1><<<st3d::cdiv((long)(N * S * (S / 4)), 256), 256, 0, s>>>(in, N, S, out)));
    } else {
        ST3D_SS_DISPATCH(a, (box_down_fwd_kernel<A_, 0><<<st3d::cdiv((long)(N * S * S), 256), 256, 0, s>>>(in, N, S, out)));
    }
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_box_down_bwd(const float *grad_out, int B, int C, int S, int a, float *grad_in, st3d_stream_t stream) {
    ST3D_CHECK_ARG(box_args_ok(grad_out, grad_in, B, C, S, a));
    const size_t N = (size_t)B * C;
    hipStream_t s = st3d::as_stream(stream);
    if (box_vec(grad_out, grad_in, S)) {
        ST3D_SS_DISPATCH(a, (box_down_bwd_kernel<A_, 1><<<st3d::cdiv((long)(N * S * (S / 4)), 256), 256, 0, s>>>(grad_out, N, S, grad_in)));
    } else {
        ST3D_SS_DISPATCH(a, (box_down_bwd_kernel<A_, 0><<<st3d::cdiv((long)(N * S * S), 256), 256, 0, s>>>(grad_out, N, S, grad_in)));
    }
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                              const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                              int B, int S, int T, int F, int VT, float *grad_texture, float *grad_uv,
                              float *grad_bary, st3d_stream_t stream) {
    return st3d_shade_ss_bwd(grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, 1, T, F, VT,
                             grad_texture, grad_uv, grad_bary, stream);
}

// (S: the side of grad_rgb; fragments and the per-pixel outputs are at a * S)
extern "C" int st3d_shade_ss_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                 const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                                 int B, int S, int a, int T, int F, int VT, float *grad_texture, float *grad_uv,
                                 float *grad_bary, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture);
    ST3D_CHECK_ARG(grad_texture || grad_uv || grad_bary);
    ST3D_CHECK_ARG(B > 0 && S > 0 && T > 1 && F > 0 && VT > 0);
    ST3D_CHECK_ARG(a >= 1 && a <= 4 && S <= kMaxSide / a);
    const int SS = a * S, tiles = (SS + 15) / 16;
    ST3D_SS_DISPATCH(a, (shade_bwd_kernel<0, 0, A_><<<dim3(tiles * tiles, B), 256, 0, st3d::as_stream(stream)>>>(
                            grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, SS, T, tiles, grad_texture,
                            grad_uv, grad_bary, nullptr)));
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

// (bound on any texel-channel sum: sum over the batch of |grad_rgb| -- blend weight and bilinear weights are <= 1: st3d_det::det_abs_sum_kernel)
using st3d_det::kPixelPartials;

extern "C" size_t st3d_shade_bwd_det_workspace_bytes(int T) {
    return st3d_det::workspace_bytes((size_t)T * T * 3, kPixelPartials);
}

// st3d_shade_bwd with a bitwise reproducible texture gradient: fixed-point accumulation (det.h); measured no slower than the
// float-atomic scatter (0.128 vs 0.137 ms at config 2), so it is the default of the Python host (st3d/ops.py).  grad_texture is ACCUMULATED into, like st3d_shade_bwd.
extern "C" int st3d_shade_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                  const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                                  int B, int S, int T, int F, int VT, float *grad_texture, float *grad_uv, float *grad_bary,
                                  void *workspace, size_t workspace_bytes, st3d_stream_t stream) {
    return st3d_shade_ss_bwd_det(grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, 1, T, F, VT,
                                 grad_texture, grad_uv, grad_bary, workspace, workspace_bytes, stream);
}

// a > 1: the bound pass runs over grad_rgb itself (B*3*S^2 values, ss_abs_sum_kernel): a block deposits a^2 contributions
// of at most |g| / a^2 each, so sum |g| over the pixels that deposit anything bounds every texel sum
extern "C" int st3d_shade_ss_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                     const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                                     int B, int S, int a, int T, int F, int VT, float *grad_texture, float *grad_uv,
                                     float *grad_bary, void *workspace, size_t workspace_bytes, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture && workspace);
    ST3D_CHECK_ARG(grad_texture);
    ST3D_CHECK_ARG(B > 0 && S > 0 && T > 1 && F > 0 && VT > 0);
    ST3D_CHECK_ARG(a >= 1 && a <= 4 && S <= kMaxSide / a);
    ST3D_CHECK_ARG(workspace_bytes >= st3d_shade_bwd_det_workspace_bytes(T) && ((uintptr_t)workspace & 15) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const st3d_det::DetRun det(workspace, kPixelPartials, (size_t)T * T * 3);
    const size_t npx = (size_t)B * 3 * S * S;
    if (a == 1) {
        st3d_det::det_abs_sum_kernel<<<kPixelPartials, 256, 0, s>>>(grad_rgb, npx, det.partials);
    } else {
        ST3D_SS_DISPATCH(a, (ss_abs_sum_kernel<A_><<<kPixelPartials, 256, 0, s>>>(grad_rgb, pix_to_face, B, S, 1.f, det.partials)));
    }
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    const int SS = a * S, tiles = (SS + 15) / 16;
    ST3D_SS_DISPATCH(a, (shade_bwd_kernel<1, 0, A_><<<dim3(tiles * tiles, B), 256, 0, s>>>(
                            grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, SS, T, tiles,
                            reinterpret_cast<float *>(det.acc), grad_uv, grad_bary, det.hdr)));
    ST3D_LAUNCH_CHECK();
    return det.convert(1, grad_texture, s);
}

extern "C" int st3d_apply_background(const float *img, const float *mask, const float *bg, int bg_batch, int B, int S,
                                     float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(img && mask && out);
    ST3D_CHECK_ARG(B > 0 && S > 0 && (bg_batch == 1 || bg_batch == B));
    const size_t n = (size_t)B * 3 * S * S;
    background_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(img, mask, bg, bg_batch, B,
                                                                                   (size_t)S * S, out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

// ------------------------------------------------------------------------------------------ lit shading (phong.h)
namespace {
st3d_phong::LitArgs lit_args(const float *verts, const float *normals, const int32_t *faces, const float *R, const float *trans,
                             const float *light, int n_lights, int kind, float *grad_np) {
    st3d_phong::LitArgs la;
    la.verts = verts; la.normals = normals; la.faces = faces; la.R = R; la.T = trans; la.light = light;
    la.n_lights = n_lights; la.kind = kind; la.grad_np = grad_np;
    return la;
}
}  // namespace

extern "C" int st3d_shade_lit_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                  const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int T,
                                  int F, int VT, const float *verts, const float *normals, const int32_t *faces, const float *R,
                                  const float *trans, const float *light, int n_lights, int kind, float *rgb, float *mask,
                                  st3d_stream_t stream) {
    return st3d_shade_ss_lit_fwd(pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, 1, T, F, VT, verts, normals,
                                 faces, R, trans, light, n_lights, kind, rgb, mask, stream);
}

extern "C" int st3d_shade_ss_lit_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                     const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int a,
                                     int T, int F, int VT, const float *verts, const float *normals, const int32_t *faces,
                                     const float *R, const float *trans, const float *light, int n_lights, int kind, float *rgb,
                                     float *coverage, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture && rgb && coverage);
    ST3D_CHECK_ARG(faces && R && trans && light && (n_lights == 1 || n_lights == B));
    ST3D_CHECK_ARG(kind >= st3d_phong::kAmbient && kind <= st3d_phong::kHeadlight);
    ST3D_CHECK_ARG(kind == st3d_phong::kAmbient || (verts && normals));
    ST3D_CHECK_ARG(B > 0 && S > 0 && T > 1 && F > 0 && VT > 0);
    ST3D_CHECK_ARG(a >= 1 && a <= 4 && S <= kMaxSide / a);
    const size_t n = (size_t)B * S * S;
    const st3d_phong::LitArgs la = lit_args(verts, normals, faces, R, trans, light, n_lights, kind, nullptr);
    if (a == 1) {
        shade_fwd_kernel<1><<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(
            pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, T, rgb, coverage, la);
    } else {
        ST3D_SS_DISPATCH(a, (shade_ss_fwd_kernel<A_, 1><<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(
                                pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, T, rgb, coverage, la)));
    }
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_lit_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                  const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                                  int B, int S, int T, int F, int VT, const float *verts, const float *normals,
                                  const int32_t *faces, const float *R, const float *trans, const float *light, int n_lights,
                                  int kind, float weight_bound, float *grad_texture, float *grad_bary, float *grad_np,
                                  void *workspace, size_t workspace_bytes, st3d_stream_t stream) {
    return st3d_shade_ss_lit_bwd(grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, S, 1, T, F, VT, verts,
                                 normals, faces, R, trans, light, n_lights, kind, weight_bound, grad_texture, grad_bary, grad_np,
                                 workspace, workspace_bytes, stream);
}

extern "C" int st3d_shade_ss_lit_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                     const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                                     int B, int S, int a, int T, int F, int VT, const float *verts, const float *normals,
                                     const int32_t *faces, const float *R, const float *trans, const float *light, int n_lights,
                                     int kind, float weight_bound, float *grad_texture, float *grad_bary, float *grad_np,
                                     void *workspace, size_t workspace_bytes, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && texture);
    ST3D_CHECK_ARG(faces && R && trans && light && (n_lights == 1 || n_lights == B));
    ST3D_CHECK_ARG(kind >= st3d_phong::kAmbient && kind <= st3d_phong::kHeadlight);
    ST3D_CHECK_ARG(kind == st3d_phong::kAmbient || (verts && normals));
    ST3D_CHECK_ARG(grad_texture || grad_bary);
    ST3D_CHECK_ARG(!grad_bary == !grad_np);
    ST3D_CHECK_ARG(B > 0 && S > 0 && T > 1 && F > 0 && VT > 0 && weight_bound >= 0.f);
    ST3D_CHECK_ARG(a >= 1 && a <= 4 && S <= kMaxSide / a);
    hipStream_t s = st3d::as_stream(stream);
    const int SS = a * S, tiles = (SS + 15) / 16;
    const st3d_phong::LitArgs la = lit_args(verts, normals, faces, R, trans, light, n_lights, kind, grad_np);
    if (!workspace) {
        ST3D_SS_DISPATCH(a, (shade_bwd_kernel<0, 1, A_><<<dim3(tiles * tiles, B), 256, 0, s>>>(
                                grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, SS, T, tiles, grad_texture,
                                nullptr, grad_bary, nullptr, la)));
        ST3D_LAUNCH_CHECK();
        return ST3D_OK;
    }
    // fixed point: every texture contribution is |g| k ad_c w <= |g| weight_bound (k, w <= 1; weight_bound >= max ad_c)
    ST3D_CHECK_ARG(grad_texture);
    ST3D_CHECK_ARG(workspace_bytes >= st3d_shade_bwd_det_workspace_bytes(T) && ((uintptr_t)workspace & 15) == 0);
    const st3d_det::DetRun det(workspace, kPixelPartials, (size_t)T * T * 3);
    const size_t npx = (size_t)B * 3 * S * S;
    if (a == 1) {
        st3d_det::det_abs_sum_scaled_kernel<<<kPixelPartials, 256, 0, s>>>(grad_rgb, npx, weight_bound, det.partials);
    } else {
        ST3D_SS_DISPATCH(a, (ss_abs_sum_kernel<A_><<<kPixelPartials, 256, 0, s>>>(grad_rgb, pix_to_face, B, S, weight_bound, det.partials)));
    }
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    ST3D_SS_DISPATCH(a, (shade_bwd_kernel<1, 1, A_><<<dim3(tiles * tiles, B), 256, 0, s>>>(
                            grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, texture, B, SS, T, tiles,
                            reinterpret_cast<float *>(det.acc), nullptr, grad_bary, det.hdr, la)));
    ST3D_LAUNCH_CHECK();
    return det.convert(1, grad_texture, s);
}
