// mipmap.hip -- mip-mapped trilinear texture sampling for the hard renderer (K = 1, unlit).
//
//   chain    level_0 = the map; level_{l+1}[r][x] = ((a + b) + (c + d)) * 0.25f over the 2 x 2 block below it.  The levels
//            live in texpyr.hip's packed layout: level l is the (T_l, T_l, 3) block at float offset 3 * sum_{k<l} T_k^2,
//            T_l = T >> l.  Adjoint, folded coarse to fine: acc_{L-1} = g_{L-1}; acc_l = g_l + 0.25f * acc_{l+1}[r>>1][x>>1].
//   lod      per covered pixel, analytic (no neighbour is read): the screen-space derivatives of the perspective-correct
//            barycentrics from the face's projected vertices -> d(u,v)/dx, d(u,v)/dy -> rho (texels per pixel step) ->
//            lambda = clamp(log2 rho + bias, 0, L-1), 0 where !(rho > 1).  Evaluated in fp64: the edge function of a
//            sub-pixel face cancels to a handful of fp32 bits, and the plane is B*S*S values, once per render.
//   sample   l0 = floor(lambda), t = lambda - l0; texel = (1 - t) bil(l0) + t bil(l0 + 1); level 0 is tapped exactly as
//            shade.hip's plain kernel taps it, level l >= 1 at ix_l = (ix + 0.5) / 2^l - 0.5 of the clamped level-0 index.
//            t == 0: the upper level is neither read nor deposited into (lambda == 0 is the plain kernel bit for bit).
//   backward d/d(level texels) scattered into a packed-pyramid gradient through the per-tile texel table (tilebins.h), run once per
//            level of the pair (lower, then upper) in the same 36 KB, then folded by the chain's adjoint; d/d(u,v) through
//            both levels' taps.  lambda is a constant of the backward.
//
// Launches: build is one tile kernel (a 32 x 32 level-0 tile goes down up to five levels through LDS: a 2 x 2 box has no
// halo, and tile origins are multiples of 32) plus, for L > 6, one workgroup for the remaining levels (side <= T / 64).
// The adjoint is ONE launch for any L: every level-0 value folds its own chain coarse to fine -- the same operations in the
// same order as the level-by-level definition; the coarse loads are shared by 4^l texels and come from the cache.
// Built like shade.hip (no FMA contraction, correctly rounded division): the expressions below are the roundings.
#include <type_traits>

#include "common.h"
#include "det.h"
#include "shadek1.h"
#include "tilebins.h"

namespace {

using namespace st3d_k1;

constexpr int kMaxLevels = 16;
constexpr int kMaxSide = 16384;          // texpyr.hip's limits: 3 * T^2 < 2^31
constexpr int kMaxRaster = 4096;         // the rasteriser's limit: fragments exist up to this side
constexpr int FT = 32;                   // level-0 tile of the build
constexpr int KTILE = 5;                 // levels the tile kernel takes a tile down

// offsets in TEXELS of every level in the packed pyramid (numel / 3 at [L]); by value into the kernels
struct Levels { int off[kMaxLevels + 1]; };

inline bool shape_ok(int T, int L) {
    if (T < 2 || T > kMaxSide || L < 1 || L > kMaxLevels) return false;
    if (L == 1) return true;
    return (T & ((1 << (L - 1)) - 1)) == 0 && (T >> (L - 1)) >= 2;
}

inline Levels levels_of(int T, int L) {
    Levels lv;
    int off = 0;
    for (int l = 0; l <= kMaxLevels; ++l) {
        lv.off[l] = off;
        if (l < L) off += (T >> l) * (T >> l);
    }
    return lv;
}

// ---------------------------------------------------------------------------------------------------- chain
// levels 0..K of one 32 x 32 level-0 tile: level 0 is copied, level 1 comes straight from global, the rest through LDS
__global__ __launch_bounds__(256) void mip_build_tile_kernel(const float *__restrict__ tex, int T, int K, Levels lv,
                                                             float *__restrict__ pyr) {
    __shared__ float buf[2][(FT / 2) * (FT / 2) * 3];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FT, y0 = blockIdx.y * FT;
    const int w0 = min(FT, T - x0), h0 = min(FT, T - y0);
    for (int i = tid; i < h0 * w0 * 3; i += 256) {
        const int r = i / (w0 * 3), f = i - r * (w0 * 3);
        const size_t at = ((size_t)(y0 + r) * T + x0) * 3 + f;
        pyr[at] = tex[at];
    }
    int cur = 0;
    for (int l = 1; l <= K; ++l) {
        const int n = T >> l, w = w0 >> l, h = h0 >> l;          // this tile's part of level l, origin (x0 >> l, y0 >> l)
        const int ws = w0 >> (l - 1);                            // width of the part of level l - 1 in LDS
        float *dst = buf[cur];
        const float *src = buf[cur ^ 1];
        float *out = pyr + (size_t)lv.off[l] * 3;
        for (int i = tid; i < h * w * 3; i += 256) {
            const int r = i / (w * 3), f = i - r * (w * 3);
            const int x = f / 3, c = f - 3 * x;
            float a, b, cc, d;
            if (l == 1) {
                const float *s = tex + ((size_t)(y0 + 2 * r) * T + x0 + 2 * x) * 3 + c;
                a = s[0]; b = s[3]; cc = s[(size_t)T * 3]; d = s[(size_t)T * 3 + 3];
            } else {
                const float *s = src + ((2 * r) * ws + 2 * x) * 3 + c;
                a = s[0]; b = s[3]; cc = s[ws * 3]; d = s[ws * 3 + 3];
            }
            const float v = ((a + b) + (cc + d)) * 0.25f;
            dst[(r * w + x) * 3 + c] = v;
            out[((size_t)((y0 >> l) + r) * n + (x0 >> l) + x) * 3 + c] = v;
        }
        __syncthreads();
        cur ^= 1;
    }
}

// ONE workgroup: levels K+1 .. L-1, each read back from the block the level before it was written to
__global__ __launch_bounds__(1024) void mip_build_tail_kernel(int T, int K, int L, Levels lv, float *pyr) {
    for (int l = K + 1; l < L; ++l) {
        const int n = T >> l;
        const float *src = pyr + (size_t)lv.off[l - 1] * 3;
        float *dst = pyr + (size_t)lv.off[l] * 3;
        if (l > K + 1) {                    // written by this workgroup: complete and visible before anybody reads it
            __threadfence();
            __syncthreads();
            __threadfence();
        }
        for (int i = threadIdx.x; i < n * n * 3; i += 1024) {
            const int t = i / 3, c = i - 3 * t;
            const int r = t / n, x = t - r * n;
            const float *s = src + ((size_t)(2 * r) * (2 * n) + 2 * x) * 3 + c;
            dst[i] = ((s[0] + s[3]) + (s[(size_t)2 * n * 3] + s[(size_t)2 * n * 3 + 3])) * 0.25f;
        }
    }
}

// grad_texture[r][x][c] (+)= acc_0, the chain folded per element from the coarsest level down
__global__ __launch_bounds__(256) void mip_adjoint_kernel(const float *__restrict__ gp, int T, int L, Levels lv, int accumulate,
                                                          float *__restrict__ gtex) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)T * T * 3) return;
    const int t = (int)(i / 3), c = (int)(i - (size_t)t * 3);
    const int r = t / T, x = t - r * T;
    float acc = 0.f;
    for (int l = L - 1; l >= 0; --l) {
        const int n = T >> l;
        const float g = gp[((size_t)lv.off[l] + (size_t)(r >> l) * n + (x >> l)) * 3 + c];
        acc = l == L - 1 ? g : g + 0.25f * acc;
    }
    gtex[i] = accumulate ? gtex[i] + acc : acc;
}

// ---------------------------------------------------------------------------------------------------- lod
__global__ __launch_bounds__(256) void mip_lod_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                      const float *__restrict__ zbuf, const float *__restrict__ ndc,
                                                      const int32_t *__restrict__ faces, const float *__restrict__ uvs,
                                                      const int32_t *__restrict__ fuv, int B, int S, int T, int L, int V,
                                                      float bias, float *__restrict__ lod) {
    const size_t HW = (size_t)S * S;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * HW) return;
    const int f = p2f[i];
    float lam = 0.f;
    if (f >= 0) {
        const size_t b = i / HW;
        const float *vn = ndc + b * (size_t)V * 3;
        double x[3], y[3], z[3], u[3], v[3], bb[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int vj = faces[3 * f + j], tj = fuv[3 * f + j];
            x[j] = vn[3 * vj]; y[j] = vn[3 * vj + 1]; z[j] = vn[3 * vj + 2];
            u[j] = uvs[2 * tj]; v[j] = uvs[2 * tj + 1];
            bb[j] = bary[3 * i + j];
        }
        const double A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
        if (A != 0.0) {
            const double zp = zbuf[i];
            const double dax[3] = {(y[1] - y[2]) / A, (y[2] - y[0]) / A, (y[0] - y[1]) / A};
            const double day[3] = {(x[2] - x[1]) / A, (x[0] - x[2]) / A, (x[1] - x[0]) / A};
            const double sx = dax[0] / z[0] + dax[1] / z[1] + dax[2] / z[2];
            const double sy = day[0] / z[0] + day[1] / z[1] + day[2] / z[2];
            double dux = 0.0, dvx = 0.0, duy = 0.0, dvy = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double dbx = zp * (dax[j] / z[j] - bb[j] * sx), dby = zp * (day[j] / z[j] - bb[j] * sy);
                dux += dbx * u[j]; dvx += dbx * v[j];
                duy += dby * u[j]; dvy += dby * v[j];
            }
            const double px = (double)(T - 1) * 2.0 / (double)S;
            const double rx = hypot(dux, dvx) * px, ry = hypot(duy, dvy) * px;
            const double rho = rx > ry ? rx : ry;
            if (rho > 1.0) {                                  // (a NaN rho fails the comparison: 0)
                const double l = log2(rho) + (double)bias;
                lam = (float)(l > 0.0 ? (l < (double)(L - 1) ? l : (double)(L - 1)) : 0.0);
            }
        }
    }
    lod[i] = lam;
}

// ---------------------------------------------------------------------------------------------------- sample
// the footprint on level l >= 1 (side n = T >> l) of the level-0 position (ix, iy); cx / cy: this level's own clamp acted
__device__ __forceinline__ Footprint level_footprint(float ix, float iy, int l, int n) {
    Footprint o;
    const float inv = 1.0f / (float)(1 << l);               // a power of two: the product is the exact quotient
    float jx = (ix + 0.5f) * inv - 0.5f, jy = (iy + 0.5f) * inv - 0.5f;
    o.cx = false; o.cy = false;
    if (!(jx >= 0.f)) { jx = 0.f; o.cx = true; } else if (jx > (float)(n - 1)) { jx = (float)(n - 1); o.cx = true; }
    if (!(jy >= 0.f)) { jy = 0.f; o.cy = true; } else if (jy > (float)(n - 1)) { jy = (float)(n - 1); o.cy = true; }
    const float fx = floorf(jx), fy = floorf(jy);
    o.x0 = (int)fx; o.x1 = o.x0 + 1;
    const int yf0 = (int)fy, yf1 = yf0 + 1;
    o.wx1 = jx - fx; o.wx0 = 1.0f - o.wx1;
    o.wy1 = jy - fy; o.wy0 = 1.0f - o.wy1;
    o.vx0 = o.x0 >= 0 && o.x0 < n; o.vx1 = o.x1 >= 0 && o.x1 < n;
    o.vy0 = yf0 >= 0 && yf0 < n;   o.vy1 = yf1 >= 0 && yf1 < n;
    o.r0 = (n - 1) - yf0; o.r1 = (n - 1) - yf1;
    o.ix = jx; o.iy = jy;
    return o;
}

// lambda as the kernels use it: inside [0, L-1] whatever the plane holds (a NaN is 0), so no level index leaves the pyramid
__device__ __forceinline__ float safe_lod(float lam, int L) {
    return !(lam > 0.f) ? 0.f : fminf(lam, (float)(L - 1));
}

// the four taps of one level, channel c, in shade_fwd_kernel's order; a tap that does not exist is never multiplied
__device__ __forceinline__ float bilinear(const float *__restrict__ lvl, int n, const Footprint &q, int c) {
    const float w00 = q.wx0 * q.wy0, w01 = q.wx1 * q.wy0, w10 = q.wx0 * q.wy1, w11 = q.wx1 * q.wy1;
    float t = 0.f;
    if (q.vy0 && q.vx0) t += lvl[((size_t)q.r0 * n + q.x0) * 3 + c] * w00;
    if (q.vy0 && q.vx1) t += lvl[((size_t)q.r0 * n + q.x1) * 3 + c] * w01;
    if (q.vy1 && q.vx0) t += lvl[((size_t)q.r1 * n + q.x0) * 3 + c] * w10;
    if (q.vy1 && q.vx1) t += lvl[((size_t)q.r1 * n + q.x1) * 3 + c] * w11;
    return t;
}

__global__ __launch_bounds__(256) void shade_mip_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ bary,
                                                            const float *__restrict__ zbuf, const float *__restrict__ dists,
                                                            const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                                            const float *__restrict__ pyr, const float *__restrict__ lod,
                                                            int B, int S, int T, int L, Levels lv,
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
    const float b0 = bary[3 * i], b1 = bary[3 * i + 1], b2 = bary[3 * i + 2];
    const FragUV fu = frag_uv(uvs, fuv, f, b0, b1, b2);
    const float u = fu.u, v = fu.v;
    const Footprint q0 = uv_footprint(u, v, T);
    const Blend bl = blend_k1(dists[i], zbuf[i]);
    const float lam = safe_lod(lod[i], L);
    const int l0 = min((int)floorf(lam), L - 1);
    const float t = lam - (float)l0;
    const Footprint qa = l0 == 0 ? q0 : level_footprint(q0.ix, q0.iy, l0, T >> l0);
    const float *la = pyr + (size_t)lv.off[l0] * 3;
    float texel[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) texel[c] = bilinear(la, T >> l0, qa, c);
    if (t != 0.f) {                                      // (t > 0 implies l0 < L - 1: lambda <= L - 1)
        const int l1 = l0 + 1;
        const Footprint qb = level_footprint(q0.ix, q0.iy, l1, T >> l1);
        const float *lb = pyr + (size_t)lv.off[l1] * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) texel[c] = (1.0f - t) * texel[c] + t * bilinear(lb, T >> l1, qb, c);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * HW] = (bl.wnum * texel[c] + bl.delta * 1.0f) / bl.denom;
    mask[i] = ((1.0f - (1.0f - bl.prob)) > 0.f) ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------------- backward
// what one level of a pixel's pair hands to the scatter and to d/d(ix, iy)
struct LevelDep {
    int texel[4];
    float w[4], g[3];
    unsigned valid;
};

// fills `d` for level l (footprint q, side n, texel offset off, channel factors g) and adds the level's d/d(ix_0, iy_0)
__device__ __forceinline__ void level_bwd(const float *__restrict__ lvl, int n, int off, const Footprint &q, int l, const float g[3],
                                          bool want_uv, LevelDep &d, float &gix, float &giy, bool first) {
    const int e00 = q.r0 * n + q.x0, e01 = q.r0 * n + q.x1, e10 = q.r1 * n + q.x0, e11 = q.r1 * n + q.x1;
    d.texel[0] = off + e00; d.texel[1] = off + e01; d.texel[2] = off + e10; d.texel[3] = off + e11;
    d.w[0] = q.wx0 * q.wy0; d.w[1] = q.wx1 * q.wy0; d.w[2] = q.wx0 * q.wy1; d.w[3] = q.wx1 * q.wy1;
    d.g[0] = g[0]; d.g[1] = g[1]; d.g[2] = g[2];
    d.valid = (q.vy0 && q.vx0 ? 1u : 0u) | (q.vy0 && q.vx1 ? 2u : 0u) | (q.vy1 && q.vx0 ? 4u : 0u) | (q.vy1 && q.vx1 ? 8u : 0u);
    if (!want_uv) return;
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = (q.vy0 && q.vx0) ? lvl[(size_t)e00 * 3 + c] : 0.f, t01 = (q.vy0 && q.vx1) ? lvl[(size_t)e01 * 3 + c] : 0.f;
        const float t10 = (q.vy1 && q.vx0) ? lvl[(size_t)e10 * 3 + c] : 0.f, t11 = (q.vy1 && q.vx1) ? lvl[(size_t)e11 * 3 + c] : 0.f;
        gx += g[c] * ((t01 - t00) * q.wy0 + (t11 - t10) * q.wy1);
        gy += g[c] * ((t10 - t00) * q.wx0 + (t11 - t01) * q.wx1);
    }
    if (l > 0) {                     // d ix_l / d ix_0 = 2^-l, 0 where this level's clamp acted
        const float inv = 1.0f / (float)(1 << l);
        gx = q.cx ? 0.f : gx * inv;
        gy = q.cy ? 0.f : gy * inv;
    }
    gix = first ? gx : gix + gx;
    giy = first ? gy : giy + gy;
}

// DET 0: float LDS table + float global atomics into the packed-pyramid gradient.  DET 1: 64-bit fixed point (det.h).
template <int DET>
__global__ __launch_bounds__(256) void shade_mip_bwd_kernel(const float *__restrict__ grad_rgb, const int32_t *__restrict__ p2f,
                                                            const float *__restrict__ bary, const float *__restrict__ zbuf,
                                                            const float *__restrict__ dists, const float *__restrict__ uvs,
                                                            const int32_t *__restrict__ fuv, const float *__restrict__ pyr,
                                                            const float *__restrict__ lod, int B, int S, int T, int L, Levels lv,
                                                            int tiles_x, float *__restrict__ gpyr, float *__restrict__ guv,
                                                            float *__restrict__ gbary,
                                                            const st3d_det::DetHeader *__restrict__ det) {
    typedef typename std::conditional<DET != 0, unsigned long long, float>::type acc_t;
    ST3D_TEXEL_BINS(bins, acc_t);          // >= 2 x the 4 x 256 corners a tile deposits on ONE level
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
    if (gpyr && !__syncthreads_or(f >= 0)) return;       // the same answer in every lane: the whole workgroup leaves
    LevelDep lo, up;
    lo.valid = 0; up.valid = 0;
    if (f >= 0) {
        const bool want_uv = guv || gbary;
        const float b0 = bary[3 * i], b1 = bary[3 * i + 1], b2 = bary[3 * i + 2];
        const FragUV fu = frag_uv(uvs, fuv, f, b0, b1, b2);
        const int u0 = fu.u0, u1 = fu.u1, u2 = fu.u2;
        const float u = fu.u, v = fu.v;
        const Footprint q0 = uv_footprint(u, v, T);
        const Blend bl = blend_k1(dists[i], zbuf[i]);
        const float k = bl.wnum / bl.denom;
        const float *g = grad_rgb + (size_t)b * 3 * HW + p;
        const float gk[3] = {g[0] * k, g[HW] * k, g[2 * HW] * k};
        const float lam = safe_lod(lod[i], L);
        const int l0 = min((int)floorf(lam), L - 1);
        const float t = lam - (float)l0;
        float gix = 0.f, giy = 0.f;
        const Footprint qa = l0 == 0 ? q0 : level_footprint(q0.ix, q0.iy, l0, T >> l0);
        if (t == 0.f) {
            level_bwd(pyr + (size_t)lv.off[l0] * 3, T >> l0, lv.off[l0], qa, l0, gk, want_uv, lo, gix, giy, true);
        } else {
            const float ga[3] = {gk[0] * (1.0f - t), gk[1] * (1.0f - t), gk[2] * (1.0f - t)};
            const float gb[3] = {gk[0] * t, gk[1] * t, gk[2] * t};
            const int l1 = l0 + 1;
            const Footprint qb = level_footprint(q0.ix, q0.iy, l1, T >> l1);
            level_bwd(pyr + (size_t)lv.off[l0] * 3, T >> l0, lv.off[l0], qa, l0, ga, want_uv, lo, gix, giy, true);
            level_bwd(pyr + (size_t)lv.off[l1] * 3, T >> l1, lv.off[l1], qb, l1, gb, want_uv, up, gix, giy, false);
        }
        if (want_uv) {
            const float gu = q0.cx ? 0.f : gix * (float)(T - 1);
            const float gv = q0.cy ? 0.f : giy * (float)(T - 1);
            if (guv) { guv[2 * i] = gu; guv[2 * i + 1] = gv; }
            if (gbary) {      // uv = sum_i b_i * uv_i
                gbary[3 * i] = gu * uvs[2 * u0] + gv * uvs[2 * u0 + 1];
                gbary[3 * i + 1] = gu * uvs[2 * u1] + gv * uvs[2 * u1 + 1];
                gbary[3 * i + 2] = gu * uvs[2 * u2] + gv * uvs[2 * u2 + 1];
            }
        }
    }
    if (!gpyr) return;
    bins.reset();
    bins.scatter(lo.texel, lo.w, lo.g, lo.valid, dscale, gpyr);
    __syncthreads();                                     // the table is free for the next pass
    if (!__syncthreads_or(up.valid != 0)) return;        // no pixel of the tile sits between two levels
    bins.reset();
    bins.scatter(up.texel, up.w, up.g, up.valid, dscale, gpyr);
}

using st3d_det::kPixelPartials;

int launch_adjoint(const float *gp, int T, int L, int accumulate, float *gtex, hipStream_t s) {
    const size_t n = (size_t)T * T * 3;
    mip_adjoint_kernel<<<st3d::cdiv((long)n, 256), 256, 0, s>>>(gp, T, L, levels_of(T, L), accumulate, gtex);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

}  // namespace

extern "C" size_t st3d_mip_numel(int T, int L) {
    return shape_ok(T, L) ? (size_t)levels_of(T, L).off[L] * 3 : 0;
}

extern "C" int st3d_mip_build(const float *texture, int T, int L, float *pyramid, st3d_stream_t stream) {
    ST3D_CHECK_ARG(texture && pyramid && texture != pyramid);
    ST3D_CHECK_ARG(shape_ok(T, L));
    hipStream_t s = st3d::as_stream(stream);
    const Levels lv = levels_of(T, L);
    const int K = L - 1 < KTILE ? L - 1 : KTILE;
    mip_build_tile_kernel<<<dim3(st3d::cdiv(T, FT), st3d::cdiv(T, FT)), 256, 0, s>>>(texture, T, K, lv, pyramid);
    ST3D_LAUNCH_CHECK();
    if (L - 1 > K) {
        mip_build_tail_kernel<<<1, 1024, 0, s>>>(T, K, L, lv, pyramid);
        ST3D_LAUNCH_CHECK();
    }
    return ST3D_OK;
}

extern "C" int st3d_mip_adjoint(const float *grad_pyramid, int T, int L, int accumulate, float *grad_texture,
                                st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_pyramid && grad_texture && grad_pyramid != grad_texture);
    ST3D_CHECK_ARG(shape_ok(T, L));
    return launch_adjoint(grad_pyramid, T, L, accumulate ? 1 : 0, grad_texture, st3d::as_stream(stream));
}

extern "C" int st3d_mip_lod(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *verts_ndc,
                            const int32_t *faces, const float *verts_uvs, const int32_t *faces_uvs, int B, int S, int T, int L,
                            int V, int F, int VT, float bias, float *lod, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && verts_ndc && faces && verts_uvs && faces_uvs && lod);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxRaster && V > 0 && F > 0 && VT > 0);
    ST3D_CHECK_ARG(shape_ok(T, L));
    ST3D_CHECK_ARG(bias == bias);
    const size_t n = (size_t)B * S * S;
    mip_lod_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(pix_to_face, bary, zbuf, verts_ndc, faces,
                                                                                 verts_uvs, faces_uvs, B, S, T, L, V, bias, lod);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_shade_mip_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                                  const float *verts_uvs, const int32_t *faces_uvs, const float *pyramid, const float *lod,
                                  int B, int S, int T, int L, int F, int VT, float *rgb, float *mask, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && pyramid && lod && rgb && mask);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxRaster && F > 0 && VT > 0);
    ST3D_CHECK_ARG(shape_ok(T, L));
    const size_t n = (size_t)B * S * S;
    shade_mip_fwd_kernel<<<st3d::cdiv((long)n, 256), 256, 0, st3d::as_stream(stream)>>>(
        pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, pyramid, lod, B, S, T, L, levels_of(T, L), rgb, mask);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_shade_mip_bwd_workspace_bytes(int T, int L) {
    const size_t n = st3d_mip_numel(T, L);
    return n ? st3d_det::workspace_bytes(n, kPixelPartials) : 0;
}

// grad_pyramid: st3d_mip_numel(T, L) floats of the caller's, OVERWRITTEN with the per-level texel gradient before the fold
// (needed whenever grad_texture is given).  Every deposit is |g| times blend, level and bilinear weights <= 1, so the sum of
// |grad_rgb| bounds any accumulator (st3d_det::det_abs_sum_kernel, as st3d_shade_bwd_det).
extern "C" int st3d_shade_mip_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                                  const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *pyramid,
                                  const float *lod, int B, int S, int T, int L, int F, int VT, float *grad_pyramid,
                                  float *grad_texture, float *grad_uv, float *grad_bary, void *workspace, size_t workspace_bytes,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_rgb && pix_to_face && bary && zbuf && dists && verts_uvs && faces_uvs && pyramid && lod);
    ST3D_CHECK_ARG(grad_texture || grad_uv || grad_bary);
    ST3D_CHECK_ARG(!grad_texture == !grad_pyramid);
    ST3D_CHECK_ARG(grad_texture || !workspace);
    ST3D_CHECK_ARG(B > 0 && S > 0 && S <= kMaxRaster && F > 0 && VT > 0);
    ST3D_CHECK_ARG(shape_ok(T, L));
    hipStream_t s = st3d::as_stream(stream);
    const Levels lv = levels_of(T, L);
    const size_t nacc = (size_t)lv.off[L] * 3;
    const int tiles = (S + 15) / 16;
    const dim3 grid(tiles * tiles, B);
    if (!workspace) {
        if (grad_pyramid) ST3D_HIP(hipMemsetAsync(grad_pyramid, 0, nacc * sizeof(float), s));
        shade_mip_bwd_kernel<0><<<grid, 256, 0, s>>>(grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, pyramid, lod,
                                                     B, S, T, L, lv, tiles, grad_pyramid, grad_uv, grad_bary, nullptr);
        ST3D_LAUNCH_CHECK();
        return grad_texture ? launch_adjoint(grad_pyramid, T, L, 1, grad_texture, s) : ST3D_OK;
    }
    ST3D_CHECK_ARG(workspace_bytes >= st3d_shade_mip_bwd_workspace_bytes(T, L) && ((uintptr_t)workspace & 15) == 0);
    const st3d_det::DetRun det(workspace, kPixelPartials, nacc);
    st3d_det::det_abs_sum_kernel<<<kPixelPartials, 256, 0, s>>>(grad_rgb, (size_t)B * 3 * S * S, det.partials);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    shade_mip_bwd_kernel<1><<<grid, 256, 0, s>>>(grad_rgb, pix_to_face, bary, zbuf, dists, verts_uvs, faces_uvs, pyramid, lod, B, S,
                                                 T, L, lv, tiles, reinterpret_cast<float *>(det.acc), grad_uv, grad_bary, det.hdr);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.convert(0, grad_pyramid, s));
    return launch_adjoint(grad_pyramid, T, L, 1, grad_texture, s);
}
