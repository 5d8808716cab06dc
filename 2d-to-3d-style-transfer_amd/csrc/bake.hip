// bake.hip -- bake a batch of views into the texture map by UV-space back-projection ("Baking views into the
// texture"): walk the texels, not the pixels.  Two stages, both gathers, neither with a float atomic, so two runs give the
// same bits; tests/_bakeref.py restates both in fp64.
//
// 1. texel -> surface (once per mesh).  Texel (row r, column x) of the map as stored sits at (x, T-1-r) in texel units
//    (UV x (T-1): the inverse of st3d_k1::uv_footprint).  It belongs to the UV triangle of the smallest squared distance d2
//    (0 inside or on the triangle, either winding), the lowest face among equals, provided d2 <= pad^2.
//      bake_claim:   one wave per face strides the texels of the face's padded bounding box; every texel within pad takes an
//                    integer atomicMin on the 64-bit key (bits of d2) << 32 | face (a non-negative float's bits order like
//                    the float), 8 B per texel, at most one atomic per (face, texel of its box)
//      bake_decode:  one thread per texel reads its key and recomputes the winner's closest point -> t2f, tbary (16 B written)
// 2. bake_views: one thread per texel with t2f >= 0 walks the B views in index order (fixed order of the sums, no atomics):
//    surface point and face normal, projection as project_verts_kernel, nearest-pixel visibility against the hard K = 1
//    fragments, bilinear colour over covered taps, weight |cos|^power.  Reads 16 B of map per texel, 36 B of face, and per
//    view 8 B of fragment + up to 4 x (4 + 12) B of taps; writes 16 B.
//    bake_resolve: acc.rgb / acc.w where acc.w > 0, the fallback map elsewhere.
// Built with -ffp-contract=off and the correctly rounded division, like cover.hip: the roundings are the ones written here.
#include "common.h"

namespace {

constexpr int kMaxSide = 16384;             // T*T <= 2^28: a texel index fits an int32 with room to spare
constexpr int kThreads = 256, kWaves = kThreads / st3d::kWave;
constexpr float kMaxPad = 8.0f;
constexpr unsigned long long kNoFace = ~0ull;

struct Closest { double d2, b0, b1, b2; bool ok; };

__device__ __forceinline__ void seg_closest(double px, double py, double ax, double ay, double bx, double by, double &d2, double &t) {
    const double ex = bx - ax, ey = by - ay;
    const double den = ex * ex + ey * ey;
    t = den > 0.0 ? ((px - ax) * ex + (py - ay) * ey) / den : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    // at t = 1 the end point itself, not a + 1 (b - a): the faces that share a vertex then find the same distance to it, bit
    // for bit, and the lowest of them wins
    const double dx = px - (t < 1.0 ? ax + t * ex : bx), dy = py - (t < 1.0 ? ay + t * ey : by);
    d2 = dx * dx + dy * dy;
}

// the closest point of triangle (a, b, c) to p, all in texel units: its squared distance and its barycentrics.
// ok = false: the triangle has no area.  Inside or on the triangle (the three edge functions, signed by the winding, all >= 0)
// d2 is exactly 0; outside, the nearest of the three edges decides, the first of ab, bc, ca among equals.
// fp64: a chart's triangles are a texel or less across while their coordinates run up to T, so fp32 would leave the
// barycentrics of a sliver with errors of 1e-4; this stage runs once per mesh, and in fp64 it is its restatement's bits.
__device__ __forceinline__ Closest closest_point(double px, double py, double ax, double ay, double bx, double by, double cx,
                                                 double cy) {
    Closest o;
    o.d2 = 0.0; o.b0 = o.b1 = o.b2 = 0.0;
    double area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
    o.ok = area != 0.0;
    if (!o.ok) return o;
    double e0 = (bx - px) * (cy - py) - (by - py) * (cx - px);
    double e1 = (cx - px) * (ay - py) - (cy - py) * (ax - px);
    double e2 = (ax - px) * (by - py) - (ay - py) * (bx - px);
    if (area < 0.0) { area = -area; e0 = -e0; e1 = -e1; e2 = -e2; }
    if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
        o.b0 = e0 / area; o.b1 = e1 / area; o.b2 = e2 / area;
        return o;
    }
    double d, t;
    seg_closest(px, py, ax, ay, bx, by, d, t);
    o.d2 = d; o.b0 = 1.0 - t; o.b1 = t; o.b2 = 0.0;
    seg_closest(px, py, bx, by, cx, cy, d, t);
    if (d < o.d2) { o.d2 = d; o.b0 = 0.0; o.b1 = 1.0 - t; o.b2 = t; }
    seg_closest(px, py, cx, cy, ax, ay, d, t);
    if (d < o.d2) { o.d2 = d; o.b0 = t; o.b1 = 0.0; o.b2 = 1.0 - t; }
    return o;
}

struct UVTri { double ax, ay, bx, by, cx, cy; bool ok; };

// the face's UV corners in texel units; ok = false: a corner index outside verts_uvs (such a face is skipped like one without
// area, never read through)
__device__ __forceinline__ UVTri uv_triangle(const float *__restrict__ uvs, const int32_t *__restrict__ fuv, int VT, int f, int T) {
    const int i0 = fuv[3 * f], i1 = fuv[3 * f + 1], i2 = fuv[3 * f + 2];
    const double s = (double)(T - 1);
    UVTri o;
    o.ok = (unsigned)i0 < (unsigned)VT && (unsigned)i1 < (unsigned)VT && (unsigned)i2 < (unsigned)VT;
    if (!o.ok) { o.ax = o.ay = o.bx = o.by = o.cx = o.cy = 0.0; return o; }
    o.ax = (double)uvs[2 * i0] * s; o.ay = (double)uvs[2 * i0 + 1] * s;
    o.bx = (double)uvs[2 * i1] * s; o.by = (double)uvs[2 * i1 + 1] * s;
    o.cx = (double)uvs[2 * i2] * s; o.cy = (double)uvs[2 * i2 + 1] * s;
    return o;
}

__global__ __launch_bounds__(kThreads) void bake_claim_kernel(const float *__restrict__ uvs, const int32_t *__restrict__ fuv,
                                                              int VT, int F, int T, float pad, float pad2,
                                                              unsigned long long *__restrict__ keys) {
    const int lane = threadIdx.x & (st3d::kWave - 1);
    const long f = (long)blockIdx.x * kWaves + threadIdx.x / st3d::kWave;
    if (f >= F) return;
    const UVTri q = uv_triangle(uvs, fuv, VT, (int)f, T);
    if (!q.ok) return;
    const double lo_x = fmin(q.ax, fmin(q.bx, q.cx)) - pad, hi_x = fmax(q.ax, fmax(q.bx, q.cx)) + pad;
    const double lo_y = fmin(q.ay, fmin(q.by, q.cy)) - pad, hi_y = fmax(q.ay, fmax(q.by, q.cy)) + pad;
    const double top = (double)(T - 1);
    if (!(hi_x >= 0.0 && hi_y >= 0.0 && lo_x <= top && lo_y <= top)) return;      // off the map, or a NaN coordinate
    // up to one texel of slack each side: the d2 <= pad^2 test below decides, never the rounding of the box
    const int x0 = (int)fmax(floor(lo_x), 0.0), x1 = (int)fmin(ceil(hi_x), top);
    const int y0 = (int)fmax(floor(lo_y), 0.0), y1 = (int)fmin(ceil(hi_y), top);
    const int w = x1 - x0 + 1;
    const long n = (long)w * (y1 - y0 + 1);
    for (long i = lane; i < n; i += st3d::kWave) {
        const int ix = x0 + (int)(i % w), iy = y0 + (int)(i / w);
        const Closest c = closest_point((double)ix, (double)iy, q.ax, q.ay, q.bx, q.by, q.cx, q.cy);
        if (!c.ok) return;
        const float d2 = (float)c.d2;           // the distances are compared as rounded to fp32: 32 bits of the key
        if (!(d2 <= pad2)) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)f;
        atomicMin(keys + ((size_t)(T - 1 - iy) * T + ix), key);
    }
}

__global__ __launch_bounds__(kThreads) void bake_decode_kernel(const float *__restrict__ uvs, const int32_t *__restrict__ fuv, int VT, int T,
                                                               const unsigned long long *__restrict__ keys,
                                                               int32_t *__restrict__ t2f, float *__restrict__ tbary) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T * T) return;
    const unsigned long long key = keys[t];
    int f = -1;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    if (key != kNoFace) {
        f = (int)(uint32_t)(key & 0xffffffffull);
        const int r = t / T, x = t - r * T;
        const UVTri q = uv_triangle(uvs, fuv, VT, f, T);        // a winner passed the index test in bake_claim
        const Closest c = closest_point((double)x, (double)(T - 1 - r), q.ax, q.ay, q.bx, q.by, q.cx, q.cy);
        b0 = (float)c.b0; b1 = (float)c.b1; b2 = (float)c.b2;
    }
    t2f[t] = f;
    tbary[3 * (size_t)t] = b0; tbary[3 * (size_t)t + 1] = b1; tbary[3 * (size_t)t + 2] = b2;
}

// one bilinear tap: dropped (weight 0) when its pixel shows no face
__device__ __forceinline__ void tap(const int32_t *__restrict__ p2f, const float *__restrict__ img, size_t HW, int S, int y, int x,
                                    float w, float &r, float &g, float &b, float &sum) {
    const size_t i = (size_t)y * S + x;
    if (p2f[i] < 0) return;
    r += w * img[i]; g += w * img[HW + i]; b += w * img[2 * HW + i];
    sum += w;
}

template <bool BEST>
__global__ __launch_bounds__(kThreads) void bake_views_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                              const int32_t *__restrict__ t2f, const float *__restrict__ tbary,
                                                              int V, int F, int TT, const float *__restrict__ R,
                                                              const float *__restrict__ Tr,
                                                              const float *__restrict__ images, const int32_t *__restrict__ p2f,
                                                              const float *__restrict__ zbuf, int B, int S, float s, float power,
                                                              float min_cos, float depth_tol, float *__restrict__ acc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= TT) return;
    const int f = t2f[t];
    if (f < 0 || f >= F) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
    const float ax = verts[3 * i0], ay = verts[3 * i0 + 1], az = verts[3 * i0 + 2];
    const float bx = verts[3 * i1], by = verts[3 * i1 + 1], bz = verts[3 * i1 + 2];
    const float cx = verts[3 * i2], cy = verts[3 * i2 + 1], cz = verts[3 * i2 + 2];
    const float b0 = tbary[3 * (size_t)t], b1 = tbary[3 * (size_t)t + 1], b2 = tbary[3 * (size_t)t + 2];
    const float Px = b0 * ax + b1 * bx + b2 * cx, Py = b0 * ay + b1 * by + b2 * cy, Pz = b0 * az + b1 * bz + b2 * cz;
    const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const float nl = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-12f);
    nx /= nl; ny /= nl; nz /= nl;
    const size_t HW = (size_t)S * S;
    float ar = acc[4 * (size_t)t], ag = acc[4 * (size_t)t + 1], ab = acc[4 * (size_t)t + 2], aw = acc[4 * (size_t)t + 3];
    const float fS = (float)S;
    for (int b = 0; b < B; ++b) {
        const float *r = R + 9 * b, *tr = Tr + 3 * b;
        const float xv = Px * r[0] + Py * r[3] + Pz * r[6] + tr[0];
        const float yv = Px * r[1] + Py * r[4] + Pz * r[7] + tr[1];
        const float zv = Px * r[2] + Py * r[5] + Pz * r[8] + tr[2];
        if (!(zv > 0.5f)) continue;
        const float x_ndc = (s * xv) / zv, y_ndc = (s * yv) / zv;
        const float ix = ((1.0f - x_ndc) * fS - 1.0f) / 2.0f, iy = ((1.0f - y_ndc) * fS - 1.0f) / 2.0f;
        const float rx = rintf(ix), ry = rintf(iy);
        if (!(rx >= 0.f && rx < fS && ry >= 0.f && ry < fS)) continue;
        const int px = (int)rx, py = (int)ry;
        const int32_t *pb = p2f + (size_t)b * HW;
        const int g = pb[(size_t)py * S + px];
        if (g < 0) continue;
        if (g != f && !(fabsf(zv - zbuf[(size_t)b * HW + (size_t)py * S + px]) <= depth_tol * zv)) continue;
        // towards the camera centre C = -T R^T (X_view = X_world R + T)
        float dx = -(tr[0] * r[0] + tr[1] * r[1] + tr[2] * r[2]) - Px;
        float dy = -(tr[0] * r[3] + tr[1] * r[4] + tr[2] * r[5]) - Py;
        float dz = -(tr[0] * r[6] + tr[1] * r[7] + tr[2] * r[8]) - Pz;
        const float dl = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
        dx /= dl; dy /= dl; dz /= dl;
        const float c = fabsf(nx * dx + ny * dy + nz * dz);
        if (!(c >= min_cos)) continue;
        const float fx = floorf(ix), fy = floorf(iy);
        const float wx1 = ix - fx, wx0 = 1.0f - wx1, wy1 = iy - fy, wy0 = 1.0f - wy1;
        const int x0 = min(max((int)fx, 0), S - 1), x1 = min(max((int)fx + 1, 0), S - 1);
        const int y0 = min(max((int)fy, 0), S - 1), y1 = min(max((int)fy + 1, 0), S - 1);
        const float *img = images + (size_t)b * 3 * HW;
        float cr = 0.f, cg = 0.f, cb = 0.f, sum = 0.f;
        tap(pb, img, HW, S, y0, x0, wy0 * wx0, cr, cg, cb, sum);
        tap(pb, img, HW, S, y0, x1, wy0 * wx1, cr, cg, cb, sum);
        tap(pb, img, HW, S, y1, x0, wy1 * wx0, cr, cg, cb, sum);
        tap(pb, img, HW, S, y1, x1, wy1 * wx1, cr, cg, cb, sum);
        if (!(sum > 0.f)) continue;             // cannot happen: the nearest pixel is covered and carries >= 1/4
        cr /= sum; cg /= sum; cb /= sum;
        const float w = powf(c, power);
        if (BEST) {
            if (w > aw) { ar = w * cr; ag = w * cg; ab = w * cb; aw = w; }
        } else {
            ar += w * cr; ag += w * cg; ab += w * cb; aw += w;
        }
    }
    acc[4 * (size_t)t] = ar; acc[4 * (size_t)t + 1] = ag; acc[4 * (size_t)t + 2] = ab; acc[4 * (size_t)t + 3] = aw;
}

__global__ __launch_bounds__(kThreads) void bake_resolve_kernel(const float *__restrict__ acc, const float *__restrict__ fallback,
                                                                int TT, float *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= TT) return;
    const float w = acc[4 * (size_t)t + 3];
    const bool baked = w > 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * (size_t)t + k] = baked ? acc[4 * (size_t)t + k] / w : fallback[3 * (size_t)t + k];
}

inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" size_t st3d_bake_workspace_bytes(int T) {
    return (T >= 2 && T <= kMaxSide) ? (size_t)T * T * sizeof(unsigned long long) : 0;
}

extern "C" int st3d_bake_surface(const float *verts_uvs, const int32_t *faces_uvs, int VT, int F, int T, float pad, void *workspace,
                                 size_t workspace_bytes, int32_t *t2f, float *tbary, st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts_uvs && faces_uvs && workspace && t2f && tbary);
    ST3D_CHECK_ARG(VT >= 1 && F >= 1 && T >= 2 && T <= kMaxSide);
    ST3D_CHECK_ARG(pad >= 0.f && pad <= kMaxPad);
    ST3D_CHECK_ARG(aligned(workspace, 8) && workspace_bytes >= st3d_bake_workspace_bytes(T));
    hipStream_t s = st3d::as_stream(stream);
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    ST3D_HIP(hipMemsetAsync(keys, 0xff, st3d_bake_workspace_bytes(T), s));
    bake_claim_kernel<<<st3d::cdiv(F, kWaves), kThreads, 0, s>>>(verts_uvs, faces_uvs, VT, F, T, pad, pad * pad, keys);
    bake_decode_kernel<<<st3d::cdiv((long)T * T, kThreads), kThreads, 0, s>>>(verts_uvs, faces_uvs, VT, T, keys, t2f, tbary);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_bake_views(const float *verts, const int32_t *faces, int V, int F, const int32_t *t2f, const float *tbary, int Tt,
                               const float *R, const float *T, const float *images, const int32_t *pix_to_face,
                               const float *zbuf, int B, int S, float inv_tan_half_fov, int mode, float power, float min_cos,
                               float depth_tol, float *acc, st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && faces && t2f && tbary && R && T && images && pix_to_face && zbuf && acc);
    ST3D_CHECK_ARG(V >= 1 && F >= 1 && Tt >= 2 && Tt <= kMaxSide && B >= 1 && S >= 1 && S <= 4096);
    ST3D_CHECK_ARG(mode == ST3D_BAKE_MEAN || mode == ST3D_BAKE_BEST);
    ST3D_CHECK_ARG(inv_tan_half_fov > 0.f && power >= 0.f && min_cos >= 0.f && min_cos <= 1.f && depth_tol >= 0.f);
    const int TT = Tt * Tt;
    hipStream_t s = st3d::as_stream(stream);
    if (mode == ST3D_BAKE_BEST)
        bake_views_kernel<true><<<st3d::cdiv(TT, kThreads), kThreads, 0, s>>>(verts, faces, t2f, tbary, V, F, TT, R, T, images, pix_to_face,
                                                                              zbuf, B, S, inv_tan_half_fov, power, min_cos,
                                                                              depth_tol, acc);
    else
        bake_views_kernel<false><<<st3d::cdiv(TT, kThreads), kThreads, 0, s>>>(verts, faces, t2f, tbary, V, F, TT, R, T, images, pix_to_face,
                                                                               zbuf, B, S, inv_tan_half_fov, power, min_cos,
                                                                               depth_tol, acc);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_bake_resolve(const float *acc, const float *fallback, int Tt, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(acc && fallback && out);
    ST3D_CHECK_ARG(Tt >= 2 && Tt <= kMaxSide);
    ST3D_CHECK_ARG(out != acc);
    const int TT = Tt * Tt;
    bake_resolve_kernel<<<st3d::cdiv(TT, kThreads), kThreads, 0, st3d::as_stream(stream)>>>(acc, fallback, TT, out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
