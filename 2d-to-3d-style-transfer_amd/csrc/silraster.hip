// silraster.hip -- the SILHOUETTE rasteriser: from face records straight to SoftSilhouetteShader's alpha (and to the
// silhouette loss), and from d loss / d alpha straight back to the projected vertices, for faces_per_pixel K = 1..64, WITHOUT
// fragments in memory.  alpha is one number per pixel and prod (1 - prob_k) does not care which fragment is which, so the
// S*S*K*24 B of fragments the general rasteriser (soft.hip) writes -- 2.5 GB for 8 views of 512^2 at K = 50 -- are never
// needed.  Between forward and backward 12 bytes per pixel are kept (16 with the fused loss), whatever K is:
//     keep = prod_k (1 - prob_k), and the CUT: (pz, record index) of the last fragment taken.
// The backward walks the same candidates again; a candidate at or before the cut is a fragment, no sorting needed.
//
// Semantics = oracle/raster_ref.c:ref_rasterize_k3 + sigmoid_alpha_blend: the candidates of a pixel are the records that pass
// ref_rasterize_k3's tests (same fp32 operation order; the file is built with -ffp-contract=off like soft.hip and
// silhouette.hip), the K nearest by (pz, record index) are taken, prob = 1 / (1 + expf(d / sigma)) and keep is multiplied in
// depth order: the expression of silhouette.hip:silhouette_pixel(), so at K <= 8 alpha equals st3d_silhouette_fwd on
// st3d_raster_soft_fwd's fragments bit for bit.  One corner differs from the oracle by definition: of the two halves of a
// quadrilateral split by the near plane the one nearer in the image plane represents the face, and that is decided per
// candidate by evaluating the sibling record ("halves first, then the K nearest"); the oracle decides it against its current
// K-list and so forgets a half that K nearer fragments had already pushed out.
//
// Forward: one 256-thread workgroup per 16x16 tile, order-preserving ballot compaction of the records whose padded bbox
// touches the tile into an LDS list (as raster_k_kernel); each lane keeps the 8 nearest candidates beyond its cut in
// registers -- (pz, d, index) only, no barycentrics --, folds them into keep, moves the cut, and the workgroup repeats the
// sweep while some lane has taken fewer than K and filled its list (__syncthreads_or).  Tiles whose pixels all have <= 8
// candidates (or K <= 8) sweep once.
// Backward: one sweep per tile; lanes whose d loss / d alpha * keep is zero do not evaluate anything, tiles without a live
// lane return at once.  The nine contributions of a fragment go through a per-tile LDS face table and then to global memory,
// as raster_k_bwd_kernel does: 64-bit fixed point with a bound pass (det.h; bitwise reproducible) or float atomics.
// NaN: a candidate whose depth or distance is NaN cannot be ordered; it poisons its pixel (keep = NaN), so alpha, the loss
// and -- through the bound pass -- the whole vertex gradient come out NaN.  Nothing is filtered.
#include <type_traits>

#include "common.h"
#include "det.h"
#include "softgeom.h"

namespace {

constexpr int TILE = 16;
constexpr int LIST_CAP = 512;
constexpr int KL = 8;                  // register-resident list of one pass
constexpr int KMAX = 64;
constexpr int kFaceSlots = 512, kProbe = 24;

struct Geo { float pz, d; bool inside; };

// the per-pixel tests of ref_rasterize_k3 on one valid record (validity -- code, zmax, degenerate area -- is in the record)
__device__ __forceinline__ bool sil_eval(float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2, float z2,
                                         float xf, float yf, float pad, float blur, int clip, int cull, int persp, Geo &g) {
    const float xmin = fminf(x0, fminf(x1, x2)) - pad, xmax = fmaxf(x0, fmaxf(x1, x2)) + pad;
    const float ymin = fminf(y0, fminf(y1, y2)) - pad, ymax = fmaxf(y0, fmaxf(y1, y2)) + pad;
    if (xf > xmax || xf < xmin || yf > ymax || yf < ymin) return false;
    const float face_area = edge_fn(x2, y2, x0, y0, x1, y1);
    if (cull && face_area < 0.f) return false;
    const float area = face_area + kEps;
    const float w0 = edge_fn(xf, yf, x1, y1, x2, y2) / area;
    const float w1 = edge_fn(xf, yf, x2, y2, x0, y0) / area;
    const float w2 = edge_fn(xf, yf, x0, y0, x1, y1) / area;
    float b0 = w0, b1 = w1, b2 = w2;
    if (persp) {
        const float t0 = w0 * z1 * z2, t1 = z0 * w1 * z2, t2 = z0 * z1 * w2;
        const float den = fmaxf(t0 + t1 + t2, kEps);
        b0 = t0 / den; b1 = t1 / den; b2 = t2 / den;
    }
    float c0 = b0, c1 = b1, c2 = b2;
    if (clip) {
        c0 = fminf(fmaxf(b0, 0.f), 1.f); c1 = fminf(fmaxf(b1, 0.f), 1.f); c2 = fminf(fmaxf(b2, 0.f), 1.f);
        const float s = fmaxf(c0 + c1 + c2, kEps);
        c0 /= s; c1 /= s; c2 /= s;
    }
    g.pz = c0 * z0 + c1 * z1 + c2 * z2;
    if (g.pz < 0.f) return false;
    g.inside = (b0 > 0.f) && (b1 > 0.f) && (b2 > 0.f);
    g.d = fminf(pld2(xf, yf, x0, y0, x1, y1), fminf(pld2(xf, yf, x1, y1, x2, y2), pld2(xf, yf, x2, y2, x0, y0)));
    return g.inside || !(g.d >= blur);
}

struct View { float xf, yf, pad, blur; int clip, cull, persp; };

// record `idx` is one half of a split quadrilateral and a candidate with distance d: does its sibling represent the face
// instead?  (the oracle keeps the earlier half unless the later one is strictly nearer in the image plane)
__device__ __forceinline__ bool sibling_wins(const float4 *__restrict__ rb, int idx, float d, const View &v) {
    const size_t o = (size_t)(idx ^ 1);
    const float4 r2 = rb[3 * o + 2];
    if (r2.y == 0.f) return false;
    const float4 r0 = rb[3 * o], r1 = rb[3 * o + 1];
    Geo g;
    if (!sil_eval(r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, v.xf, v.yf, v.pad, v.blur, v.clip, v.cull, v.persp, g))
        return false;
    return (idx & 1) ? !(d < g.d) : (g.d < d);
}

__device__ __forceinline__ float sel3(int i, float a, float b, float c) { return i == 0 ? a : (i == 1 ? b : c); }

// d loss / d (the face's three projected vertices) of one fragment for gd = d loss / d (signed distance): the distance branch of
// raster_k_frag_grad (soft.hip) -- nearest edge, first minimum, projection parameter constant; on a clipped record through
// the cut points p4 = cut(p1, p2, w2), p5 = cut(p1, p3, w3), w = (z1 - z_clip) / (z1 - z_far) -- written without indexed
// arrays, so nothing goes to scratch.  t: the record's triangle; ov: the face's own vertices; c9 = {d/dx0, d/dy0, d/dz0, ...}.
__device__ __forceinline__ void sil_frag_grad(const float t[9], bool inside, float gd, float px, float py, int code, float cw2,
                                              float cw3, const float ov[9], float z_clip, int persp, float c9[9]) {
    const float x0 = t[0], y0 = t[1], x1 = t[3], y1 = t[4], x2 = t[6], y2 = t[7];
    const float gdd = inside ? -gd : gd;
    const float d01 = pld2(px, py, x0, y0, x1, y1), d12 = pld2(px, py, x1, y1, x2, y2), d20 = pld2(px, py, x2, y2, x0, y0);
    int e = 0; float dm = d01;
    if (d12 < dm) { dm = d12; e = 1; }
    if (d20 < dm) { dm = d20; e = 2; }
    const float ax = sel3(e, x0, x1, x2), ay = sel3(e, y0, y1, y2), bx = sel3(e, x1, x2, x0), by = sel3(e, y1, y2, y0);
    const float bax = bx - ax, bay = by - ay, l2 = bax * bax + bay * bay;
    float gax, gay, gbx, gby;
    if (l2 <= kEps) {
        gax = 0.f; gay = 0.f; gbx = gdd * 2.f * (bx - px); gby = gdd * 2.f * (by - py);
    } else {
        float u = (bax * (px - ax) + bay * (py - ay)) / l2;
        u = u < 0.f ? 0.f : (u > 1.f ? 1.f : u);
        const float qx = ax + u * bax - px, qy = ay + u * bay - py;
        gax = gdd * (1.f - u) * 2.f * qx; gay = gdd * (1.f - u) * 2.f * qy;
        gbx = gdd * u * 2.f * qx; gby = gdd * u * 2.f * qy;
    }
    // edge e runs from the triangle's vertex e to vertex (e + 1) % 3
    const float q0x = e == 0 ? gax : (e == 2 ? gbx : 0.f), q0y = e == 0 ? gay : (e == 2 ? gby : 0.f);
    const float q1x = e == 1 ? gax : (e == 0 ? gbx : 0.f), q1y = e == 1 ? gay : (e == 0 ? gby : 0.f);
    const float q2x = e == 2 ? gax : (e == 1 ? gbx : 0.f), q2y = e == 2 ? gay : (e == 1 ? gby : 0.f);
    if (code <= 1) {
        c9[0] = q0x; c9[1] = q0y; c9[2] = 0.f; c9[3] = q1x; c9[4] = q1y; c9[5] = 0.f; c9[6] = q2x; c9[7] = q2y; c9[8] = 0.f;
        return;
    }
    const int k1 = (code - 2) % 3, kind = (code - 2) / 3, k2 = (k1 + 1) % 3, k3 = (k1 + 2) % 3;
    const float X1 = sel3(k1, ov[0], ov[3], ov[6]), Y1 = sel3(k1, ov[1], ov[4], ov[7]), Z1 = sel3(k1, ov[2], ov[5], ov[8]);
    const float X2 = sel3(k2, ov[0], ov[3], ov[6]), Y2 = sel3(k2, ov[1], ov[4], ov[7]), Z2 = sel3(k2, ov[2], ov[5], ov[8]);
    const float X3 = sel3(k3, ov[0], ov[3], ov[6]), Y3 = sel3(k3, ov[1], ov[4], ov[7]), Z3 = sel3(k3, ov[2], ov[5], ov[8]);
    float g1x = 0.f, g1y = 0.f, g1z = 0.f, g2x = 0.f, g2y = 0.f, g2z = 0.f, g3x = 0.f, g3y = 0.f, g3z = 0.f, dw2 = 0.f, dw3 = 0.f;
    // a gradient (gx, gy) on the cut point of the edge p1 -> (Xo, Yo, Zo) with parameter w
    auto cut = [&](float gx, float gy, float w, float Xo, float Yo, float Zo, float &gox, float &goy, float &goz, float &dw)
                   __attribute__((always_inline)) {
        if (persp) {
            g1x += gx * (1.0f - w) * Z1 / z_clip; g1z += gx * (1.0f - w) * X1 / z_clip;
            gox += gx * w * Zo / z_clip;          goz += gx * w * Xo / z_clip;
            dw += gx * (Xo * Zo - X1 * Z1) / z_clip;
            g1y += gy * (1.0f - w) * Z1 / z_clip; g1z += gy * (1.0f - w) * Y1 / z_clip;
            goy += gy * w * Zo / z_clip;          goz += gy * w * Yo / z_clip;
            dw += gy * (Yo * Zo - Y1 * Z1) / z_clip;
        } else {
            g1x += gx * (1.0f - w); gox += gx * w; dw += gx * (Xo - X1);
            g1y += gy * (1.0f - w); goy += gy * w; dw += gy * (Yo - Y1);
        }
    };
    if (kind == 0) {                // (p4, p2, p5)
        cut(q0x, q0y, cw2, X2, Y2, Z2, g2x, g2y, g2z, dw2);
        g2x += q1x; g2y += q1y;
        cut(q2x, q2y, cw3, X3, Y3, Z3, g3x, g3y, g3z, dw3);
    } else if (kind == 1) {         // (p5, p2, p3)
        cut(q0x, q0y, cw3, X3, Y3, Z3, g3x, g3y, g3z, dw3);
        g2x += q1x; g2y += q1y;
        g3x += q2x; g3y += q2y;
    } else {                        // (p1, p4, p5)
        g1x += q0x; g1y += q0y;
        cut(q1x, q1y, cw2, X2, Y2, Z2, g2x, g2y, g2z, dw2);
        cut(q2x, q2y, cw3, X3, Y3, Z3, g3x, g3y, g3z, dw3);
    }
    const float z12 = Z1 - Z2, z13 = Z1 - Z3;
    g1z += dw2 * (z_clip - Z2) / (z12 * z12) + dw3 * (z_clip - Z3) / (z13 * z13);
    g2z += dw2 * (Z1 - z_clip) / (z12 * z12);
    g3z += dw3 * (Z1 - z_clip) / (z13 * z13);
#pragma unroll
    for (int q = 0; q < 3; ++q) {   // p1 p2 p3 are the face's vertices k1 k2 k3
        c9[3 * q] = q == k1 ? g1x : (q == k2 ? g2x : g3x);
        c9[3 * q + 1] = q == k1 ? g1y : (q == k2 ? g2y : g3y);
        c9[3 * q + 2] = q == k1 ? g1z : (q == k2 ? g2z : g3z);
    }
}

struct TileList {
    float face[LIST_CAP][10];
    int fidx[LIST_CAP];
    int wcnt[4];
};

// every valid record of the view whose padded bbox touches the tile, in index order, in chunks of <= LIST_CAP: fn(i) is called
// by every lane for every entry i of the LDS list (workgroup-uniform control flow)
template <typename Fn>
__device__ __forceinline__ void sweep_tile(const float4 *__restrict__ rb, int NR, int S, float pad, TileList &L, Fn fn) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px_hi = min(blockIdx.x * TILE + TILE - 1, S - 1), py_hi = min(blockIdx.y * TILE + TILE - 1, S - 1);
    const float tx_max = pix_to_ndc(S - 1 - blockIdx.x * TILE, S), tx_min = pix_to_ndc(S - 1 - px_hi, S);
    const float ty_max = pix_to_ndc(S - 1 - blockIdx.y * TILE, S), ty_min = pix_to_ndc(S - 1 - py_hi, S);
    int count = 0;
    for (int base = 0; base < NR; base += 256) {
        const int f = base + tid;
        bool hit = false;
        float4 r0, r1, r2;
        if (f < NR) {
            r0 = rb[3 * (size_t)f]; r1 = rb[3 * (size_t)f + 1]; r2 = rb[3 * (size_t)f + 2];
            const float xmin = fminf(r0.x, fminf(r0.w, r1.z)) - pad, xmax = fmaxf(r0.x, fmaxf(r0.w, r1.z)) + pad;
            const float ymin = fminf(r0.y, fminf(r1.x, r1.w)) - pad, ymax = fmaxf(r0.y, fmaxf(r1.x, r1.w)) + pad;
            hit = (r2.y != 0.f) && !(tx_min > xmax || tx_max < xmin || ty_min > ymax || ty_max < ymin);
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) L.wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = count;
        for (int w = 0; w < wave; ++w) off += L.wcnt[w];
        const int total = L.wcnt[0] + L.wcnt[1] + L.wcnt[2] + L.wcnt[3];
        if (hit) {
            const int slot = off + __popcll(m & ((1ull << lane) - 1ull));       // < count + 256 <= LIST_CAP
            L.fidx[slot] = f;
            L.face[slot][0] = r0.x; L.face[slot][1] = r0.y; L.face[slot][2] = r0.z;
            L.face[slot][3] = r0.w; L.face[slot][4] = r1.x; L.face[slot][5] = r1.y;
            L.face[slot][6] = r1.z; L.face[slot][7] = r1.w; L.face[slot][8] = r2.x;
            L.face[slot][9] = r2.y;                     // record code (which kind of sub-triangle)
        }
        count += total;
        __syncthreads();
        if (count > LIST_CAP - 256 || base + 256 >= NR) {
            for (int i = 0; i < count; ++i) fn(i);
            count = 0;
            __syncthreads();
        }
    }
}

struct RasterArgs {
    const float4 *rec; int NR, S, K; float blur; int clip, cull, persp; float sigma;
};

// state: planes of B*S*S values -- 0 keep, 1 cut depth, 2 cut record index (int bits), 3 (LOSS) alpha - target
template <int LOSS>
__global__ __launch_bounds__(256) void silraster_fwd_kernel(const RasterArgs a, const float *__restrict__ target,
                                                            float *__restrict__ alpha, float *__restrict__ state, size_t n) {
    __shared__ TileList L;
    const int b = blockIdx.z, tid = threadIdx.x, S = a.S;
    const int px = blockIdx.x * TILE + (tid & (TILE - 1));
    const int py = blockIdx.y * TILE + (tid >> 4);
    const bool in_img = px < S && py < S;
    View v;
    v.xf = pix_to_ndc(S - 1 - px, S); v.yf = pix_to_ndc(S - 1 - py, S);
    v.pad = sqrtf(a.blur); v.blur = a.blur; v.clip = a.clip; v.cull = a.cull; v.persp = a.persp;
    const float4 *rb = a.rec + (size_t)b * a.NR * 3;

    float keep = 1.f, cz = -1.f;        // the cut: nothing taken yet (pz >= 0 always)
    int ci = -1, taken = 0;
    bool more = in_img, poison = false;
    for (;;) {
        int qi[KL]; float qz[KL], qd[KL];
#pragma unroll
        for (int k = 0; k < KL; ++k) { qi[k] = -1; qz[k] = 3.0e38f; qd[k] = 0.f; }
        sweep_tile(rb, a.NR, S, v.pad, L, [&](int i) __attribute__((always_inline)) {
            if (!more) return;
            Geo g;
            if (!sil_eval(L.face[i][0], L.face[i][1], L.face[i][2], L.face[i][3], L.face[i][4], L.face[i][5], L.face[i][6],
                          L.face[i][7], L.face[i][8], v.xf, v.yf, v.pad, v.blur, v.clip, v.cull, v.persp, g))
                return;
            if (g.pz != g.pz || g.d != g.d) { poison = true; return; }
            const int idx = L.fidx[i];
            if (!(g.pz > cz || (g.pz == cz && idx > ci))) return;       // at or before the cut: taken by an earlier pass
            if (!(g.pz < qz[KL - 1])) return;                           // not among the next 8 (ties keep the earlier record)
            const int code = (int)L.face[i][9];
            if (code >= 2 && code < 8 && sibling_wins(rb, idx, g.d, v)) return;
            // sorted insertion, fully unrolled (raster_k_kernel's): the list stays in registers
            int cf = idx; float cpz = g.pz, cd = g.inside ? -g.d : g.d;
            bool placed = false;
#pragma unroll
            for (int k = 0; k < KL; ++k) {
                if (placed || cpz < qz[k]) {
                    placed = true;
                    const int tf = qi[k]; const float tz = qz[k], td = qd[k];
                    qi[k] = cf; qz[k] = cpz; qd[k] = cd;
                    cf = tf; cpz = tz; cd = td;
                }
            }
        });
        const int want = min(KL, a.K - taken);
#pragma unroll
        for (int k = 0; k < KL; ++k) {
            if (k < want && qi[k] >= 0) {
                const float prob = 1.0f / (1.0f + expf(qd[k] / a.sigma));
                keep *= (1.0f - prob);
                cz = qz[k]; ci = qi[k]; ++taken;
            }
        }
        more = more && taken < a.K && qi[KL - 1] >= 0;
        if (!__syncthreads_or(more ? 1 : 0)) break;
    }
    if (!in_img) return;
    if (poison) keep = __int_as_float(0x7fc00000);
    const size_t p = ((size_t)b * S + py) * S + px;
    const float al = 1.0f - keep;
    state[p] = keep; state[n + p] = cz; state[2 * n + p] = __int_as_float(ci);
    if (LOSS) state[3 * n + p] = al - target[p];
    else alpha[p] = al;
}

// partials[blk] = sum diff^2 over the block's pixels: the decomposition and summation order of silhouette_loss_kernel
// (silhouette.hip), so the loss equals st3d_silhouette_loss's bit for bit when alpha does
__global__ __launch_bounds__(256) void silraster_sqsum_kernel(const float *__restrict__ diffs, size_t n, float *__restrict__ partials) {
    float acc = 0.f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float diff = diffs[i];
        acc += diff * diff;
    }
    __shared__ float s[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// DET 0: float table + float global atomics; DET 1: the bound pass (partials[block] = sum of |contributions|); DET 2: 64-bit
// fixed point with the scale derived from that bound (gndc is then the int64 accumulator array).  grad_alpha NULL: the
// upstream gradient of a pixel is grad_scale * state plane 3 (the fused loss's alpha - target).
template <int DET>
__global__ __launch_bounds__(256) void silraster_bwd_kernel(const RasterArgs a, const float *__restrict__ state, size_t n,
                                                            const float *__restrict__ grad_alpha, float grad_scale,
                                                            const float *__restrict__ ndc, const int32_t *__restrict__ faces,
                                                            int V, float z_clip, float *__restrict__ gndc,
                                                            const st3d_det::DetHeader *__restrict__ det,
                                                            float *__restrict__ partials) {
    typedef typename std::conditional<DET == 2, unsigned long long, float>::type acc_t;
    __shared__ TileList L;
    __shared__ int s_key[DET == 1 ? 1 : kFaceSlots];
    __shared__ acc_t s_acc[DET == 1 ? 1 : kFaceSlots][9];
    __shared__ float s4[4];
    const int b = blockIdx.z, tid = threadIdx.x, S = a.S;
    const int px = blockIdx.x * TILE + (tid & (TILE - 1));
    const int py = blockIdx.y * TILE + (tid >> 4);
    const bool in_img = px < S && py < S;
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    float keep = 0.f, cz = -1.f, ga = 0.f;
    int ci = -1;
    if (in_img) {
        const size_t p = ((size_t)b * S + py) * S + px;
        keep = state[p]; cz = state[n + p]; ci = __float_as_int(state[2 * n + p]);
        ga = grad_alpha ? grad_alpha[p] : grad_scale * state[3 * n + p];
    }
    // -prob * keep / sigma is 0 for every fragment of a pixel whose keep is 0 (saturated interior), ga = 0 likewise
    const bool live = in_img && !(keep == 0.f || ga == 0.f);
    if (!__syncthreads_or(live ? 1 : 0)) {
        if (DET == 1 && tid == 0) partials[blk] = 0.f;
        return;
    }
    if (DET != 1) {
        for (int e = tid; e < kFaceSlots; e += 256) s_key[e] = -1;
        for (int e = tid; e < kFaceSlots * 9; e += 256) (&s_acc[0][0])[e] = (acc_t)0;
        __syncthreads();
    }
    const double dscale = DET == 2 ? det->scale : 1.0;
    View v;
    v.xf = pix_to_ndc(S - 1 - px, S); v.yf = pix_to_ndc(S - 1 - py, S);
    v.pad = sqrtf(a.blur); v.blur = a.blur; v.clip = a.clip; v.cull = a.cull; v.persp = a.persp;
    const float4 *rb = a.rec + (size_t)b * a.NR * 3;
    const float *vb = ndc + (size_t)b * V * 3;
    float bound = 0.f;
    sweep_tile(rb, a.NR, S, v.pad, L, [&](int i) __attribute__((always_inline)) {
        if (!live) return;
        Geo g;
        if (!sil_eval(L.face[i][0], L.face[i][1], L.face[i][2], L.face[i][3], L.face[i][4], L.face[i][5], L.face[i][6],
                      L.face[i][7], L.face[i][8], v.xf, v.yf, v.pad, v.blur, v.clip, v.cull, v.persp, g))
            return;
        const int idx = L.fidx[i];
        const bool nanc = g.pz != g.pz || g.d != g.d;          // poisoned its pixel in the forward: keep is NaN
        if (!nanc && !(g.pz < cz || (g.pz == cz && idx <= ci))) return;     // beyond the cut: not a fragment
        const int code = (int)L.face[i][9];
        if (code >= 2 && code < 8 && sibling_wins(rb, idx, g.d, v)) return;
        const float sd = g.inside ? -g.d : g.d;
        const float prob = 1.0f / (1.0f + expf(sd / a.sigma));
        const float gd = ga * (-prob * keep / a.sigma);
        if (gd == 0.f) return;
        const int f = idx >> 1;
        const float t9[9] = {L.face[i][0], L.face[i][1], L.face[i][2], L.face[i][3], L.face[i][4], L.face[i][5], L.face[i][6],
                             L.face[i][7], L.face[i][8]};
        float ov[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, cw2 = 0.f, cw3 = 0.f;
        if (code > 1) {             // a clipped record: the face's own vertices and the cut parameters
            const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            ov[0] = vb[3 * i0]; ov[1] = vb[3 * i0 + 1]; ov[2] = vb[3 * i0 + 2];
            ov[3] = vb[3 * i1]; ov[4] = vb[3 * i1 + 1]; ov[5] = vb[3 * i1 + 2];
            ov[6] = vb[3 * i2]; ov[7] = vb[3 * i2 + 1]; ov[8] = vb[3 * i2 + 2];
            const float4 r2 = rb[3 * (size_t)idx + 2];
            cw2 = r2.z; cw3 = r2.w;
        }
        float c9[9];
        sil_frag_grad(t9, g.inside, gd, v.xf, v.yf, code, cw2, cw3, ov, z_clip, a.persp, c9);
        if (DET == 1) {
#pragma unroll
            for (int c = 0; c < 9; ++c) bound += fabsf(c9[c]);
            return;
        }
        int slot = (int)(((unsigned)f * 2654435761u) >> 23) & (kFaceSlots - 1);
        bool found = false;
        for (int tries = 0; tries < kProbe; ++tries) {
            const int prev = atomicCAS(&s_key[slot], -1, f);
            if (prev == -1 || prev == f) { found = true; break; }
            slot = (slot + 1) & (kFaceSlots - 1);
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const size_t o = (size_t)b * V * 3 + 3 * (size_t)faces[3 * f + c / 3] + (c % 3);
            if (DET == 2) {
                const unsigned long long q = (unsigned long long)st3d_det::det_quantise(c9[c], dscale);
                if (found) atomicAdd(reinterpret_cast<unsigned long long *>(&s_acc[slot][c]), q);
                else atomicAdd(reinterpret_cast<unsigned long long *>(gndc) + o, q);
            } else {
                if (found) atomicAdd(reinterpret_cast<float *>(&s_acc[slot][c]), c9[c]);
                else atomicAdd(gndc + o, c9[c]);
            }
        }
    });
    if (DET == 1) {
        const float t = st3d_det::det_block_sum(bound, s4);
        if (tid == 0) partials[blk] = t;
        return;
    }
    __syncthreads();
    for (int e = tid; e < kFaceSlots * 9; e += 256) {
        const int slot = e / 9, c = e - slot * 9;
        const int fk = s_key[slot];
        if (fk < 0) continue;
        const acc_t val = s_acc[slot][c];
        if (val == (acc_t)0) continue;
        const size_t o = (size_t)b * V * 3 + 3 * (size_t)faces[3 * fk + c / 3] + (c % 3);
        if (DET == 2) atomicAdd(reinterpret_cast<unsigned long long *>(gndc) + o, (unsigned long long)val);
        else atomicAdd(gndc + o, (float)val);
    }
}

}  // namespace

#define ST3D_SILRASTER_SHAPE()                                         \
    ST3D_CHECK_ARG(B > 0 && S > 0 && F > 0);                           \
    ST3D_CHECK_ARG(blur_radius >= 0.f);                                \
    ST3D_CHECK_ARG(sigma > 0.f);                                       \
    ST3D_CHECK_ARG(((uintptr_t)face_records & 15) == 0)

#define ST3D_SILRASTER_ARGS(K_)                                                                                       \
    RasterArgs a{reinterpret_cast<const float4 *>(face_records), 2 * F, S, (K_), blur_radius, clip_bary ? 1 : 0,      \
                 cull_backfaces ? 1 : 0, perspective_correct ? 1 : 0, sigma}

extern "C" int st3d_silraster_fwd(const float *face_records, int B, int F, int S, int K, float blur_radius, int clip_bary,
                                  int cull_backfaces, int perspective_correct, float sigma, float *alpha, float *state,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(face_records && alpha && state);
    ST3D_SILRASTER_SHAPE();
    ST3D_CHECK_ARG(K >= 1 && K <= KMAX);
    ST3D_SILRASTER_ARGS(K);
    const int tiles = st3d::cdiv(S, TILE);
    silraster_fwd_kernel<0><<<dim3(tiles, tiles, B), 256, 0, st3d::as_stream(stream)>>>(a, nullptr, alpha, state,
                                                                                        (size_t)B * S * S);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_silraster_loss(const float *face_records, int B, int F, int S, int K, float blur_radius, int clip_bary,
                                   int cull_backfaces, int perspective_correct, float sigma, const float *target, float scale,
                                   float *state, float *partials, float *loss_out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(face_records && target && state && partials && loss_out);
    ST3D_SILRASTER_SHAPE();
    ST3D_CHECK_ARG(K >= 1 && K <= KMAX);
    ST3D_SILRASTER_ARGS(K);
    hipStream_t s = st3d::as_stream(stream);
    const size_t n = (size_t)B * S * S;
    const int tiles = st3d::cdiv(S, TILE);
    silraster_fwd_kernel<1><<<dim3(tiles, tiles, B), 256, 0, s>>>(a, target, nullptr, state, n);
    ST3D_LAUNCH_CHECK();
    const size_t blocks = (n + 255) / 256;
    const int np = st3d_reduce_partials();
    const int grid = (int)(blocks > (size_t)np ? (size_t)np : blocks);
    silraster_sqsum_kernel<<<grid, 256, 0, s>>>(state + 3 * n, n, partials);
    ST3D_LAUNCH_CHECK();
    return st3d::finish_partials(partials, grid, scale, loss_out, s);
}

extern "C" size_t st3d_silraster_bwd_workspace_bytes(int B, int V, int S) {
    const size_t tiles = (size_t)((S + TILE - 1) / TILE);
    return st3d_det::workspace_bytes((size_t)B * V * 3, tiles * tiles * B);
}

extern "C" int st3d_silraster_bwd(const float *face_records, const float *verts_ndc, const int32_t *faces, int B, int V, int F,
                                  int S, float blur_radius, int clip_bary, int cull_backfaces, int perspective_correct,
                                  float z_clip, float sigma, const float *state, const float *grad_alpha, float grad_scale,
                                  float *grad_verts_ndc, void *workspace, size_t workspace_bytes, st3d_stream_t stream) {
    ST3D_CHECK_ARG(face_records && verts_ndc && faces && state && grad_verts_ndc);
    ST3D_SILRASTER_SHAPE();
    ST3D_CHECK_ARG(V > 0 && z_clip > 0.f);
    ST3D_SILRASTER_ARGS(KMAX);
    hipStream_t s = st3d::as_stream(stream);
    const size_t n = (size_t)B * S * S, nacc = (size_t)B * V * 3;
    const int tiles = st3d::cdiv(S, TILE);
    const dim3 grid(tiles, tiles, B);
    if (!workspace) {
        ST3D_HIP(hipMemsetAsync(grad_verts_ndc, 0, nacc * sizeof(float), s));
        silraster_bwd_kernel<0><<<grid, 256, 0, s>>>(a, state, n, grad_alpha, grad_scale, verts_ndc, faces, V, z_clip,
                                                     grad_verts_ndc, nullptr, nullptr);
        ST3D_LAUNCH_CHECK();
        return ST3D_OK;
    }
    ST3D_CHECK_ARG(workspace_bytes >= st3d_silraster_bwd_workspace_bytes(B, V, S) && ((uintptr_t)workspace & 15) == 0);
    const size_t np = (size_t)tiles * tiles * B;
    const st3d_det::DetRun det(workspace, np, nacc);
    silraster_bwd_kernel<1><<<grid, 256, 0, s>>>(a, state, n, grad_alpha, grad_scale, verts_ndc, faces, V, z_clip, nullptr, nullptr,
                                                 det.partials);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    silraster_bwd_kernel<2><<<grid, 256, 0, s>>>(a, state, n, grad_alpha, grad_scale, verts_ndc, faces, V, z_clip,
                                                 reinterpret_cast<float *>(det.acc), det.hdr, nullptr);
    ST3D_LAUNCH_CHECK();
    return det.convert(0, grad_verts_ndc, s);
}
