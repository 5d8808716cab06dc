// mesh.hip -- view-independent mesh regularisers of optimization_target 'mesh'/'both'
// (reference losses.py:84-87,93-96,112-115,121-124: F.mse_loss(verts, target_verts) +
// pytorch3d.loss mesh_edge_loss + mesh_laplacian_smoothing('uniform') + mesh_normal_consistency),
// forward and gradient for ONE mesh (kernel K15).  Topology is static: the host
// builds the unique edge list, the CSR vertex adjacency and the list of face pairs once.
// O(V + E + P) work, a few tens of KB: latency-bound; losses are reduced in fixed order
// (per-workgroup partials, then one workgroup) so they are bitwise reproducible; so are the
// gradients: every term's gradient is a per-vertex GATHER over static CSR lists in a fixed order
// (round 3: the edge term walks the vertex adjacency, the normal term the vertex -> (pair, role)
// list over per-pair gradients staged in scratch) -- no float atomics anywhere.
#include "common.h"

namespace {

constexpr int NPART = 1024;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ void block_partial(float v, float *partials) {
    __shared__ float s[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float *p, int i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ void st3(float *p, int i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

// mse(verts, target): mean over V*3; grad = 2 w (v - t) / (3V)
__global__ __launch_bounds__(256) void verts_mse_kernel(const float *__restrict__ v, const float *__restrict__ t, int n,
                                                        float gcoef, float *__restrict__ g, float *__restrict__ partials) {
    float acc = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float d = v[i] - t[i];
        acc += d * d;
        if (gcoef != 0.f) g[i] += gcoef * d;     // one thread per element: no race
    }
    block_partial(acc, partials);
}

// mean over edges of |v0 - v1|^2 (target length 0)
__global__ __launch_bounds__(256) void edge_kernel(const float *__restrict__ v, const int32_t *__restrict__ edges, int E,
                                                   float *__restrict__ partials) {
    float acc = 0.f;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const int a = edges[2 * e], b = edges[2 * e + 1];
        const V3 d = sub(ld3(v, a), ld3(v, b));
        acc += dot(d, d);
    }
    block_partial(acc, partials);
}

// edge gradient as a gather: every unique edge (a, b) is listed once in a's and once in b's adjacency row, and
// d|a-b|^2/da = 2 (a - b), so grad_k += gcoef * sum_{j in N(k)} (v_k - v_j) in the row's (ascending j) order
__global__ __launch_bounds__(256) void edge_bwd_kernel(const float *__restrict__ v, const int32_t *__restrict__ off,
                                                       const int32_t *__restrict__ nbr, int V, float gcoef,
                                                       float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    const V3 vk = ld3(v, k);
    V3 s = {0.f, 0.f, 0.f};
    for (int q = off[k]; q < off[k + 1]; ++q) s = add(s, sub(vk, ld3(v, nbr[q])));
    g[3 * k] += gcoef * s.x; g[3 * k + 1] += gcoef * s.y; g[3 * k + 2] += gcoef * s.z;
}

// y_i = mean_{j in N(i)} v_j - v_i ; loss += |y_i| ; u_i = y_i / |y_i| (0 at |y_i| = 0)
__global__ __launch_bounds__(256) void laplacian_fwd_kernel(const float *__restrict__ v, const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ nbr, int V, float *__restrict__ u,
                                                            float *__restrict__ partials) {
    float acc = 0.f;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x) {
        const int b = off[i], e = off[i + 1];
        V3 y = {0.f, 0.f, 0.f};
        if (e > b) {
            V3 s = {0.f, 0.f, 0.f};
            for (int k = b; k < e; ++k) s = add(s, ld3(v, nbr[k]));
            y = sub(mul(s, 1.0f / (float)(e - b)), ld3(v, i));
        }
        const float n = sqrtf(dot(y, y));
        acc += n;
        const V3 ui = n > 0.f ? mul(y, 1.0f / n) : V3{0.f, 0.f, 0.f};
        u[3 * i] = ui.x; u[3 * i + 1] = ui.y; u[3 * i + 2] = ui.z;
    }
    block_partial(acc, partials);
}

// grad_k += c * ( sum_{i in N(k)} u_i / deg_i - u_k )      (adjacency is symmetric)
__global__ __launch_bounds__(256) void laplacian_bwd_kernel(const float *__restrict__ u, const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ nbr, int V, float c,
                                                            float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    V3 s = {0.f, 0.f, 0.f};
    for (int q = off[k]; q < off[k + 1]; ++q) {
        const int i = nbr[q];
        const int deg = off[i + 1] - off[i];
        s = add(s, mul(ld3(u, i), 1.0f / (float)deg));
    }
    if (off[k + 1] > off[k]) s = sub(s, ld3(u, k));
    g[3 * k] += c * s.x; g[3 * k + 1] += c * s.y; g[3 * k + 2] += c * s.z;
}

// pairs (v0, v1, a, b): n0 = (v1-v0) x (a-v0), n1 = -(v1-v0) x (b-v0); loss = 1 - cos(n0, n1)
__global__ __launch_bounds__(256) void normal_kernel(const float *__restrict__ v, const int32_t *__restrict__ pairs, int P,
                                                     float gcoef, float *__restrict__ pg, float *__restrict__ partials) {
    float acc = 0.f;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
        const int i0 = pairs[4 * p], i1 = pairs[4 * p + 1], ia = pairs[4 * p + 2], ib = pairs[4 * p + 3];
        const V3 v0 = ld3(v, i0);
        const V3 e = sub(ld3(v, i1), v0), pa = sub(ld3(v, ia), v0), pb = sub(ld3(v, ib), v0);
        const V3 n0 = cross(e, pa), n1 = mul(cross(e, pb), -1.0f);
        const float eps = 1e-8f;
        const float l0 = fmaxf(sqrtf(dot(n0, n0)), eps), l1 = fmaxf(sqrtf(dot(n1, n1)), eps);
        const float c = dot(n0, n1) / (l0 * l1);
        acc += 1.0f - c;
        if (gcoef != 0.f) {
            // d(1-c)/dn0 = -(n1/(l0 l1) - c n0/l0^2), same for n1
            const V3 g0 = mul(sub(mul(n1, 1.0f / (l0 * l1)), mul(n0, c / (l0 * l0))), -gcoef);
            const V3 g1 = mul(sub(mul(n0, 1.0f / (l0 * l1)), mul(n1, c / (l1 * l1))), -gcoef);
            // n0 = e x pa: de = pa x g0, dpa = g0 x e ; n1 = -(e x pb): de -= pb x g1, dpb = -(g1 x e)
            const V3 de = sub(cross(pa, g0), cross(pb, g1));
            const V3 dpa = cross(g0, e);
            const V3 dpb = mul(cross(g1, e), -1.0f);
            // staged per (pair, role) -- role = column of the pair row (v0, v1, a, b); normal_gather_kernel sums them per vertex
            st3(pg, 4 * p + 0, mul(add(add(de, dpa), dpb), -1.0f));
            st3(pg, 4 * p + 1, de);
            st3(pg, 4 * p + 2, dpa);
            st3(pg, 4 * p + 3, dpb);
        }
    }
    block_partial(acc, partials);
}

// grad_k += sum over the (pair, role) entries of vertex k, in list order (static, built by the host: ascending pair * 4 + role)
__global__ __launch_bounds__(256) void normal_gather_kernel(const float *__restrict__ pg, const int32_t *__restrict__ off,
                                                            const int32_t *__restrict__ ref, int V, float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    V3 s = {0.f, 0.f, 0.f};
    for (int q = off[k]; q < off[k + 1]; ++q) s = add(s, ld3(pg, ref[q]));
    g[3 * k] += s.x; g[3 * k + 1] += s.y; g[3 * k + 2] += s.z;
}

// loss_out = {sum_k w_k * term_k, mse, edge, laplacian, normal}
__global__ __launch_bounds__(256) void mesh_finish_kernel(const float *__restrict__ partials, int n0, int n1, int n2, int n3,
                                                          float s0, float s1, float s2, float s3, float w0, float w1,
                                                          float w2, float w3, float *__restrict__ out) {
    __shared__ double red[256];
    const int cnt[4] = {n0, n1, n2, n3};
    const float sc[4] = {s0, s1, s2, s3};
    const float w[4] = {w0, w1, w2, w3};
    double total = 0.0;
    for (int k = 0; k < 4; ++k) {
        double a = 0.0;
        for (int i = threadIdx.x; i < cnt[k]; i += 256) a += (double)partials[k * NPART + i];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        const double term = red[0] * (double)sc[k];
        if (threadIdx.x == 0) out[1 + k] = (float)term;
        total += (double)w[k] * term;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

inline int grid_for(int n) {
    int b = (n + 255) / 256;
    return b < 1 ? 1 : (b > NPART ? NPART : b);
}

}  // namespace

extern "C" size_t st3d_mesh_reg_scratch_floats(int V, int P) { return (size_t)3 * V + (size_t)12 * P; }

extern "C" int st3d_mesh_reg(const float *verts, const float *target_verts, int V, const int32_t *edges, int E,
                             const int32_t *nbr_off, const int32_t *nbr_idx, const int32_t *pairs, int P,
                             const int32_t *pair_off, const int32_t *pair_ref,
                             const float *weights, float *scratch, float *partials, float *loss_out, float *grad_verts,
                             st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && target_verts && edges && nbr_off && nbr_idx && weights && scratch && partials && loss_out);
    ST3D_CHECK_ARG(V > 0 && E > 0 && P >= 0 && (P == 0 || (pairs && pair_off && pair_ref)));
    hipStream_t s = st3d::as_stream(stream);
    const float wv = weights[0], we = weights[1], wl = weights[2], wn = weights[3];
    const bool wg = grad_verts != nullptr;
    const int g0 = grid_for(3 * V), g1 = grid_for(E), g2 = grid_for(V), g3 = P > 0 ? grid_for(P) : 0;
    verts_mse_kernel<<<g0, 256, 0, s>>>(verts, target_verts, 3 * V, wg ? 2.0f * wv / (3.0f * V) : 0.f, grad_verts, partials);
    ST3D_LAUNCH_CHECK();
    edge_kernel<<<g1, 256, 0, s>>>(verts, edges, E, partials + NPART);
    ST3D_LAUNCH_CHECK();
    if (wg && we != 0.f) {
        edge_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(verts, nbr_off, nbr_idx, V, 2.0f * we / (float)E, grad_verts);
        ST3D_LAUNCH_CHECK();
    }
    laplacian_fwd_kernel<<<g2, 256, 0, s>>>(verts, nbr_off, nbr_idx, V, scratch, partials + 2 * NPART);
    ST3D_LAUNCH_CHECK();
    if (wg && wl != 0.f) {
        laplacian_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(scratch, nbr_off, nbr_idx, V, wl / (float)V, grad_verts);
        ST3D_LAUNCH_CHECK();
    }
    if (P > 0) {
        float *pg = scratch + (size_t)3 * V;        // (P, 4, 3) per-pair gradients
        const bool ng = wg && wn != 0.f;
        normal_kernel<<<g3, 256, 0, s>>>(verts, pairs, P, ng ? wn / (float)P : 0.f, pg, partials + 3 * NPART);
        ST3D_LAUNCH_CHECK();
        if (ng) {
            normal_gather_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(pg, pair_off, pair_ref, V, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    }
    mesh_finish_kernel<<<1, 256, 0, s>>>(partials, g0, g1, g2, g3, 1.0f / (3.0f * V), 1.0f / (float)E, 1.0f / (float)V,
                                        P > 0 ? 1.0f / (float)P : 0.f, wv, we, wl, wn, loss_out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// st3d_mesh_reg_ex: the same four terms with PyTorch3D's cotangent Laplacian ('cot' / 'cotcurv') and an edge target
// length t > 0.  At method 0 / t = 0 every launch above is issued unchanged.  The cotangent weights are
// constants of the backward; they change with the vertices, so every call rebuilds them:
//   cot_face_kernel    per face: the three cotangents and the clamped area
//   cot_vertex_kernel  per vertex i: every adjacency slot's weight L_ij (its edge's incident (face, corner) entries summed
//                      in list order -- both ends of an edge walk the same list, so L is symmetric to the bit), Lsum_i,
//                      sum_j L_ij v_j, Asum_i over the vertex's faces, the residual, |r_i| and what the gradient gathers
//   cot_bwd_kernel     per vertex k: sum_i L_ki q_i - s_k over its adjacency row
// All sums are gathers over static host-built lists in list order: no float atomics, two runs are bit-equal.  The new
// kernels compute in fp64 from the fp32 vertices and keep their intermediates in fp64 (a few hundred KB at most, the
// work is latency-bound): each output is rounded to fp32 once, so the result does not depend on how well conditioned
// Heron's formula or B^2 + C^2 - A^2 is on a needle triangle.
namespace {

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ldd(const float *p, int i) { return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]}; }
__device__ __forceinline__ D3 ldd(const double *p, int i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 mul(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ void std3(double *p, int i, D3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

__device__ __forceinline__ void block_partial_d(double v, double *partials) {
    __shared__ double s[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// fc[4 f + c] = cot of corner c, fc[4 f + 3] = area.  area^2 = s(s-A)(s-B)(s-C) = |(v1-v0) x (v2-v0)|^2 / 4 inside the same
// 1e-12 clamp, and B^2 + C^2 - A^2 = 2 (v1-v0).(v2-v0), so cot_0 = (v1-v0).(v2-v0) / (2 area), likewise at v1 and v2.
// A NaN passes the clamp (nothing is clamped away).
__global__ __launch_bounds__(256) void cot_face_kernel(const float *__restrict__ v, const int32_t *__restrict__ faces, int F,
                                                       double *__restrict__ fc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const D3 p0 = ldd(v, faces[3 * f]), p1 = ldd(v, faces[3 * f + 1]), p2 = ldd(v, faces[3 * f + 2]);
    const D3 e01 = sub(p1, p0), e02 = sub(p2, p0), e12 = sub(p2, p1);
    const D3 n = cross(e01, e02);
    const double a2 = 0.25 * dot(n, n);
    const double area = sqrt(a2 <= 1e-12 ? 1e-12 : a2);
    const double h = 0.5 / area;
    fc[4 * f] = dot(e01, e02) * h;
    fc[4 * f + 1] = -dot(e01, e12) * h;
    fc[4 * f + 2] = dot(e02, e12) * h;
    fc[4 * f + 3] = area;
}

// method 1 (cot):     r_i = (sum_j L_ij v_j) nw_i - v_i,  nw_i = 1 / Lsum_i where Lsum_i > 0, else Lsum_i itself;
//                     q_i = nw_i u_i, s_i = u_i
// method 2 (cotcurv): r_i = (sum_j L_ij v_j - Lsum_i v_i) c_i,  c_i = 0.25 / Asum_i (0 where Asum_i is not > 0);
//                     q_i = c_i u_i, s_i = Lsum_i c_i u_i
// u_i = r_i / |r_i| (0 at |r_i| = 0).  edge_ref / inc_ref entries are face * 3 + corner.
__global__ __launch_bounds__(256) void cot_vertex_kernel(const float *__restrict__ v, const int32_t *__restrict__ off,
                                                         const int32_t *__restrict__ nbr, const int32_t *__restrict__ nbr_edge,
                                                         const int32_t *__restrict__ edge_off, const int32_t *__restrict__ edge_ref,
                                                         const int32_t *__restrict__ inc_off, const int32_t *__restrict__ inc_ref,
                                                         const double *__restrict__ fc, int V, int method,
                                                         double *__restrict__ wslot, double *__restrict__ q, double *__restrict__ sv,
                                                         double *__restrict__ partials) {
    double acc = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x) {
        const D3 vi = ldd(v, i);
        double lsum = 0.0;
        D3 d = {0.0, 0.0, 0.0};          // sum_j L_ij (v_j - v_i): a neighbour AT v_i contributes exactly 0, whatever its weight
        for (int k = off[i]; k < off[i + 1]; ++k) {
            const int e = nbr_edge[k];
            double w = 0.0;
            for (int r = edge_off[e]; r < edge_off[e + 1]; ++r) {
                const int ref = edge_ref[r];
                w += fc[ref + ref / 3];          // 4 * face + corner
            }
            wslot[k] = w;
            lsum += w;
            d = add(d, mul(sub(ldd(v, nbr[k]), vi), w));
        }
        D3 r;
        double cq, cs;
        if (method == 1) {
            // (sum_j L_ij v_j) / Lsum_i - v_i = d / Lsum_i where Lsum_i > 0; else nw_i = Lsum_i and sum_j L_ij v_j = d + Lsum_i v_i
            const double nw = lsum > 0.0 ? 1.0 / lsum : lsum;
            r = lsum > 0.0 ? mul(d, nw) : sub(mul(add(d, mul(vi, lsum)), nw), vi);
            cq = nw;
            cs = 1.0;
        } else {
            double asum = 0.0;
            for (int k = inc_off[i]; k < inc_off[i + 1]; ++k) asum += fc[4 * (inc_ref[k] / 3) + 3];
            const double c = asum > 0.0 ? 0.25 / asum : 0.0;
            r = mul(d, c);
            cq = c;
            cs = lsum * c;
        }
        const double n = sqrt(dot(r, r));
        acc += n;
        const D3 u = n == 0.0 ? D3{0.0, 0.0, 0.0} : mul(r, 1.0 / n);
        std3(q, i, mul(u, cq));
        std3(sv, i, mul(u, cs));
    }
    block_partial_d(acc, partials);
}

// grad_k += c ( sum_i L_ki q_i - s_k ), L_ki = the slot's weight (L is symmetric)
__global__ __launch_bounds__(256) void cot_bwd_kernel(const double *__restrict__ q, const double *__restrict__ sv,
                                                      const int32_t *__restrict__ off, const int32_t *__restrict__ nbr,
                                                      const double *__restrict__ wslot, int V, double c, float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    D3 s = {0.0, 0.0, 0.0};
    for (int t = off[k]; t < off[k + 1]; ++t) s = add(s, mul(ldd(q, nbr[t]), wslot[t]));
    s = mul(sub(s, ldd(sv, k)), c);
    g[3 * k] += (float)s.x; g[3 * k + 1] += (float)s.y; g[3 * k + 2] += (float)s.z;
}

// mean over edges of (|a - b| - t)^2
__global__ __launch_bounds__(256) void edge_target_kernel(const float *__restrict__ v, const int32_t *__restrict__ edges, int E,
                                                          double t, double *__restrict__ partials) {
    double acc = 0.0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const D3 d = sub(ldd(v, edges[2 * e]), ldd(v, edges[2 * e + 1]));
        const double x = sqrt(dot(d, d)) - t;
        acc += x * x;
    }
    block_partial_d(acc, partials);
}

// d(l - t)^2/da = 2 (l - t)(a - b)/l, the direction 0 at l = 0; a gather over the adjacency row like edge_bwd_kernel
__global__ __launch_bounds__(256) void edge_target_bwd_kernel(const float *__restrict__ v, const int32_t *__restrict__ off,
                                                              const int32_t *__restrict__ nbr, int V, double t, double gcoef,
                                                              float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    const D3 vk = ldd(v, k);
    D3 s = {0.0, 0.0, 0.0};
    for (int j = off[k]; j < off[k + 1]; ++j) {
        const D3 d = sub(vk, ldd(v, nbr[j]));
        const double l = sqrt(dot(d, d));
        if (l != 0.0) s = add(s, mul(d, (l - t) / l));
    }
    g[3 * k] += (float)(gcoef * s.x); g[3 * k + 1] += (float)(gcoef * s.y); g[3 * k + 2] += (float)(gcoef * s.z);
}

// mesh_finish_kernel with the edge (bit 1 of dmask) and / or Laplacian (bit 2) partials in fp64: dparts[(k - 1) * NPART + i]
__global__ __launch_bounds__(256) void mesh_finish_ex_kernel(const float *__restrict__ partials, const double *__restrict__ dparts,
                                                             int dmask, int n0, int n1, int n2, int n3, float s0, float s1,
                                                             float s2, float s3, int E, int V, float w0, float w1, float w2,
                                                             float w3, float *__restrict__ out) {
    __shared__ double red[256];
    const int cnt[4] = {n0, n1, n2, n3};
    const float sc[4] = {s0, s1, s2, s3};
    const int div[4] = {1, E, V, 1};
    const float w[4] = {w0, w1, w2, w3};
    double total = 0.0;
    for (int k = 0; k < 4; ++k) {
        const bool dbl = (dmask >> k) & 1;
        double a = 0.0;
        for (int i = threadIdx.x; i < cnt[k]; i += 256) a += dbl ? dparts[(k - 1) * NPART + i] : (double)partials[k * NPART + i];
        red[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        const double term = dbl ? red[0] / (double)div[k] : red[0] * (double)sc[k];      // an fp64 term is rounded once, at the store
        if (threadIdx.x == 0) out[1 + k] = (float)term;
        total += (double)w[k] * term;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)total;
}

inline size_t even_up(size_t n) { return (n + 1) & ~(size_t)1; }

}  // namespace

extern "C" size_t st3d_mesh_reg_ex_scratch_floats(int V, int E, int F, int P) {
    if (V <= 0 || E <= 0 || F < 0 || P < 0) return 0;
    const size_t doubles = (size_t)2 * NPART + (size_t)4 * F + (size_t)2 * E + (size_t)6 * V;
    return even_up(st3d_mesh_reg_scratch_floats(V, P)) + 2 * doubles;
}

extern "C" int st3d_mesh_reg_ex(const float *verts, const float *target_verts, int V, const int32_t *edges, int E,
                                const int32_t *nbr_off, const int32_t *nbr_idx, const int32_t *pairs, int P,
                                const int32_t *pair_off, const int32_t *pair_ref, const int32_t *faces, int F,
                                const int32_t *nbr_edge, const int32_t *edge_off, const int32_t *edge_ref,
                                const int32_t *inc_off, const int32_t *inc_ref, int laplacian_method, float edge_target_length,
                                const float *weights, float *scratch, float *partials, float *loss_out, float *grad_verts,
                                st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && target_verts && edges && nbr_off && nbr_idx && weights && scratch && partials && loss_out);
    ST3D_CHECK_ARG(V > 0 && E > 0 && P >= 0 && (P == 0 || (pairs && pair_off && pair_ref)));
    ST3D_CHECK_ARG(laplacian_method >= 0 && laplacian_method <= 2);
    ST3D_CHECK_ARG(edge_target_length >= 0.f && edge_target_length <= 3.0e38f);      // finite; a NaN fails the first
    ST3D_CHECK_ARG(laplacian_method == 0 || (faces && F > 0 && nbr_edge && edge_off && edge_ref && inc_off && inc_ref));
    ST3D_CHECK_ARG(((uintptr_t)scratch & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const float wv = weights[0], we = weights[1], wl = weights[2], wn = weights[3];
    const bool wg = grad_verts != nullptr;
    const bool cot = laplacian_method != 0, tgt = edge_target_length != 0.f;
    const int g0 = grid_for(3 * V), g1 = grid_for(E), g2 = grid_for(V), g3 = P > 0 ? grid_for(P) : 0;
    double *dparts = reinterpret_cast<double *>(scratch + even_up(st3d_mesh_reg_scratch_floats(V, P)));
    double *fc = dparts + 2 * NPART, *wslot = fc + (size_t)4 * (cot ? F : 0), *q = wslot + (size_t)2 * E, *sv = q + (size_t)3 * V;
    verts_mse_kernel<<<g0, 256, 0, s>>>(verts, target_verts, 3 * V, wg ? 2.0f * wv / (3.0f * V) : 0.f, grad_verts, partials);
    ST3D_LAUNCH_CHECK();
    if (!tgt) {
        edge_kernel<<<g1, 256, 0, s>>>(verts, edges, E, partials + NPART);
        ST3D_LAUNCH_CHECK();
        if (wg && we != 0.f) {
            edge_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(verts, nbr_off, nbr_idx, V, 2.0f * we / (float)E, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    } else {
        edge_target_kernel<<<g1, 256, 0, s>>>(verts, edges, E, (double)edge_target_length, dparts);
        ST3D_LAUNCH_CHECK();
        if (wg && we != 0.f) {
            edge_target_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(verts, nbr_off, nbr_idx, V, (double)edge_target_length,
                                                                      2.0 * (double)we / (double)E, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    }
    if (!cot) {
        laplacian_fwd_kernel<<<g2, 256, 0, s>>>(verts, nbr_off, nbr_idx, V, scratch, partials + 2 * NPART);
        ST3D_LAUNCH_CHECK();
        if (wg && wl != 0.f) {
            laplacian_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(scratch, nbr_off, nbr_idx, V, wl / (float)V, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    } else {
        cot_face_kernel<<<st3d::cdiv(F, 256), 256, 0, s>>>(verts, faces, F, fc);
        ST3D_LAUNCH_CHECK();
        cot_vertex_kernel<<<g2, 256, 0, s>>>(verts, nbr_off, nbr_idx, nbr_edge, edge_off, edge_ref, inc_off, inc_ref, fc, V,
                                            laplacian_method, wslot, q, sv, dparts + NPART);
        ST3D_LAUNCH_CHECK();
        if (wg && wl != 0.f) {
            cot_bwd_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(q, sv, nbr_off, nbr_idx, wslot, V, (double)wl / (double)V, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    }
    if (P > 0) {
        float *pg = scratch + (size_t)3 * V;        // (P, 4, 3) per-pair gradients
        const bool ng = wg && wn != 0.f;
        normal_kernel<<<g3, 256, 0, s>>>(verts, pairs, P, ng ? wn / (float)P : 0.f, pg, partials + 3 * NPART);
        ST3D_LAUNCH_CHECK();
        if (ng) {
            normal_gather_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(pg, pair_off, pair_ref, V, grad_verts);
            ST3D_LAUNCH_CHECK();
        }
    }
    const float s0 = 1.0f / (3.0f * V), s1 = 1.0f / (float)E, s2 = 1.0f / (float)V, s3 = P > 0 ? 1.0f / (float)P : 0.f;
    if (!cot && !tgt)
        mesh_finish_kernel<<<1, 256, 0, s>>>(partials, g0, g1, g2, g3, s0, s1, s2, s3, wv, we, wl, wn, loss_out);
    else
        mesh_finish_ex_kernel<<<1, 256, 0, s>>>(partials, dparts, (tgt ? 2 : 0) | (cot ? 4 : 0), g0, g1, g2, g3, s0, s1, s2, s3,
                                               E, V, wv, we, wl, wn, loss_out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
