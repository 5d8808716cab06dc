// lighting.hip -- the mesh-side half of Phong lighting (the per-fragment half is phong.h, inside the shade kernels):
//   * vertex normals of PyTorch3D's Meshes.verts_normals_packed, forward and backward: per face c_f = (v2 - v1) x (v0 - v1)
//     (area-weighted, unnormalised), m_v = sum of c_f over the faces of v, n_v = m_v / max(|m_v|, 1e-6);
//   * the world-space gradient scatter of the lit backward: every fragment's d/dN and d/dP (written by the shade backward)
//     goes to its face's corners with weights b_i (N = sum b_i n_i, P = sum b_i v_i).
// Vertex sums are GATHERS over a static vertex -> (face, corner) incidence list (CSR, ascending face * 3 + corner, built
// once per topology by the host) in a fixed order: no float atomics, bitwise reproducible -- the pattern of
// normal_kernel / normal_gather_kernel in mesh.hip.  The fragment scatter bins per face in LDS per 16x16 tile as
// raster_k_bwd_kernel does; DET 2 accumulates in 64-bit fixed point (det.h) after a DET 1 bound pass.
// O(V + F) and O(fragments) work on tens of KB: latency-bound, one small kernel per job.
#include <type_traits>

#include "common.h"
#include "det.h"

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float *p, int i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ void st3(float *p, int i, V3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }

constexpr float kNormEps = 1e-6f;

// stage[f] = (v2 - v1) x (v0 - v1)
__global__ __launch_bounds__(256) void face_normal_kernel(const float *__restrict__ v, const int32_t *__restrict__ faces, int F,
                                                          float *__restrict__ stage) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const V3 p0 = ld3(v, faces[3 * f]), p1 = ld3(v, faces[3 * f + 1]), p2 = ld3(v, faces[3 * f + 2]);
    st3(stage, f, cross(sub(p2, p1), sub(p0, p1)));
}

// m_k = sum over the (face, corner) entries of vertex k in list order; n_k = m_k / max(|m_k|, eps)
__global__ __launch_bounds__(256) void vertex_normal_gather_kernel(const float *__restrict__ stage, const int32_t *__restrict__ off,
                                                                   const int32_t *__restrict__ ref, int V, float *__restrict__ n,
                                                                   float *__restrict__ m) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    V3 s = {0.f, 0.f, 0.f};
    for (int q = off[k]; q < off[k + 1]; ++q) s = add(s, ld3(stage, ref[q] / 3));
    st3(m, k, s);
    st3(n, k, mul(s, 1.0f / __builtin_elementwise_maximum(sqrtf(dot(s, s)), kNormEps)));
}

// d/dm of n = m / max(|m|, eps)
__device__ __forceinline__ V3 normalize_bwd(V3 m, V3 g) {
    const float len = sqrtf(dot(m, m));
    if (!(len > kNormEps)) return mul(g, 1.0f / kNormEps);
    const V3 nh = mul(m, 1.0f / len);
    return mul(sub(g, mul(nh, dot(nh, g))), 1.0f / len);
}

// per face: g_c = sum over its corners of d/dm; c = a x b with a = v2 - v1, b = v0 - v1:
//   d/dv2 = b x g_c, d/dv0 = g_c x a, d/dv1 = -(both); staged per (face, corner)
__global__ __launch_bounds__(256) void face_normal_bwd_kernel(const float *__restrict__ v, const int32_t *__restrict__ faces, int F,
                                                              const float *__restrict__ m, const float *__restrict__ gn,
                                                              float *__restrict__ stage) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const V3 gc = add(add(normalize_bwd(ld3(m, i0), ld3(gn, i0)), normalize_bwd(ld3(m, i1), ld3(gn, i1))),
                      normalize_bwd(ld3(m, i2), ld3(gn, i2)));
    const V3 p0 = ld3(v, i0), p1 = ld3(v, i1), p2 = ld3(v, i2);
    const V3 d2 = cross(sub(p0, p1), gc), d0 = cross(gc, sub(p2, p1));
    st3(stage, 3 * f + 0, d0);
    st3(stage, 3 * f + 1, sub(mul(d2, -1.0f), d0));
    st3(stage, 3 * f + 2, d2);
}

// g_k += (gpos_k) + sum over the (face, corner) entries of vertex k in list order
__global__ __launch_bounds__(256) void vertex_normal_bwd_gather_kernel(const float *__restrict__ stage, const int32_t *__restrict__ off,
                                                                       const int32_t *__restrict__ ref, int V,
                                                                       const float *__restrict__ gpos, float *__restrict__ g) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    V3 s = gpos ? ld3(gpos, k) : V3{0.f, 0.f, 0.f};
    for (int q = off[k]; q < off[k + 1]; ++q) s = add(s, ld3(stage, ref[q]));
    g[3 * k] += s.x; g[3 * k + 1] += s.y; g[3 * k + 2] += s.z;
}

// ---- fragment scatter: grad_np (per fragment d/dN, d/dP) -> out (2,V,3) = [d/d(vertex positions), d/d(vertex normals)]
constexpr int kFaceSlots = 256, kProbe = 24;

template <int DET>
__global__ __launch_bounds__(256) void phong_scatter_kernel(const float *__restrict__ gnp, const int32_t *__restrict__ p2f,
                                                            const float *__restrict__ bary, const int32_t *__restrict__ faces,
                                                            int V, int S, int K, int tiles_x, float *__restrict__ out,
                                                            const st3d_det::DetHeader *__restrict__ det,
                                                            float *__restrict__ partials) {
    typedef typename std::conditional<DET == 2, unsigned long long, float>::type acc_t;
    __shared__ int s_key[kFaceSlots];
    __shared__ acc_t s_acc[DET == 1 ? 1 : kFaceSlots][18];
    __shared__ float s4[4];
    const int tid = threadIdx.x;
    if (DET != 1) {
        for (int e = tid; e < kFaceSlots; e += 256) s_key[e] = -1;
        for (int e = tid; e < kFaceSlots * 18; e += 256) (&s_acc[0][0])[e] = (acc_t)0;
        __syncthreads();
    }
    const double dscale = DET == 2 ? det->scale : 1.0;
    const size_t HW = (size_t)S * S;
    const int b = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int yi = ty * 16 + (tid >> 4), xi = tx * 16 + (tid & 15);
    float bound = 0.f;
    if (yi < S && xi < S) {
        const size_t pix = (size_t)b * HW + (size_t)yi * S + xi;
        for (int k = 0; k < K; ++k) {
            const size_t i = pix * K + k;
            const int f = p2f[i];
            if (f < 0) continue;
            const float bw[3] = {bary[3 * i], bary[3 * i + 1], bary[3 * i + 2]};
            const float *g = gnp + 6 * i;
            float c18[18];       // corner j: [d/dP * b_j (3), d/dN * b_j (3)]
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { c18[6 * j + c] = g[3 + c] * bw[j]; c18[6 * j + 3 + c] = g[c] * bw[j]; }
            }
            if (DET == 1) {
#pragma unroll
                for (int c = 0; c < 18; ++c) bound += fabsf(c18[c]);
                continue;
            }
            int slot = (int)(((unsigned)f * 2654435761u) >> 24) & (kFaceSlots - 1);
            bool found = false;
            for (int tries = 0; tries < kProbe; ++tries) {
                const int prev = atomicCAS(&s_key[slot], -1, f);
                if (prev == -1 || prev == f) { found = true; break; }
                slot = (slot + 1) & (kFaceSlots - 1);
            }
#pragma unroll
            for (int c = 0; c < 18; ++c) {
                const size_t o = (size_t)((c % 6) / 3) * V * 3 + 3 * (size_t)faces[3 * f + c / 6] + (c % 3);
                if (DET == 2) {
                    const unsigned long long q = (unsigned long long)st3d_det::det_quantise(c18[c], dscale);
                    if (found) atomicAdd(reinterpret_cast<unsigned long long *>(&s_acc[slot][c]), q);
                    else atomicAdd(reinterpret_cast<unsigned long long *>(out) + o, q);
                } else {
                    if (found) atomicAdd(reinterpret_cast<float *>(&s_acc[slot][c]), c18[c]);
                    else atomicAdd(out + o, c18[c]);
                }
            }
        }
    }
    if (DET == 1) {
        const float t = st3d_det::det_block_sum(bound, s4);
        if (tid == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        return;
    }
    __syncthreads();
    for (int e = tid; e < kFaceSlots * 18; e += 256) {
        const int slot = e / 18, c = e - slot * 18;
        const int fk = s_key[slot];
        if (fk < 0) continue;
        const acc_t v = s_acc[slot][c];
        if (v == (acc_t)0) continue;
        const size_t o = (size_t)((c % 6) / 3) * V * 3 + 3 * (size_t)faces[3 * fk + c / 6] + (c % 3);
        if (DET == 2) atomicAdd(reinterpret_cast<unsigned long long *>(out) + o, (unsigned long long)v);
        else atomicAdd(out + o, (float)v);
    }
}

}  // namespace

extern "C" size_t st3d_vertex_normals_scratch_floats(int F) { return (size_t)9 * F; }

extern "C" int st3d_vertex_normals(const float *verts, const int32_t *faces, int V, int F, const int32_t *inc_off,
                                   const int32_t *inc_ref, float *scratch, float *normals, float *unnormalised,
                                   st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && faces && inc_off && inc_ref && scratch && normals && unnormalised);
    ST3D_CHECK_ARG(V > 0 && F > 0);
    hipStream_t s = st3d::as_stream(stream);
    face_normal_kernel<<<st3d::cdiv(F, 256), 256, 0, s>>>(verts, faces, F, scratch);
    ST3D_LAUNCH_CHECK();
    vertex_normal_gather_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(scratch, inc_off, inc_ref, V, normals, unnormalised);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_vertex_normals_bwd(const float *verts, const int32_t *faces, int V, int F, const int32_t *inc_off,
                                       const int32_t *inc_ref, const float *unnormalised, const float *grad_normals,
                                       const float *grad_pos, float *scratch, float *grad_verts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && faces && inc_off && inc_ref && unnormalised && grad_normals && scratch && grad_verts);
    ST3D_CHECK_ARG(V > 0 && F > 0);
    hipStream_t s = st3d::as_stream(stream);
    face_normal_bwd_kernel<<<st3d::cdiv(F, 256), 256, 0, s>>>(verts, faces, F, unnormalised, grad_normals, scratch);
    ST3D_LAUNCH_CHECK();
    vertex_normal_bwd_gather_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(scratch, inc_off, inc_ref, V, grad_pos, grad_verts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_phong_scatter_workspace_bytes(int B, int V, int S) {
    const size_t tiles = (size_t)((S + 15) / 16);
    return st3d_det::workspace_bytes((size_t)V * 6, tiles * tiles * B);
}

extern "C" int st3d_phong_scatter(const float *grad_np, const int32_t *pix_to_face, const float *bary, const int32_t *faces,
                                  int B, int V, int F, int S, int K, float *out, void *workspace, size_t workspace_bytes,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_np && pix_to_face && bary && faces && out);
    ST3D_CHECK_ARG(B > 0 && V > 0 && F > 0 && S > 0 && K >= 1);
    hipStream_t s = st3d::as_stream(stream);
    const int tiles = (S + 15) / 16;
    const size_t nacc = (size_t)V * 6;
    if (!workspace) {
        ST3D_HIP(hipMemsetAsync(out, 0, nacc * sizeof(float), s));
        phong_scatter_kernel<0><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_np, pix_to_face, bary, faces, V, S, K, tiles, out,
                                                                        nullptr, nullptr);
        ST3D_LAUNCH_CHECK();
        return ST3D_OK;
    }
    ST3D_CHECK_ARG(workspace_bytes >= st3d_phong_scatter_workspace_bytes(B, V, S) && ((uintptr_t)workspace & 15) == 0);
    const size_t np = (size_t)tiles * tiles * B;
    const st3d_det::DetRun det(workspace, np, nacc);
    phong_scatter_kernel<1><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_np, pix_to_face, bary, faces, V, S, K, tiles, nullptr,
                                                                    nullptr, det.partials);
    ST3D_LAUNCH_CHECK();
    ST3D_TRY(det.scale_and_clear(s));
    phong_scatter_kernel<2><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_np, pix_to_face, bary, faces, V, S, K, tiles,
                                                                    reinterpret_cast<float *>(det.acc), det.hdr, nullptr);
    ST3D_LAUNCH_CHECK();
    return det.convert(0, out, s);
}
