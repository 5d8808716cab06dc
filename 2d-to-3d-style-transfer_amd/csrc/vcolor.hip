// vcolor.hip -- per-vertex colours (PyTorch3D TexturesVertex) on the hard renderer: barycentric interpolation of a (V,3)
// colour array + unlit white-ambient shading + the K = 1 softmax blend, forward and backward: the device work of
// TexturesVertex.sample_textures / interpolate_face_attributes under SoftPhongShader(AmbientLights) and of their autograd
// backward.  No UV atlas and no texture map: the colour of a covered pixel is
//     t_c = b0 C[v0][c] + b1 C[v1][c] + b2 C[v2][c]        (v_i = faces[f][i], left to right, no contraction)
//     rgb_c = (wnum t_c + delta 1.0f) / denom               (blend_k1 and the mask exactly as shade.hip's shade_fwd_kernel)
// and white with mask 0 where there is no face.  Backward, with k = wnum / denom and gk_c = g_c k:
//     dC[v_i][c] += b_i gk_c  (nine deposits per covered pixel),   db_i = sum_c gk_c C[v_i][c]  (0 on uncovered pixels);
// nothing flows through dists / zbuf (as on the UV path).
// HBM-bound like the shade kernels: 24 B of fragments + 16 B written per pixel forward (the three face indices and nine
// colour floats of a covered pixel come from L2: 35 KB of colours for the cow), 24 + 12 B read backward.
// Built with shade.hip's flags (-ffp-contract=off, correctly rounded division): blend and mask are its bits.
#include <type_traits>

#include "common.h"
#include "det.h"

namespace {

constexpr float kSigma = 1e-4f, kGamma = 1e-4f, kBlendEps = 1e-10f, kZnear = 1.0f, kZfar = 100.0f;

struct Blend { float prob, wnum, delta, denom; };

// (shade.hip's blend_k1: the same expressions in the same order)
__device__ __forceinline__ Blend blend_k1(float dist, float z) {
    Blend o;
    o.prob = 1.0f / (1.0f + expf(dist / kSigma));
    const float z_inv = (kZfar - z) / (kZfar - kZnear);
    const float z_max = fmaxf(z_inv, kBlendEps);
    o.wnum = o.prob * expf((z_inv - z_max) / kGamma);
    o.delta = fmaxf(expf((kBlendEps - z_max) / kGamma), kBlendEps);
    o.denom = o.wnum + o.delta;
    return o;
}

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
// vertex index in the texel's place: the nine contributions of a pixel are summed per vertex in LDS first and each distinct
// vertex of the tile then costs three global atomics.  A tile in which no pixel has a face writes its zero rows of gbary and
// leaves (one workgroup-wide OR).
//   s_key   open addressing on the vertex index; kVcSlots >= 2 x the 3 x 256 corners a tile can deposit into, so the probe
//           always terminates and no overflow path to global memory exists.  The lane whose CAS claimed a slot owns the vertex.
//   s_vert, s_acc   one compact entry per distinct vertex, kVcMax = 3 x 256: after a barrier every owner takes the next
//           entry (one LDS atomic per wave and corner), zeroes its three sums, notes the vertex and replaces the key by the
//           entry's number; after the next barrier every lane reads the entries of its slots and deposits.
// 29 KB + 4 B of LDS in fixed point, 20 KB + 4 B in float.
// DET 0: float table + float global atomics into gcol (V,3).  DET 1: the same binning in 64-bit fixed point (det.h): gcol is
// the int64 accumulator array and `det` holds the power-of-two scale.  gcol == nullptr (the vertices alone are optimised):
// no table, gbary only.
constexpr int kVcSlots = 2048;
constexpr int kVcMax = 768;

template <int DET>
__global__ __launch_bounds__(256) void shade_vc_bwd_kernel(const float *__restrict__ grad_rgb, const int32_t *__restrict__ p2f,
                                                           const float *__restrict__ bary, const float *__restrict__ zbuf,
                                                           const float *__restrict__ dists, const int32_t *__restrict__ faces,
                                                           const float *__restrict__ col, int B, int S, int tiles_x,
                                                           float *__restrict__ gcol, float *__restrict__ gbary,
                                                           const st3d_det::DetHeader *__restrict__ det) {
    typedef typename std::conditional<DET != 0, unsigned long long, float>::type acc_t;
    __shared__ int s_key[kVcSlots];
    __shared__ int s_vert[kVcMax];
    __shared__ acc_t s_acc[kVcMax][3];
    __shared__ int s_count;
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
        for (int e = tid; e < kVcSlots; e += 256) s_key[e] = -1;
        if (tid == 0) s_count = 0;
        __syncthreads();
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
    if (!gcol) return;
    const bool dep = f >= 0;
    int slot[3] = {0, 0, 0};
    unsigned mine = 0;               // bit j: this lane's CAS claimed the slot of corner j
    if (dep) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int v = dep_vert[j];
            int s = (int)(((unsigned)v * 2654435761u) >> 21) & (kVcSlots - 1);
            for (;;) {
                const int prev = atomicCAS(&s_key[s], -1, v);
                if (prev == -1) mine |= 1u << j;
                if (prev == -1 || prev == v) break;
                s = (s + 1) & (kVcSlots - 1);
            }
            slot[j] = s;
        }
    }
    __syncthreads();                 // every key is in: nobody probes any more
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool own = mine >> j & 1;
        const unsigned long long owners = __ballot(own);
        if (owners == 0) continue;
        const int lane = tid & 63, leader = __ffsll((long long)owners) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&s_count, __popcll(owners));
        base = __shfl(base, leader);
        if (own) {
            const int e = base + __popcll(owners & ((1ull << lane) - 1ull));
            s_vert[e] = dep_vert[j];
            s_acc[e][0] = (acc_t)0; s_acc[e][1] = (acc_t)0; s_acc[e][2] = (acc_t)0;
            s_key[slot[j]] = e;
        }
    }
    __syncthreads();
    if (dep) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int e = s_key[slot[j]];
            const float w = dep_w[j];
            if (DET) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    atomicAdd(reinterpret_cast<unsigned long long *>(&s_acc[e][ch]),
                              (unsigned long long)st3d_det::det_quantise(w * dep_g[ch], dscale));
            } else {
                atomicAdd(reinterpret_cast<float *>(&s_acc[e][0]), w * dep_g[0]);
                atomicAdd(reinterpret_cast<float *>(&s_acc[e][1]), w * dep_g[1]);
                atomicAdd(reinterpret_cast<float *>(&s_acc[e][2]), w * dep_g[2]);
            }
        }
    }
    __syncthreads();
    const int used = s_count * 3;
    for (int e = tid; e < used; e += 256) {
        const int entry = e / 3, c = e - entry * 3;
        const acc_t v = s_acc[entry][c];
        if (v == (acc_t)0) continue;
        const int vert = s_vert[entry];
        if (DET) atomicAdd(reinterpret_cast<unsigned long long *>(gcol) + (size_t)vert * 3 + c, (unsigned long long)v);
        else atomicAdd(gcol + (size_t)vert * 3 + c, (float)v);
    }
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
constexpr int kDetPartials = 1024;

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
    return V > 0 ? st3d_det::workspace_bytes((size_t)V * 3, kDetPartials) : 0;
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
    auto *hdr = reinterpret_cast<st3d_det::DetHeader *>(workspace);
    float *partials = st3d_det::partials_of(workspace);
    long long *acc = st3d_det::accum_of(workspace, kDetPartials);
    const size_t nacc = (size_t)V * 3;
    vc_abs_sum_kernel<<<kDetPartials, 256, 0, s>>>(grad_rgb, pix_to_face, bary, B, S, partials);
    ST3D_LAUNCH_CHECK();
    st3d_det::det_scale_kernel<<<1, 256, 0, s>>>(partials, kDetPartials, hdr);
    ST3D_LAUNCH_CHECK();
    ST3D_HIP(hipMemsetAsync(acc, 0, nacc * sizeof(long long), s));
    const int tiles = (S + 15) / 16;
    shade_vc_bwd_kernel<1><<<dim3(tiles * tiles, B), 256, 0, s>>>(grad_rgb, pix_to_face, bary, zbuf, dists, faces, verts_colors, B,
                                                                  S, tiles, reinterpret_cast<float *>(acc), grad_bary, hdr);
    ST3D_LAUNCH_CHECK();
    st3d_det::det_convert_kernel<<<st3d::cdiv((long)nacc, 256), 256, 0, s>>>(acc, nacc, hdr, 1, grad_colors);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
