// silhouette.hip -- PyTorch3D's SoftSilhouetteShader (blending.sigmoid_alpha_blend) on the fragments of the general soft
// rasteriser, and the silhouette loss built on it:
//     prob_k = sigmoid(-dists_k / sigma) on the covered layers (pix_to_face_k >= 0)
//     alpha  = 1 - prod_k (1 - prob_k)
//     d alpha / d dists_k = -prob_k * prod_j (1 - prob_j) / sigma      (the FULL product: no division, 0 at prob_k -> 1)
// Three streaming kernels, one thread per pixel; a pixel's K distances are contiguous (16-byte loads at K = 4 and 8).  All
// three go through silhouette_pixel(), whose expression is the alpha pass of soft_shade_kernel (soft.hip) and which is
// compiled like it (no FMA contraction), so the forward equals softmax_rgb_blend's alpha bit for bit and the fused loss
// equals the forward / squared difference / backward composition bit for bit.
//   bytes per pixel at K = 8: fused loss 32 + 32 + 4 read, 32 written = 100 B; forward (68 B) + squared difference (12 B)
//   + backward (100 B) = 180 B.
// A NaN distance gives a NaN prob, alpha, loss and gradient for its pixel; nothing is filtered.
#include "common.h"

namespace {

constexpr int KMAX = 8;

struct Pixel {
    int f[KMAX];
    float d[KMAX];
};

// KT = 4 / 8: the compile-time K with 16-byte loads (pointers 16-byte aligned, checked on the host); KT = 0: any K <= 8
template <int KT>
__device__ __forceinline__ void load_pixel(const int32_t *__restrict__ p2f, const float *__restrict__ dists, size_t i, int K,
                                           Pixel &px) {
    if (KT == 4 || KT == 8) {
#pragma unroll
        for (int q = 0; q < KT / 4; ++q) {
            const int4 f4 = reinterpret_cast<const int4 *>(p2f + i * KT)[q];
            const float4 d4 = reinterpret_cast<const float4 *>(dists + i * KT)[q];
            px.f[4 * q] = f4.x; px.f[4 * q + 1] = f4.y; px.f[4 * q + 2] = f4.z; px.f[4 * q + 3] = f4.w;
            px.d[4 * q] = d4.x; px.d[4 * q + 1] = d4.y; px.d[4 * q + 2] = d4.z; px.d[4 * q + 3] = d4.w;
        }
#pragma unroll
        for (int k = KT; k < KMAX; ++k) { px.f[k] = -1; px.d[k] = 0.f; }
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const bool in = k < K;
            px.f[k] = in ? p2f[i * K + k] : -1;
            px.d[k] = in ? dists[i * K + k] : 0.f;
        }
    }
}

// -> alpha; prob[k] (0 on empty layers) and keep = prod (1 - prob_k), in layer order
__device__ __forceinline__ float silhouette_pixel(const Pixel &px, float sigma, float (&prob)[KMAX], float &keep) {
    keep = 1.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        prob[k] = 0.f;
        if (px.f[k] < 0) continue;
        prob[k] = 1.0f / (1.0f + expf(px.d[k] / sigma));
        keep *= (1.0f - prob[k]);
    }
    return 1.0f - keep;
}

// grad_dists of one pixel for the incoming d loss / d alpha = ga
template <int KT>
__device__ __forceinline__ void store_grad(const Pixel &px, const float (&prob)[KMAX], float keep, float sigma, float ga,
                                           int accumulate, float *__restrict__ gd, size_t i, int K) {
    float g[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) g[k] = px.f[k] < 0 ? 0.f : ga * (-prob[k] * keep / sigma);
    if (KT == 4 || KT == 8) {
#pragma unroll
        for (int q = 0; q < KT / 4; ++q) {
            float4 *o = reinterpret_cast<float4 *>(gd + i * KT) + q;
            float4 v = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
            if (accumulate) {
                const float4 old = *o;
                v.x = px.f[4 * q] < 0 ? old.x : old.x + v.x;
                v.y = px.f[4 * q + 1] < 0 ? old.y : old.y + v.y;
                v.z = px.f[4 * q + 2] < 0 ? old.z : old.z + v.z;
                v.w = px.f[4 * q + 3] < 0 ? old.w : old.w + v.w;
            }
            *o = v;
        }
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k >= K) continue;
            if (!accumulate) gd[i * K + k] = g[k];
            else if (px.f[k] >= 0) gd[i * K + k] = gd[i * K + k] + g[k];
        }
    }
}

template <int KT>
__global__ __launch_bounds__(256) void silhouette_fwd_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ dists,
                                                             size_t n, int K, float sigma, float *__restrict__ alpha) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pixel px;
    load_pixel<KT>(p2f, dists, i, K, px);
    float prob[KMAX], keep;
    alpha[i] = silhouette_pixel(px, sigma, prob, keep);
}

template <int KT>
__global__ __launch_bounds__(256) void silhouette_bwd_kernel(const float *__restrict__ grad_alpha, const int32_t *__restrict__ p2f,
                                                             const float *__restrict__ dists, size_t n, int K, float sigma,
                                                             int accumulate, float *__restrict__ gd) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pixel px;
    load_pixel<KT>(p2f, dists, i, K, px);
    float prob[KMAX], keep;
    silhouette_pixel(px, sigma, prob, keep);
    store_grad<KT>(px, prob, keep, sigma, grad_alpha[i], accumulate, gd, i, K);
}

// partials[blk] = sum (alpha - target)^2 over the block's pixels (grid-strided, <= st3d_reduce_partials() blocks);
// gd = two_scale * (alpha - target) * d alpha / d dists in the same pass (gd may be NULL)
template <int KT>
__global__ __launch_bounds__(256) void silhouette_loss_kernel(const int32_t *__restrict__ p2f, const float *__restrict__ dists,
                                                              const float *__restrict__ target, size_t n, int K, float sigma,
                                                              float two_scale, float *__restrict__ gd,
                                                              float *__restrict__ partials) {
    float acc = 0.f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Pixel px;
        load_pixel<KT>(p2f, dists, i, K, px);
        float prob[KMAX], keep;
        const float diff = silhouette_pixel(px, sigma, prob, keep) - target[i];
        acc += diff * diff;
        if (gd) store_grad<KT>(px, prob, keep, sigma, two_scale * diff, 0, gd, i, K);
    }
    // ordered block sum: wave shuffles, then the four waves in index order (as loss.hip)
    __shared__ float s[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

inline bool aligned16(const void *a, const void *b, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

}  // namespace

#define ST3D_SILHOUETTE_SHAPE()                                        \
    ST3D_CHECK_ARG(B > 0 && S > 0);                                    \
    ST3D_CHECK_ARG(K >= 1 && K <= KMAX);                               \
    ST3D_CHECK_ARG(sigma > 0.f)

extern "C" int st3d_silhouette_fwd(const int32_t *pix_to_face, const float *dists, int B, int S, int K, float sigma,
                                   float *alpha, st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && dists && alpha);
    ST3D_SILHOUETTE_SHAPE();
    hipStream_t s = st3d::as_stream(stream);
    const size_t n = (size_t)B * S * S;
    const int grid = st3d::cdiv((long)n, 256);
    const int kt = aligned16(pix_to_face, dists) && (K == 4 || K == 8) ? K : 0;
    if (kt == 8) silhouette_fwd_kernel<8><<<grid, 256, 0, s>>>(pix_to_face, dists, n, K, sigma, alpha);
    else if (kt == 4) silhouette_fwd_kernel<4><<<grid, 256, 0, s>>>(pix_to_face, dists, n, K, sigma, alpha);
    else silhouette_fwd_kernel<0><<<grid, 256, 0, s>>>(pix_to_face, dists, n, K, sigma, alpha);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_silhouette_bwd(const float *grad_alpha, const int32_t *pix_to_face, const float *dists, int B, int S, int K,
                                   float sigma, int accumulate, float *grad_dists, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_alpha && pix_to_face && dists && grad_dists);
    ST3D_SILHOUETTE_SHAPE();
    hipStream_t s = st3d::as_stream(stream);
    const size_t n = (size_t)B * S * S;
    const int grid = st3d::cdiv((long)n, 256);
    const int kt = aligned16(pix_to_face, dists, grad_dists) && (K == 4 || K == 8) ? K : 0;
    if (kt == 8) silhouette_bwd_kernel<8><<<grid, 256, 0, s>>>(grad_alpha, pix_to_face, dists, n, K, sigma, accumulate, grad_dists);
    else if (kt == 4) silhouette_bwd_kernel<4><<<grid, 256, 0, s>>>(grad_alpha, pix_to_face, dists, n, K, sigma, accumulate, grad_dists);
    else silhouette_bwd_kernel<0><<<grid, 256, 0, s>>>(grad_alpha, pix_to_face, dists, n, K, sigma, accumulate, grad_dists);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_silhouette_loss(const int32_t *pix_to_face, const float *dists, const float *target, int B, int S, int K,
                                    float sigma, float scale, float *grad_dists, float *partials, float *loss_out,
                                    st3d_stream_t stream) {
    ST3D_CHECK_ARG(pix_to_face && dists && target && partials && loss_out);
    ST3D_SILHOUETTE_SHAPE();
    hipStream_t s = st3d::as_stream(stream);
    const size_t n = (size_t)B * S * S;
    const size_t blocks = (n + 255) / 256;
    const int np = st3d_reduce_partials();
    const int grid = (int)(blocks > (size_t)np ? (size_t)np : blocks);
    const float two_scale = 2.0f * scale;
    const int kt = aligned16(pix_to_face, dists, grad_dists) && (K == 4 || K == 8) ? K : 0;
    if (kt == 8) silhouette_loss_kernel<8><<<grid, 256, 0, s>>>(pix_to_face, dists, target, n, K, sigma, two_scale, grad_dists, partials);
    else if (kt == 4) silhouette_loss_kernel<4><<<grid, 256, 0, s>>>(pix_to_face, dists, target, n, K, sigma, two_scale, grad_dists, partials);
    else silhouette_loss_kernel<0><<<grid, 256, 0, s>>>(pix_to_face, dists, target, n, K, sigma, two_scale, grad_dists, partials);
    ST3D_LAUNCH_CHECK();
    return st3d::finish_partials(partials, grid, scale, loss_out, s);
}
