// color.hip -- colour control for the style terms ("Colour preservation"; Gatys et al. 2017, section 5): the
// luminance of an image and its exact transpose, the recombination of an optimised luminance with the chroma of an
// original, an affine recolouring, and the first and second moments of the pixels of an image.
//
// Every image is planar (B,3,P) fp32, P = H W pixels per channel plane.  The arithmetic, restated in numpy by
// tests/_colorref.py (W = (0.299f, 0.587f, 0.114f), Rec. 601, as fp32 constants; fmaf is one rounding):
//     Y(r, g, b)   = fmaf(W2, b, fmaf(W1, g, W0 * r))
//     luma_fwd     out_c = Y(x)                                  for c = 0, 1, 2: a grey image is three equal planes
//     luma_bwd     s = (g0 + g1) + g2,  out_c = W_c * s          the exact transpose of luma_fwd
//     recombine    d = Y(opt) - Y(orig),  out_c = orig_c + d     (the inverse YIQ transform multiplies Y by the column
//                                                                 (1,1,1): a new Y with the old I and Q adds d to all three)
//     affine       out_c = fmaf(A[c][2], x2, fmaf(A[c][1], x1, fmaf(A[c][0], x0, b_c))), then with clamp != 0
//                  v < 0 ? 0 : (v > 1 ? 1 : v)                   (a NaN fails both comparisons and stays, as in torch.clamp)
//     stats        over the pixels whose mask byte is non-zero: the count, sum x_c, sum x_c x_d (c <= d), the products formed
//                  in fp64 from the fp32 values (exact), the sums in fp64 in a fixed two-stage order
// All of it is per pixel: NaN and +-Inf stay in their own pixel (stats: in their own sums).  No atomics anywhere: gathers
// and fixed-order reductions, two runs give the same bits.
//
// The four streaming kernels read every input once and write the output once.  A thread owns four consecutive pixels of one
// image.  When P % 4 == 0 and the buffers are 16-byte aligned every channel plane starts on a 16-byte boundary and the
// thread moves its pixels as one float4 per plane (one 1 KiB access per wave and plane); otherwise the three planes of an
// image are misaligned against each other (plane c starts c P floats in), no pixel quad is aligned in all of them, and the
// kernel takes scalar accesses -- consecutive lanes on consecutive floats, still coalesced.  The tail (P % 4 pixels of the
// scalar form) is guarded per pixel.
//
// stats: a workgroup of 256 threads owns kChunk = 4096 consecutive pixels of one image; thread t takes pixels t, t + 256, ...
// of the chunk in ascending order into ten fp64 accumulators; the 256 x 10 values are folded in LDS by halving strides
// (t += t + s for s = 128 ... 1), and the ten sums of the workgroup go to partials[block * 10 ...].  A second launch of one
// workgroup adds the partials of each of the ten quantities in block order.  Blocks are ordered image-major.
// Built with -ffp-contract=off: the only fused operations are the fmaf written here.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kQuad = 4;                        // pixels per thread in the streaming kernels
constexpr int kChunk = 4096;                    // pixels per workgroup in stats
constexpr int kSums = 10;
constexpr float kW0 = 0.299f, kW1 = 0.587f, kW2 = 0.114f;

__device__ __forceinline__ float luma_of(float r, float g, float b) { return fmaf(kW2, b, fmaf(kW1, g, kW0 * r)); }

struct Px {
    float c[3];
};

enum Op { kLumaFwd, kLumaBwd, kRecombine, kAffine };

struct Affine {             // travels by value in the kernel arguments: no upload, no device pointer
    float A[9], b[3];       // A row-major (3,3)
    int clamp;
};

template <int OP>
__device__ __forceinline__ Px pixel_op(const Px &x, const Px &y, const float *__restrict__ A, const float *__restrict__ b, int clamp) {
    Px o;
    if (OP == kLumaFwd) {
        const float v = luma_of(x.c[0], x.c[1], x.c[2]);
        o.c[0] = o.c[1] = o.c[2] = v;
    } else if (OP == kLumaBwd) {
        const float s = (x.c[0] + x.c[1]) + x.c[2];
        o.c[0] = kW0 * s;
        o.c[1] = kW1 * s;
        o.c[2] = kW2 * s;
    } else if (OP == kRecombine) {      // x = optimised, y = original
        const float d = luma_of(x.c[0], x.c[1], x.c[2]) - luma_of(y.c[0], y.c[1], y.c[2]);
        for (int c = 0; c < 3; ++c) o.c[c] = y.c[c] + d;
    } else {
        for (int c = 0; c < 3; ++c) {
            float v = fmaf(A[3 * c + 2], x.c[2], fmaf(A[3 * c + 1], x.c[1], fmaf(A[3 * c], x.c[0], b[c])));
            if (clamp) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
            o.c[c] = v;
        }
    }
    return o;
}

// grid (quads of an image, B); VEC: P % 4 == 0 and every buffer 16-byte aligned
template <int OP, bool VEC>
__global__ __launch_bounds__(kThreads) void stream_kernel(const float *__restrict__ x, const float *__restrict__ y, Affine aff, size_t P,
                                                          float *__restrict__ out) {
    const size_t img = (size_t)blockIdx.y * 3 * P;
    float A[9] = {}, b[3] = {};
    if (OP == kAffine) {
        for (int i = 0; i < 9; ++i) A[i] = aff.A[i];
        for (int i = 0; i < 3; ++i) b[i] = aff.b[i];
    }
    if (VEC) {
        const size_t p0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * kQuad;
        if (p0 >= P) return;
        float4 xv[3], yv[3], ov[3];
        for (int c = 0; c < 3; ++c) {
            xv[c] = *reinterpret_cast<const float4 *>(x + img + c * P + p0);
            if (OP == kRecombine) yv[c] = *reinterpret_cast<const float4 *>(y + img + c * P + p0);
        }
#pragma unroll
        for (int k = 0; k < kQuad; ++k) {
            Px a, o, d = {};
            for (int c = 0; c < 3; ++c) {
                a.c[c] = reinterpret_cast<const float *>(&xv[c])[k];
                if (OP == kRecombine) d.c[c] = reinterpret_cast<const float *>(&yv[c])[k];
            }
            o = pixel_op<OP>(a, d, A, b, aff.clamp);
            for (int c = 0; c < 3; ++c) reinterpret_cast<float *>(&ov[c])[k] = o.c[c];
        }
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(out + img + c * P + p0) = ov[c];
    } else {
        // lane l of the block's pass k touches pixel base + k * kThreads + l: consecutive lanes, consecutive floats
        const size_t base = (size_t)blockIdx.x * kThreads * kQuad + threadIdx.x;
        for (int k = 0; k < kQuad; ++k) {
            const size_t p = base + (size_t)k * kThreads;
            if (p >= P) break;
            Px a, o, d = {};
            for (int c = 0; c < 3; ++c) {
                a.c[c] = x[img + c * P + p];
                if (OP == kRecombine) d.c[c] = y[img + c * P + p];
            }
            o = pixel_op<OP>(a, d, A, b, aff.clamp);
            for (int c = 0; c < 3; ++c) out[img + c * P + p] = o.c[c];
        }
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int OP>
int launch_stream(const float *x, const float *y, Affine aff, int B, size_t P, float *out, hipStream_t stream) {
    const size_t quads = (P + kQuad - 1) / kQuad;
    const size_t blocks = (quads + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffu || B > 65535) {
        st3d::set_error("color: %d images of %zu pixels do not fit one grid", B, P);
        return ST3D_E_INVALID;
    }
    const dim3 grid((unsigned)blocks, (unsigned)B);
    const bool vec = P % kQuad == 0 && aligned16(x) && aligned16(out) && (y == nullptr || aligned16(y));
    if (vec)
        stream_kernel<OP, true><<<grid, kThreads, 0, stream>>>(x, y, aff, P, out);
    else
        stream_kernel<OP, false><<<grid, kThreads, 0, stream>>>(x, y, aff, P, out);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

// grid (chunks of an image, B): partials[(b * chunks + chunk) * 10 + q]
__global__ __launch_bounds__(kThreads) void stats_chunk_kernel(const float *__restrict__ x, const uint8_t *__restrict__ mask, size_t P,
                                                               double *__restrict__ partials) {
    __shared__ double acc[kSums][kThreads];
    const size_t img = (size_t)blockIdx.y * 3 * P;
    const size_t p0 = (size_t)blockIdx.x * kChunk;
    const size_t p1 = p0 + kChunk < P ? p0 + kChunk : P;
    double s[kSums];
    for (int q = 0; q < kSums; ++q) s[q] = 0.0;
    for (size_t p = p0 + threadIdx.x; p < p1; p += kThreads) {
        if (mask != nullptr && mask[(size_t)blockIdx.y * P + p] == 0) continue;
        const double r = (double)x[img + p], g = (double)x[img + P + p], b = (double)x[img + 2 * P + p];
        s[0] += 1.0;
        s[1] += r;
        s[2] += g;
        s[3] += b;
        s[4] += r * r;
        s[5] += r * g;
        s[6] += r * b;
        s[7] += g * g;
        s[8] += g * b;
        s[9] += b * b;
    }
    for (int q = 0; q < kSums; ++q) acc[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride)
            for (int q = 0; q < kSums; ++q) acc[q][threadIdx.x] += acc[q][threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x < kSums) partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kSums + threadIdx.x] = acc[threadIdx.x][0];
}

__global__ __launch_bounds__(st3d::kWave) void stats_finish_kernel(const double *__restrict__ partials, long blocks, double *__restrict__ out10) {
    const int q = threadIdx.x;
    if (q >= kSums) return;
    double s = 0.0;
    for (long k = 0; k < blocks; ++k) s += partials[k * kSums + q];
    out10[q] = s;
}

inline bool shape_ok(int B, size_t P) { return B > 0 && P > 0 && P <= ((size_t)1 << 40) / 3 / (size_t)B; }

}  // namespace

extern "C" int st3d_color_stats_chunk(void) { return kChunk; }

extern "C" int st3d_luma_fwd(const float *x, int B, size_t P, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && out && x != out);
    ST3D_CHECK_ARG(shape_ok(B, P));
    return launch_stream<kLumaFwd>(x, nullptr, Affine{}, B, P, out, st3d::as_stream(stream));
}

extern "C" int st3d_luma_bwd(const float *g, int B, size_t P, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(g && out && g != out);
    ST3D_CHECK_ARG(shape_ok(B, P));
    return launch_stream<kLumaBwd>(g, nullptr, Affine{}, B, P, out, st3d::as_stream(stream));
}

extern "C" int st3d_luma_recombine(const float *opt, const float *orig, int B, size_t P, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(opt && orig && out && opt != out && orig != out);
    ST3D_CHECK_ARG(shape_ok(B, P));
    return launch_stream<kRecombine>(opt, orig, Affine{}, B, P, out, st3d::as_stream(stream));
}

extern "C" int st3d_color_affine(const float *x, const float *A9, const float *b3, int clamp, int B, size_t P, float *out,
                                 st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && A9 && b3 && out && x != out);
    ST3D_CHECK_ARG(shape_ok(B, P));
    Affine aff{};
    for (int i = 0; i < 9; ++i) aff.A[i] = A9[i];
    for (int i = 0; i < 3; ++i) aff.b[i] = b3[i];
    aff.clamp = clamp != 0;
    return launch_stream<kAffine>(x, nullptr, aff, B, P, out, st3d::as_stream(stream));
}

extern "C" int st3d_color_stats(const float *x, const uint8_t *mask, int B, size_t P, double *partials, double *out10,
                                st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && partials && out10 && partials != out10);
    ST3D_CHECK_ARG(shape_ok(B, P));
    const size_t chunks = (P + kChunk - 1) / kChunk;
    ST3D_CHECK_ARG(chunks <= 0x7fffffffu && B <= 65535);
    const hipStream_t s = st3d::as_stream(stream);
    stats_chunk_kernel<<<dim3((unsigned)chunks, (unsigned)B), kThreads, 0, s>>>(x, mask, P, partials);
    ST3D_LAUNCH_CHECK();
    stats_finish_kernel<<<1, st3d::kWave, 0, s>>>(partials, (long)(chunks * (size_t)B), out10);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
