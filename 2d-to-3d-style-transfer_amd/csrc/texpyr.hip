// texpyr.hip -- the texture pyramid: the texture map as the sum of L maps of sides T, T/2, ... T/2^(L-1), each
// upsampled to T x T, and the adjoint of that sum.  `params` is ONE flat fp32 tensor; level l is the (T_l, T_l, 3) row-major
// block at offset 3 * sum_{k<l} T_k^2 (the HWC layout of a texture map).
//     synth:    acc_{L-1} = level_{L-1};  acc_l = level_l + up2(acc_{l+1});  texture = acc_0
//     adjoint:  g_0 = grad_texture;  g_{l+1} = up2^T(g_l);  grad level_l = g_l
// up2 is F.interpolate(scale_factor=2, mode='bilinear', align_corners=False) per channel: fine 2j takes
// 0.25 c[j-1] + 0.75 c[j], fine 2j+1 takes 0.75 c[j] + 0.25 c[j+1], indices clamped to [0, n-1]; in 2-D
//     wy_a * (wx_a * c[ya][xa] + wx_b * c[ya][xb]) + wy_b * (wx_a * c[yb][xa] + wx_b * c[yb][xb]).
// up2^T is the gather of that: coarse j collects fine 2j-1, 2j, 2j+1, 2j+2 with weights 0.25, 0.75, 0.75, 0.25; at j = 0
// fine -1 does not exist and fine 0 weighs 0.75 + 0.25 = 1, at j = n-1 the same on the other side.  Taps that do not exist
// are SKIPPED, not weighted by zero, so a NaN stays inside its footprint.  No atomics, one fixed order: bitwise reproducible.
//
// Launches: synth is ONE whatever L is -- a workgroup owns a 32 x 32 fine tile and rebuilds the chain for it in LDS from
// the coarsest level down (level l of a tile is at most 32 / 2^l + 2 texels a side: two ping-pong buffers of 18 x 18 x 3).
// The adjoint is at most TWO: the first reduces levels 1..3 in LDS per 32 x 32 fine tile (the fine gradient region a tile's
// 4 x 4 level-3 outputs need is 46 x 46: the halo grows by 2 * halo + 2 a level) and copies g_0 into the level-0 block on
// the way, so grad_texture leaves HBM once; the second, one workgroup, finishes levels 4.. from the level-3 block (128^2 at
// T = 1024), keeping every level of side <= 64 in LDS for the next one.  Halo values are recomputed by the neighbouring tiles in the same operation order; only the owner stores, so
// every output element is produced by exactly one thread.  Only level 0's block is 16-byte aligned (T = 6 holds 108
// floats): float4 is used on the level-0 block and the texture when T % 4 == 0, everything deeper is 4-byte accesses.
// Compiled without FMA contraction: the roundings are the ones written here (DESIGN 7 counts them for the test bounds).
#include "common.h"

namespace {

constexpr int kMaxLevels = 16;
constexpr int kMaxSide = 16384;          // 3 * T^2 < 2^31: indices inside one block are ints
constexpr int FT = 32;                   // fine tile side of both kernels
constexpr int FS = FT / 2 + 2;           // synth: widest LDS region (level 1 of a tile)
constexpr int KMAXB = 3;                 // adjoint: levels reduced by the first launch
constexpr int BS0 = 8 * (FT >> 3) + 14;  // adjoint: widest level-0 region (46), level-1 (22), level-2 (10)
constexpr int BS1 = 4 * (FT >> 3) + 6;
constexpr int BS2 = 2 * (FT >> 3) + 2;

__host__ __device__ inline size_t level_offset(int T, int l) {
    size_t off = 0;
    for (int k = 0; k < l; ++k) off += (size_t)3 * (T >> k) * (T >> k);
    return off;
}

// up2 of the coarse map held in LDS (`src`: rows of `stride` texels, origin (sx, sy), side n) at fine (gy, gx), channel c
__device__ __forceinline__ float up2_at(const float *src, int stride, int sx, int sy, int n, int gy, int gx, int c) {
    const int jy = gy >> 1, jx = gx >> 1;
    const bool oy = gy & 1, ox = gx & 1;
    int ya = oy ? jy : jy - 1, yb = oy ? jy + 1 : jy;
    int xa = ox ? jx : jx - 1, xb = ox ? jx + 1 : jx;
    const float wya = oy ? 0.75f : 0.25f, wyb = oy ? 0.25f : 0.75f;
    const float wxa = ox ? 0.75f : 0.25f, wxb = ox ? 0.25f : 0.75f;
    ya = max(ya, 0); xa = max(xa, 0);
    yb = min(yb, n - 1); xb = min(xb, n - 1);
    const int ra = ((ya - sy) * stride - sx) * 3 + c, rb = ((yb - sy) * stride - sx) * 3 + c;
    return wya * (wxa * src[ra + xa * 3] + wxb * src[ra + xb * 3]) + wyb * (wxa * src[rb + xa * 3] + wxb * src[rb + xb * 3]);
}

// One launch for any L >= 2.  VEC: T % 4 == 0, so every row of a tile starts 16-byte aligned in level 0 and in the texture.
template <bool VEC>
__global__ __launch_bounds__(256) void texpyr_synth_kernel(const float *__restrict__ params, int T, int L,
                                                           float *__restrict__ texture) {
    __shared__ float buf[2][FS * FS * 3];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FT, y0 = blockIdx.y * FT;
    const int x1 = min(x0 + FT, T) - 1, y1 = min(y0 + FT, T) - 1;

    // the chain, coarsest level first: acc_l on the region the tile needs, [lo, hi] = [(lo_0 - (2^l - 1)) >> l, (hi_0 + 2^l - 1) >> l]
    size_t off = level_offset(T, L - 1);
    int cur = 0, psx = 0, psy = 0;                       // origin of the region in buf[cur ^ 1]
    for (int l = L - 1; l >= 1; --l) {
        const int n = T >> l, m = (1 << l) - 1;
        const int lox = max((x0 - m) >> l, 0), hix = min((x1 + m) >> l, n - 1);
        const int loy = max((y0 - m) >> l, 0), hiy = min((y1 + m) >> l, n - 1);
        const int w3 = (hix - lox + 1) * 3, h = hiy - loy + 1;
        const float *lvl = params + off;
        float *dst = buf[cur];
        const float *src = buf[cur ^ 1];
        for (int i = tid; i < h * w3; i += 256) {
            const int r = i / w3, f = i - r * w3;
            const int x = f / 3, c = f - 3 * x;
            float v = lvl[((loy + r) * n + lox) * 3 + f];
            if (l < L - 1) v = v + up2_at(src, FS, psx, psy, n >> 1, loy + r, lox + x, c);
            dst[r * FS * 3 + f] = v;
        }
        __syncthreads();
        psx = lox; psy = loy;
        cur ^= 1;
        off -= (size_t)3 * (T >> (l - 1)) * (T >> (l - 1));
    }

    // texture tile = level 0 + up2(acc_1), written once
    const float *src = buf[cur ^ 1];
    const int w3 = (x1 - x0 + 1) * 3, h = y1 - y0 + 1, n1 = T >> 1;
    if (VEC) {
        const int w4 = w3 >> 2;                          // the tile is a multiple of 4 texels wide when T % 4 == 0
        for (int i = tid; i < h * w4; i += 256) {
            const int r = i / w4, q = i - r * w4;
            const size_t at = ((size_t)(y0 + r) * T + x0) * 3 + 4 * q;
            float4 v = *reinterpret_cast<const float4 *>(params + at);
            float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = 4 * q + k, x = f / 3, c = f - 3 * x;
                e[k] = e[k] + up2_at(src, FS, psx, psy, n1, y0 + r, x0 + x, c);
            }
            *reinterpret_cast<float4 *>(texture + at) = make_float4(e[0], e[1], e[2], e[3]);
        }
    } else {
        for (int i = tid; i < h * w3; i += 256) {
            const int r = i / w3, f = i - r * w3;
            const int x = f / 3, c = f - 3 * x;
            const size_t at = ((size_t)(y0 + r) * T + x0) * 3 + f;
            texture[at] = params[at] + up2_at(src, FS, psx, psy, n1, y0 + r, x0 + x, c);
        }
    }
}

// 1-D weight of tap t (fine index 2j - 1 + t) of coarse j on a side of n coarse texels; the tap exists iff 0 <= 2j-1+t < 2n
__device__ __forceinline__ float tap_weight(int t, int j, int n) {
    if (t == 1) return j == 0 ? 1.0f : 0.75f;
    if (t == 2) return j == n - 1 ? 1.0f : 0.75f;
    return 0.25f;
}

// up2^T at coarse (jy, jx), channel c, of the fine map `src` (rows of `stride` texels, origin (sx, sy), side 2n).  The 16
// loads are unconditional (at clamped, always valid indices) so that they are in flight together; a tap that does not exist
// contributes the constant 0, never 0 * what was loaded there.
__device__ __forceinline__ float up2t_at(const float *src, int stride, int sx, int sy, int n, int jy, int jx, int c) {
    float v[4][4];
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
        const int fy = min(max(2 * jy - 1 + ty, 0), 2 * n - 1);
        const int row = ((fy - sy) * stride - sx) * 3 + c;
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) {
            const int fx = min(max(2 * jx - 1 + tx, 0), 2 * n - 1);
            v[ty][tx] = src[row + fx * 3];
        }
    }
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
        const int fy = 2 * jy - 1 + ty;
        float s = 0.f;
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) {
            const int fx = 2 * jx - 1 + tx;
            s += tap_weight(tx, jx, n) * (fx < 0 || fx >= 2 * n ? 0.f : v[ty][tx]);
        }
        acc += tap_weight(ty, jy, n) * (fy < 0 || fy >= 2 * n ? 0.f : s);
    }
    return acc;
}

// One level of the first adjoint launch: g_l = up2^T(g_{l-1}) on [lox, hix] x [loy, hiy], kept in LDS (dst, may be null) for
// the next level; the part inside the tile's own [ox0, ox1] x [oy0, oy1] goes to the level's block.
__device__ __forceinline__ void reduce_level(const float *src, int sstride, int sx, int sy, float *dst, int dstride, int n,
                                             int lox, int hix, int loy, int hiy, int ox0, int ox1, int oy0, int oy1,
                                             float *__restrict__ block) {
    const int w3 = (hix - lox + 1) * 3, h = hiy - loy + 1;
    for (int i = threadIdx.x; i < h * w3; i += 256) {
        const int r = i / w3, f = i - r * w3;
        const int x = f / 3, c = f - 3 * x;
        const int jy = loy + r, jx = lox + x;
        const float v = up2t_at(src, sstride, sx, sy, n, jy, jx, c);
        if (dst) dst[r * dstride * 3 + f] = v;
        if (jy >= oy0 && jy <= oy1 && jx >= ox0 && jx <= ox1) block[(jy * n + jx) * 3 + c] = v;
    }
}

// First adjoint launch: levels 0..K (K = min(L - 1, 3)) of grad_params for one 32 x 32 fine tile.
template <bool VEC>
__global__ __launch_bounds__(256) void texpyr_adjoint_kernel(const float *__restrict__ g, int T, int K,
                                                             float *__restrict__ gp) {
    __shared__ float b0[BS0 * BS0 * 3];
    __shared__ float b1[BS1 * BS1 * 3];
    __shared__ float b2[BS2 * BS2 * 3];
    const int tid = threadIdx.x;
    // own[l] = [(FT >> l) * b, min((FT >> l) * (b + 1), T_l) - 1]; need[K] = own[K], need[l - 1] = [2 lo - 1, 2 hi + 2]
    int olx[KMAXB + 1], ohx[KMAXB + 1], oly[KMAXB + 1], ohy[KMAXB + 1];
    int nlx[KMAXB + 1], nhx[KMAXB + 1], nly[KMAXB + 1], nhy[KMAXB + 1];
#pragma unroll
    for (int l = 0; l <= KMAXB; ++l) {
        const int n = T >> l, t = FT >> l, d = K - l;       // d < 0: level not reduced here, never read
        olx[l] = t * blockIdx.x; ohx[l] = min(t * (blockIdx.x + 1), n) - 1;
        oly[l] = t * blockIdx.y; ohy[l] = min(t * (blockIdx.y + 1), n) - 1;
        const int tk = FT >> K, nk = T >> K, e = d >= 0 ? (1 << d) : 1;
        const int klx = tk * blockIdx.x, khx = min(tk * (blockIdx.x + 1), nk) - 1;
        const int kly = tk * blockIdx.y, khy = min(tk * (blockIdx.y + 1), nk) - 1;
        nlx[l] = max(e * klx - (e - 1), 0); nhx[l] = min(e * khx + 2 * (e - 1), n - 1);
        nly[l] = max(e * kly - (e - 1), 0); nhy[l] = min(e * khy + 2 * (e - 1), n - 1);
    }

    // g_0 on the needed region -> LDS; the tile's own part also -> the level-0 block (grad_texture is read here only)
    const int w3 = (nhx[0] - nlx[0] + 1) * 3, h = nhy[0] - nly[0] + 1;
    if (VEC) {
        const int w4 = ((ohx[0] - olx[0] + 1) * 3) >> 2, oh = ohy[0] - oly[0] + 1;
        for (int i = tid; i < oh * w4; i += 256) {
            const int r = i / w4, q = i - r * w4;
            const size_t at = ((size_t)(oly[0] + r) * T + olx[0]) * 3 + 4 * q;
            const float4 v = *reinterpret_cast<const float4 *>(g + at);
            *reinterpret_cast<float4 *>(gp + at) = v;
            float *d = b0 + ((oly[0] + r - nly[0]) * BS0 + (olx[0] - nlx[0])) * 3 + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    }
#pragma unroll 4
    for (int i = tid; i < h * w3; i += 256) {
        const int r = i / w3, f = i - r * w3;
        const int gy = nly[0] + r, gx = nlx[0] + f / 3;
        const bool own = gy >= oly[0] && gy <= ohy[0] && gx >= olx[0] && gx <= ohx[0];
        if (VEC && own) continue;
        const size_t at = ((size_t)gy * T + nlx[0]) * 3 + f;
        const float v = g[at];
        b0[r * BS0 * 3 + f] = v;
        if (own) gp[at] = v;
    }
    __syncthreads();

    float *blk = gp + (size_t)3 * T * T;
    reduce_level(b0, BS0, nlx[0], nly[0], K > 1 ? b1 : nullptr, BS1, T >> 1, nlx[1], nhx[1], nly[1], nhy[1],
                 olx[1], ohx[1], oly[1], ohy[1], blk);
    if (K == 1) return;
    __syncthreads();
    blk += (size_t)3 * (T >> 1) * (T >> 1);
    reduce_level(b1, BS1, nlx[1], nly[1], K > 2 ? b2 : nullptr, BS2, T >> 2, nlx[2], nhx[2], nly[2], nhy[2],
                 olx[2], ohx[2], oly[2], ohy[2], blk);
    if (K == 2) return;
    __syncthreads();
    blk += (size_t)3 * (T >> 2) * (T >> 2);
    reduce_level(b2, BS2, nlx[2], nly[2], nullptr, 0, T >> 3, nlx[3], nhx[3], nly[3], nhy[3],
                 olx[3], ohx[3], oly[3], ohy[3], blk);
}

// Second adjoint launch, ONE workgroup: levels K+1 .. L-1.  The first of them gathers from the level-K block the first launch
// wrote (1/64 of the map); from a side of TS = 64 down every level also stays in LDS (two buffers, 64^2 and 32^2 texels,
// taking turns) and the next one gathers from there, so up to T = 1024 the chain needs no global round trip.  Above that
// the levels still too large for LDS are read back from grad_params, each complete and visible before the next reads it.
constexpr int TS = 64;

__global__ __launch_bounds__(1024) void texpyr_adjoint_tail_kernel(int T, int K, int L, float *gp) {
    __shared__ float la[TS * TS * 3];
    __shared__ float lb[(TS / 2) * (TS / 2) * 3];
    float *src = gp + level_offset(T, K);
    const float *lsrc = nullptr;                // the source level in LDS, if it is there
    bool to_a = true;
    for (int l = K + 1; l < L; ++l) {
        const int n = T >> l;
        float *dst = src + (size_t)3 * (2 * n) * (2 * n);
        float *ldst = n <= TS ? (to_a ? la : lb) : nullptr;
        if (!lsrc && l > K + 1) {               // written by this workgroup, read back through the vector cache
            __threadfence();
            __syncthreads();
            __threadfence();
        }
        for (int i = threadIdx.x; i < n * n * 3; i += 1024) {
            const int t = i / 3, c = i - 3 * t;
            const int jy = t / n, jx = t - jy * n;
            const float v = lsrc ? up2t_at(lsrc, 2 * n, 0, 0, n, jy, jx, c) : up2t_at(src, 2 * n, 0, 0, n, jy, jx, c);
            dst[i] = v;
            if (ldst) ldst[i] = v;
        }
        __syncthreads();
        if (ldst) to_a = !to_a;
        lsrc = ldst;
        src = dst;
    }
}

// L >= 1, the sides halve exactly down to a coarsest side >= 2
inline bool shape_ok(int T, int L) {
    if (T < 1 || T > kMaxSide || L < 1 || L > kMaxLevels) return false;
    if (L == 1) return true;
    return (T & ((1 << (L - 1)) - 1)) == 0 && (T >> (L - 1)) >= 2;
}

}  // namespace

extern "C" size_t st3d_texpyr_numel(int T, int L) {
    return shape_ok(T, L) ? level_offset(T, L) : 0;
}

extern "C" int st3d_texpyr_synth(const float *params, int T, int L, float *texture, st3d_stream_t stream) {
    ST3D_CHECK_ARG(params && texture);
    ST3D_CHECK_ARG(shape_ok(T, L));
    ST3D_CHECK_ARG(params != texture);
    hipStream_t s = st3d::as_stream(stream);
    if (L == 1) {
        ST3D_HIP(hipMemcpyAsync(texture, params, (size_t)3 * T * T * sizeof(float), hipMemcpyDeviceToDevice, s));
        return ST3D_OK;
    }
    const dim3 grid(st3d::cdiv(T, FT), st3d::cdiv(T, FT));
    const bool vec = T % 4 == 0 && (((uintptr_t)params | (uintptr_t)texture) & 15u) == 0;
    if (vec) texpyr_synth_kernel<true><<<grid, 256, 0, s>>>(params, T, L, texture);
    else texpyr_synth_kernel<false><<<grid, 256, 0, s>>>(params, T, L, texture);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_texpyr_adjoint(const float *grad_texture, int T, int L, float *grad_params, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_texture && grad_params);
    ST3D_CHECK_ARG(shape_ok(T, L));
    ST3D_CHECK_ARG(grad_texture != grad_params);
    hipStream_t s = st3d::as_stream(stream);
    if (L == 1) {
        ST3D_HIP(hipMemcpyAsync(grad_params, grad_texture, (size_t)3 * T * T * sizeof(float), hipMemcpyDeviceToDevice, s));
        return ST3D_OK;
    }
    const int K = L - 1 < KMAXB ? L - 1 : KMAXB;
    const dim3 grid(st3d::cdiv(T, FT), st3d::cdiv(T, FT));
    const bool vec = T % 4 == 0 && (((uintptr_t)grad_texture | (uintptr_t)grad_params) & 15u) == 0;
    if (vec) texpyr_adjoint_kernel<true><<<grid, 256, 0, s>>>(grad_texture, T, K, grad_params);
    else texpyr_adjoint_kernel<false><<<grid, 256, 0, s>>>(grad_texture, T, K, grad_params);
    ST3D_LAUNCH_CHECK();
    if (L - 1 > K) {
        texpyr_adjoint_tail_kernel<<<1, 1024, 0, s>>>(T, K, L, grad_params);
        ST3D_LAUNCH_CHECK();
    }
    return ST3D_OK;
}
