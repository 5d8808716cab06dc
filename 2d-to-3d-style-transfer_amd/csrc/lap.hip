// lap.hip -- the Laplacian content term ("Laplacian content loss"; Li, Xu, Nie and Chua 2017): the squared
// difference between the Laplacian of the average-pooled render and that of the average-pooled content image.
//
// A stack of N planes (H,W) fp32 and a pool side p in {1,2,4,8,16} that divides H and W, h = H/p >= 2, w = W/p >= 2:
//     pool   P(i,j) = ((s_0 + s_1) + ... + s_{p-1}) * (1/p^2),  s_r = ((x(ip+r, jp) + x(ip+r, jp+1)) + ...) + x(ip+r, jp+p-1):
//            every row of the block summed from left to right, the row sums added from top to bottom, then one product
//            with the exact constant 1/p^2 (p = 1: P = x, no arithmetic)
//     D      L(i,j) = 4 P(i,j) - ((P(i-1,j) + P(i+1,j)) + (P(i,j-1) + P(i,j+1))), indices clamped to the plane (replicate
//            border).  A constant plane gives 0 everywhere; along one axis row 0 of the matrix is [1, -1]: D is symmetric
//     loss   r = L(x) - T,  value = fp32((sum of (double) r * (double) r) * scale): every workgroup adds the squares of its tile
//            (thread t takes the cells t, t + 256, ... of the tile in ascending order, the 256 sums are folded by halving
//            strides), the finishing launch adds the workgroups' partials (thread t takes t, t + 256, ..., folded the same way)
//     grad   g(y,x) = k * D(r)(y / p, x / p), k = fp32(2 scale / p^2) from the host: the transpose of the pool hands every
//            pixel of a block the block's value, the transpose of D is D.  A gather, no atomics: two runs give the same bits.
//
// One workgroup of 256 threads owns a tile of kTH x kTW pooled cells (Tile<P>, st3d_lap_tile reports it in fine pixels).
//   residual launch: the fine rows of the tile's cells plus a halo go to LDS as per-cell row sums, read along W -- with W % 4
//     == 0 and 16-byte aligned planes as float4 (a halo of max(1, 4/p) cells keeps every load aligned), otherwise by scalars;
//     the row sums fold to pooled cells in LDS, the stencil reads those.  The image is read once plus the halo cells
//     ((kTH + 2)(kTW + 2) / (kTH kTW) of it, the re-reads served by L2); r is written at pooled size.
//   gradient launch: r of the tile plus a halo of one cell goes to LDS, k D(r) is formed once per cell, and every fine row
//     of the tile is written in full, as float4 where the alignment allows.
//   finishing launch: one workgroup.
// Planes whose pooled sides are no multiple of the tile: only cells on the plane are loaded, the stencil clamps its indices,
// stores are guarded.  Built with -ffp-contract=off: the roundings are the ones written here (tests/_lapref.py restates them).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 32768;

template <int P>
struct Tile;        // pooled cells per workgroup: fine tiles of 16 x 128 ... 128 x 256 pixels
template <>
struct Tile<1> {
    static constexpr int H = 16, W = 128;
};
template <>
struct Tile<2> {
    static constexpr int H = 16, W = 64;
};
template <>
struct Tile<4> {
    static constexpr int H = 16, W = 32;
};
template <>
struct Tile<8> {
    static constexpr int H = 16, W = 16;
};
template <>
struct Tile<16> {
    static constexpr int H = 8, W = 16;
};

// the grid is one-dimensional: block -> (plane, tile row, tile column)
__device__ __forceinline__ void tile_of(int tiles_y, int tiles_x, int &n, int &ty, int &tx) {
    const int b = blockIdx.x;
    tx = b % tiles_x;
    ty = (b / tiles_x) % tiles_y;
    n = b / (tiles_x * tiles_y);
}

// the 256 values of a workgroup folded by halving strides; the sum is in acc[0] afterwards
__device__ __forceinline__ void fold(double *acc) {
    __syncthreads();
    for (int stride = kThreads / 2; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride) acc[threadIdx.x] += acc[threadIdx.x + stride];
        __syncthreads();
    }
}

// D at cell (i, j) of the plane, read from an LDS array whose entry [a][b] holds cell (i0 - 1 + a, j0 - G + b)
template <int LW>
__device__ __forceinline__ float stencil(const float (*c)[LW], int i, int j, int i0, int j0, int G, int h, int w) {
    const int a = i - i0 + 1, b = j - j0 + G;
    const int au = max(i - 1, 0) - i0 + 1, ad = min(i + 1, h - 1) - i0 + 1;
    const int bl = max(j - 1, 0) - j0 + G, br = min(j + 1, w - 1) - j0 + G;
    return 4.f * c[a][b] - ((c[au][b] + c[ad][b]) + (c[a][bl] + c[a][br]));
}

// LOSS = false: out = D(pool(x)).  LOSS = true: r = D(pool(x)) - target, to out unless it is null, and the sum of r^2 of
// the tile to partials[block].  VEC: W % 4 == 0 and x 16-byte aligned.
template <int P, bool VEC, bool LOSS>
__global__ __launch_bounds__(kThreads) void lap_res_kernel(const float *__restrict__ x, const float *__restrict__ target, int H, int W,
                                                           float *__restrict__ out, double *__restrict__ partials, int tiles_y,
                                                           int tiles_x) {
    constexpr int TH = Tile<P>::H, TW = Tile<P>::W;
    constexpr int G = P >= 4 ? 1 : 4 / P;           // halo cells along W: whole float4 groups
    constexpr int LW = TW + 2 * G;
    constexpr float kInv = 1.f / (float)(P * P);
    __shared__ float rows[(TH + 2) * P][LW];        // [cell row * P + r][cell column]: the sum of row r of the cell's block
    __shared__ float cells[P > 1 ? TH + 2 : 1][LW];
    __shared__ double acc[LOSS ? kThreads : 1];
    int n, ty, tx;
    tile_of(tiles_y, tiles_x, n, ty, tx);
    const int h = H / P, w = W / P;
    const int i0 = ty * TH, j0 = tx * TW;
    const float *plane = x + (size_t)n * H * W;

    if (VEC) {
        // one item is one float4-aligned group of a fine row: a whole cell row (P >= 4) or 4 / P cells (P < 4)
        constexpr int GW = LW / G;
        for (int t = threadIdx.x; t < (TH + 2) * P * GW; t += kThreads) {
            const int fr = t / GW, g = t % GW;
            const int i = i0 - 1 + fr / P, j = j0 - G + g * G;
            if (i < 0 || i >= h || j < 0 || j >= w) continue;       // (w % G == 0: a group is on the plane or off it)
            const float4 *src = reinterpret_cast<const float4 *>(plane + (size_t)(i * P + fr % P) * W + (size_t)j * P);
            if (P >= 4) {
                float4 v = src[0];
                float s = ((v.x + v.y) + v.z) + v.w;
#pragma unroll
                for (int q = 1; q < P / 4; ++q) {
                    v = src[q];
                    s = (((s + v.x) + v.y) + v.z) + v.w;
                }
                rows[fr][g] = s;
            } else if (P == 2) {
                const float4 v = src[0];
                rows[fr][2 * g] = v.x + v.y;
                rows[fr][2 * g + 1] = v.z + v.w;
            } else {
                const float4 v = src[0];
                rows[fr][4 * g] = v.x;
                rows[fr][4 * g + 1] = v.y;
                rows[fr][4 * g + 2] = v.z;
                rows[fr][4 * g + 3] = v.w;
            }
        }
    } else {
        for (int t = threadIdx.x; t < (TH + 2) * P * LW; t += kThreads) {
            const int fr = t / LW, b = t % LW;
            const int i = i0 - 1 + fr / P, j = j0 - G + b;
            if (i < 0 || i >= h || j < 0 || j >= w) continue;
            const float *src = plane + (size_t)(i * P + fr % P) * W + (size_t)j * P;
            float s = src[0];
            for (int q = 1; q < P; ++q) s += src[q];
            rows[fr][b] = s;
        }
    }
    __syncthreads();
    if (P > 1) {
        for (int t = threadIdx.x; t < (TH + 2) * LW; t += kThreads) {
            const int a = t / LW, b = t % LW;
            const int i = i0 - 1 + a, j = j0 - G + b;
            if (i < 0 || i >= h || j < 0 || j >= w) continue;
            float s = rows[a * P][b];
            for (int r = 1; r < P; ++r) s += rows[a * P + r][b];
            cells[a][b] = s * kInv;
        }
        __syncthreads();
    }
    const float(*c)[LW] = P > 1 ? cells : rows;

    double sum = 0.0;
    for (int t = threadIdx.x; t < TH * TW; t += kThreads) {
        const int i = i0 + t / TW, j = j0 + t % TW;
        if (i >= h || j >= w) continue;
        const size_t at = ((size_t)n * h + i) * w + j;
        const float L = stencil<LW>(c, i, j, i0, j0, G, h, w);
        if (LOSS) {
            const float r = L - target[at];
            if (out != nullptr) out[at] = r;
            sum += (double)r * (double)r;
        } else {
            out[at] = L;
        }
    }
    if (LOSS) {
        acc[threadIdx.x] = sum;
        fold(acc);
        if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
    }
}

// grad(y, x) = k * D(r)(y / P, x / P) over the tile's fine pixels.  VEC: W % 4 == 0 and grad 16-byte aligned.
template <int P, bool VEC>
__global__ __launch_bounds__(kThreads) void lap_grad_kernel(const float *__restrict__ r, int H, int W, float k, float *__restrict__ grad,
                                                            int tiles_y, int tiles_x) {
    constexpr int TH = Tile<P>::H, TW = Tile<P>::W;
    constexpr int LW = TW + 2;
    __shared__ float res[TH + 2][LW];
    __shared__ float g[TH][TW];
    int n, ty, tx;
    tile_of(tiles_y, tiles_x, n, ty, tx);
    const int h = H / P, w = W / P;
    const int i0 = ty * TH, j0 = tx * TW;
    const float *plane = r + (size_t)n * h * w;

    for (int t = threadIdx.x; t < (TH + 2) * LW; t += kThreads) {
        const int i = i0 - 1 + t / LW, j = j0 - 1 + t % LW;
        if (i < 0 || i >= h || j < 0 || j >= w) continue;
        res[t / LW][t % LW] = plane[(size_t)i * w + j];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TH * TW; t += kThreads) {
        const int i = i0 + t / TW, j = j0 + t % TW;
        if (i >= h || j >= w) continue;
        g[t / TW][t % TW] = k * stencil<LW>(res, i, j, i0, j0, 1, h, w);
    }
    __syncthreads();
    float *gplane = grad + (size_t)n * H * W;
    constexpr int FW = TW * P;          // fine columns of the tile, a multiple of 4
    if (VEC) {
        for (int t = threadIdx.x; t < TH * P * (FW / 4); t += kThreads) {
            const int fy = t / (FW / 4), fx = 4 * (t % (FW / 4));
            const int y = i0 * P + fy, x0 = j0 * P + fx;
            if (y >= H || x0 >= W) continue;        // (W % 4 == 0: a quad is on the plane or off it)
            float4 v;
            if (P >= 4) {
                v.x = v.y = v.z = v.w = g[fy / P][fx / P];
            } else if (P == 2) {
                v.x = v.y = g[fy / 2][fx / 2];
                v.z = v.w = g[fy / 2][fx / 2 + 1];
            } else {
                v.x = g[fy][fx];
                v.y = g[fy][fx + 1];
                v.z = g[fy][fx + 2];
                v.w = g[fy][fx + 3];
            }
            *reinterpret_cast<float4 *>(gplane + (size_t)y * W + x0) = v;
        }
    } else {
        for (int t = threadIdx.x; t < TH * P * FW; t += kThreads) {
            const int fy = t / FW, fx = t % FW;
            const int y = i0 * P + fy, x0 = j0 * P + fx;
            if (y >= H || x0 >= W) continue;
            gplane[(size_t)y * W + x0] = g[fy / P][fx / P];
        }
    }
}

// loss = fp32(scale * sum of the partials): thread t adds partials t, t + 256, ... in ascending order, then the fold
__global__ __launch_bounds__(kThreads) void lap_finish_kernel(const double *__restrict__ partials, long blocks, double scale,
                                                              float *__restrict__ loss) {
    __shared__ double acc[kThreads];
    double s = 0.0;
    for (long b = threadIdx.x; b < blocks; b += kThreads) s += partials[b];
    acc[threadIdx.x] = s;
    fold(acc);
    if (threadIdx.x == 0) loss[0] = (float)(acc[0] * scale);
}

inline bool pool_ok(int p) { return p == 1 || p == 2 || p == 4 || p == 8 || p == 16; }

inline bool shape_ok(int N, int H, int W, int p) {
    return N > 0 && pool_ok(p) && H > 0 && W > 0 && H <= kMaxSide && W <= kMaxSide && H % p == 0 && W % p == 0 && H / p >= 2 && W / p >= 2;
}

inline void tile_cells(int p, int &th, int &tw) {
    switch (p) {
        case 1: th = Tile<1>::H, tw = Tile<1>::W; break;
        case 2: th = Tile<2>::H, tw = Tile<2>::W; break;
        case 4: th = Tile<4>::H, tw = Tile<4>::W; break;
        case 8: th = Tile<8>::H, tw = Tile<8>::W; break;
        default: th = Tile<16>::H, tw = Tile<16>::W; break;
    }
}

// tiles of all planes, or 0 when they do not fit the one-dimensional grid
inline long grid_blocks(int N, int H, int W, int p, int &tiles_y, int &tiles_x) {
    int th, tw;
    tile_cells(p, th, tw);
    tiles_y = st3d::cdiv(H / p, th);
    tiles_x = st3d::cdiv(W / p, tw);
    const long blocks = (long)N * tiles_y * tiles_x;
    return blocks <= 0x7fffffffL ? blocks : 0;
}

inline bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

inline size_t partial_bytes(long blocks) { return (size_t)blocks * sizeof(double); }

template <int P, bool LOSS>
void launch_res(const float *x, const float *target, int H, int W, float *out, double *partials, int tiles_y, int tiles_x, long blocks,
                hipStream_t s) {
    if (W % 4 == 0 && aligned16(x))
        lap_res_kernel<P, true, LOSS><<<(unsigned)blocks, kThreads, 0, s>>>(x, target, H, W, out, partials, tiles_y, tiles_x);
    else
        lap_res_kernel<P, false, LOSS><<<(unsigned)blocks, kThreads, 0, s>>>(x, target, H, W, out, partials, tiles_y, tiles_x);
}

template <int P>
void launch_grad(const float *r, int H, int W, float k, float *grad, int tiles_y, int tiles_x, long blocks, hipStream_t s) {
    if (W % 4 == 0 && aligned16(grad))
        lap_grad_kernel<P, true><<<(unsigned)blocks, kThreads, 0, s>>>(r, H, W, k, grad, tiles_y, tiles_x);
    else
        lap_grad_kernel<P, false><<<(unsigned)blocks, kThreads, 0, s>>>(r, H, W, k, grad, tiles_y, tiles_x);
}

#define LAP_DISPATCH(p, CALL)        \
    switch (p) {                     \
        case 1: CALL(1); break;      \
        case 2: CALL(2); break;      \
        case 4: CALL(4); break;      \
        case 8: CALL(8); break;      \
        default: CALL(16); break;    \
    }

}  // namespace

extern "C" int st3d_lap_tile(int p, int *tile_h, int *tile_w) {
    ST3D_CHECK_ARG(tile_h && tile_w);
    ST3D_CHECK_ARG(pool_ok(p));
    int th, tw;
    tile_cells(p, th, tw);
    *tile_h = th * p;
    *tile_w = tw * p;
    return ST3D_OK;
}

extern "C" size_t st3d_lap_workspace_bytes(int N, int H, int W, int p) {
    if (!shape_ok(N, H, W, p)) return 0;
    int tiles_y, tiles_x;
    const long blocks = grid_blocks(N, H, W, p, tiles_y, tiles_x);
    if (blocks <= 0) return 0;
    return partial_bytes(blocks) + (size_t)N * (H / p) * (W / p) * sizeof(float);
}

extern "C" int st3d_lap_fwd(const float *x, int N, int H, int W, int p, float *out, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && out && x != out);
    ST3D_CHECK_ARG(shape_ok(N, H, W, p));
    int tiles_y, tiles_x;
    const long blocks = grid_blocks(N, H, W, p, tiles_y, tiles_x);
    ST3D_CHECK_ARG(blocks > 0);
    const hipStream_t s = st3d::as_stream(stream);
#define CALL(P) launch_res<P, false>(x, nullptr, H, W, out, nullptr, tiles_y, tiles_x, blocks, s)
    LAP_DISPATCH(p, CALL)
#undef CALL
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_lap_loss(const float *x, const float *target, int N, int H, int W, int p, double scale, void *workspace,
                             size_t workspace_bytes, float *loss, float *grad, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && target && workspace && loss);
    ST3D_CHECK_ARG(x != target && x != grad && target != grad);
    ST3D_CHECK_ARG((const void *)x != workspace && (const void *)target != workspace && (void *)grad != workspace);
    ST3D_CHECK_ARG((void *)loss != workspace && loss != grad && loss != x && loss != target);
    ST3D_CHECK_ARG(shape_ok(N, H, W, p));
    ST3D_CHECK_ARG(std::isfinite(scale) && scale >= 0.0);
    ST3D_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
    int tiles_y, tiles_x;
    const long blocks = grid_blocks(N, H, W, p, tiles_y, tiles_x);
    ST3D_CHECK_ARG(blocks > 0);
    ST3D_CHECK_ARG(workspace_bytes >= st3d_lap_workspace_bytes(N, H, W, p));
    double *partials = static_cast<double *>(workspace);
    float *r = grad != nullptr ? reinterpret_cast<float *>(static_cast<char *>(workspace) + partial_bytes(blocks)) : nullptr;
    const float k = (float)(2.0 * scale / (double)(p * p));
    const hipStream_t s = st3d::as_stream(stream);
#define CALL(P) launch_res<P, true>(x, target, H, W, r, partials, tiles_y, tiles_x, blocks, s)
    LAP_DISPATCH(p, CALL)
#undef CALL
    ST3D_LAUNCH_CHECK();
    if (grad != nullptr) {
#define CALL(P) launch_grad<P>(r, H, W, k, grad, tiles_y, tiles_x, blocks, s)
        LAP_DISPATCH(p, CALL)
#undef CALL
        ST3D_LAUNCH_CHECK();
    }
    lap_finish_kernel<<<1, kThreads, 0, s>>>(partials, blocks, scale, loss);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
