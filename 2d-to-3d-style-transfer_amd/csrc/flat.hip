// flat.hip -- which output tiles of the shallow forward convs see more than the render's flat background.
//
// A hard render is texel-or-background: most pixels of a view hold one colour bit for bit.  A conv output tile whose input
// patch holds nothing but the field that colour produces computes the numbers every other such tile computes (one fixed
// operation order per in-tile position, conv.hip / wino43.hip) -- up to the distance to the image border, where the zero
// padding shows.  So such tiles are computed once per border class and copied (flat_fill_kernel); the forward launches of
// conv1_2 (S x S), conv2_1 and conv2_2 (S/2 x S/2) walk a list of the other tiles plus one representative per class.
//
//   V0 (N,S,S)      pixel differs from the colour in any channel, compared as bits (NaN is varying, -0 is not +0)
//   "varying" means: may differ from the flat field's value IN ANY BIT.  The direct conv1_1 maps V -> dilate(V, 1) (one fma
//   chain per pixel over its 3x3 window).  A Winograd F(4x4,3x3) conv computes a 4x4 output block from its 6x6 patch, and
//   every output of the block is rounded from sums over the WHOLE patch: a pixel whose own 3x3 window is flat but whose
//   block's patch is not comes out equal in value, not in bits (measured: conv2_2 tiles differed under the per-pixel rule).
//   So a Winograd conv maps V -> block4(dilate(V, 1)), the aligned 4x4 blocks that meet it; a 2x2 pool maps V -> the 2x2 OR.
//   A tile (a union of whole blocks) is varying iff its input patch (tile +- 1, clipped) meets the V of its input:
//     conv1_2 tile   meets dilate(V0, 2)                       = the tile's pooled pixels meet V2
//     V2 (N,S/2,S/2) = pool(block4(dilate(V0, 2))): the input of conv2_1 -- aligned 2x2 blocks of pooled pixels
//     conv2_1 tile   tile +- 1 meets V2
//     conv2_2 tile   tile +- 1 meets block4(dilate(V2, 1))    = tile +- 5 meets V2 (the blocks that touch tile +- 1 start
//                    at most 4 before it and end at most 4 behind it; tiles start and end on block borders)
//   class of a non-varying tile = (min(ty, D), min(TY - 1 - ty, D), min(tx, D), min(TX - 1 - tx, D)) with D = 2.  The field a
//   launch reads differs from its interior value only in a band along the image border: 1 pixel behind conv1_1; behind a
//   Winograd conv the first block, 4 pixels, so 2 behind pool1 and 4 behind conv2_1.  The patch of tile ty >= 2 starts at
//   row 2 rows - 1 >= 7 (rows >= 4; columns >= 32), past every such band, while tile 1's patch starts at row 3 and with
//   4-row tiles still reads conv2_1's band: D = 1 would not do for conv2_2.  So the first two and the last two tiles along
//   either axis are classes of their own and all others of one kind are one class (at most 5 x 5 = 25).
// A list = varying tiles + the lowest-indexed member (over the whole batch) of every class of non-varying tiles, ascending,
// in the launch's own tile numbering (st3d_wino43_tile_geometry); next to it the map tile -> representative (-1: listed).
// Four small launches (V0, V2, one flag per tile, one 1024-thread workgroup per list: ordered prefix-sum compaction as in
// need.hip; the class minimum is taken in LDS): no atomics to global memory, the same lists every time, nothing read back.
#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// one thread per 4 pixels of a row
__global__ __launch_bounds__(256) void flat_v0_kernel(const float *__restrict__ img, const float *__restrict__ color, int S,
                                                      int total4, uint8_t *__restrict__ v0) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int per = (S * S) >> 2;
    const int n = i / per, r = i - n * per;
    u32x4 d = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const u32x4 q = *reinterpret_cast<const u32x4 *>(img + ((size_t)(n * 3 + c) * per + r) * 4);
        d |= q ^ __float_as_uint(color[c]);
    }
    reinterpret_cast<unsigned *>(v0)[i] = (d[0] ? 1u : 0u) | (d[1] ? 0x100u : 0u) | (d[2] ? 0x10000u : 0u) | (d[3] ? 0x1000000u : 0u);
}

// one thread per 4 pooled pixels of a row = two aligned pairs: with yb = y / 2, xb = x / 2 (the 4x4 block of conv1_2's
// output the pooled pixel comes from), V2(y, x) = any V0 in rows 4 yb - 2 .. 4 yb + 5, columns 4 xb - 2 .. 4 xb + 5
__global__ __launch_bounds__(256) void flat_v2_kernel(const uint8_t *__restrict__ v0, int S, int total4, uint8_t *__restrict__ v2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int Sh = S >> 1, q4 = Sh >> 2;
    const int x4 = i % q4, y = (i / q4) % Sh, n = i / (q4 * Sh);
    const int c0 = 8 * x4;
    unsigned w[4] = {0u, 0u, 0u, 0u};          // bytes = columns c0 - 4 .. c0 + 11, OR-ed over the eight rows
#pragma unroll
    for (int dy = -2; dy <= 5; ++dy) {
        const int yy = 4 * (y >> 1) + dy;
        if (yy < 0 || yy >= S) continue;
        const uint8_t *row = v0 + ((size_t)n * S + yy) * S + c0;           // 8-byte aligned
        const u32x2 m = *reinterpret_cast<const u32x2 *>(row);
        w[1] |= m[0]; w[2] |= m[1];
        if (c0 > 0) w[0] |= *reinterpret_cast<const unsigned *>(row - 4);
        if (c0 + 8 < S) w[3] |= *reinterpret_cast<const unsigned *>(row + 8);
    }
    unsigned out = 0;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {           // pair pr: columns c0 + 4 pr - 2 .. c0 + 4 pr + 5 = bytes 4 pr + 2 .. 4 pr + 9
        unsigned any = 0;
#pragma unroll
        for (int k = 4 * pr + 2; k <= 4 * pr + 9; ++k) any |= (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        out |= (any ? 0x0101u : 0u) << (16 * pr);
    }
    reinterpret_cast<unsigned *>(v2)[i] = out;
}

struct FlatGeo {
    int tiles_x, tiles_y, rows, cols;      // a launch's output tiles: rows x cols pixels each
};

// one wave per tile of the three launches: flags[0 .. t1) conv1_2 (the tile's pooled pixels), [t1 .. t1 + t2) conv2_1
// (tile +- 1), [t1 + t2 .. t1 + 2 t2) conv2_2 (tile +- 5), all read from V2 and clipped to the map.  The lanes share the
// region's bytes (up to 18 x 74: independent loads, one vote at the end)
__global__ __launch_bounds__(256) void flat_flags_kernel(const uint8_t *__restrict__ v2, int S, FlatGeo g1, FlatGeo g2, int t1, int t2,
                                                         int total, uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= total) return;                    // (the whole wave)
    const int Sh = S >> 1;
    const int launch = i < t1 ? 0 : (i < t1 + t2 ? 1 : 2);
    const FlatGeo g = launch == 0 ? FlatGeo{g1.tiles_x, g1.tiles_y, g1.rows >> 1, g1.cols >> 1} : g2;     // in V2 pixels
    const int t = launch == 0 ? i : (launch == 1 ? i - t1 : i - t1 - t2);
    const int per_img = g.tiles_x * g.tiles_y;
    const int n = t / per_img, r = t - n * per_img;
    const int ty = r / g.tiles_x, tx = r - ty * g.tiles_x;
    const int x0 = tx * g.cols, y0 = ty * g.rows;
    const int margin = launch == 0 ? 0 : (launch == 1 ? 1 : 5);
    const int ya = max(0, y0 - margin), yb = min(Sh - 1, y0 + g.rows - 1 + margin);
    const int xa = max(0, x0 - margin), xb = min(Sh - 1, x0 + g.cols - 1 + margin);
    const int w = xb - xa + 1, count = (yb - ya + 1) * w;
    const uint8_t *base = v2 + (size_t)n * Sh * Sh;
    unsigned any = 0;
    for (int k = lane; k < count; k += 64) {
        const int y = ya + k / w, x = xa + k % w;
        any |= base[(size_t)y * Sh + x];
    }
    const bool vary = __any(any != 0);
    if (lane == 0) flags[i] = vary ? 1 : 0;
}

struct FlatLists {
    int *list[3], *map[3];
};

// workgroup l builds the list and the map of launch l.  Thread t owns the run [t * per, (t + 1) * per) of tiles: the class
// minima first (an LDS minimum per class: the lowest index whatever the order; a thread asks only where its tile is below
// the minimum it sees, so the many tiles of the interior class do not queue up on one address), then the ordered compaction
// of varying-or-representative as in need_lists_kernel
__global__ __launch_bounds__(1024) void flat_lists_kernel(const uint8_t *__restrict__ flags, FlatGeo g1, FlatGeo g2, int t1, int t2,
                                                          FlatLists out, int *__restrict__ counts) {
    __shared__ int scan[1024];
    __shared__ int rep[81];
    const int launch = blockIdx.x, tid = threadIdx.x;
    const uint8_t *__restrict__ f = flags + (launch == 0 ? 0 : (launch == 1 ? t1 : t1 + t2));
    const FlatGeo g = launch == 0 ? g1 : g2;
    const int total = launch == 0 ? t1 : t2;
    int *__restrict__ list = out.list[launch];
    int *__restrict__ map = out.map[launch];
    const int per = (total + 1023) / 1024;
    const int lo = min(total, tid * per), hi = min(total, lo + per);
    // the run's tiles in order: (ty, tx) stepped, not divided out per tile
    struct Walk { int ty, tx; };
    const int r0 = lo % (g.tiles_x * g.tiles_y);
    const Walk w0{r0 / g.tiles_x, r0 % g.tiles_x};
    auto cls = [&](const Walk &w) {
        return ((min(w.ty, 2) * 3 + min(g.tiles_y - 1 - w.ty, 2)) * 3 + min(w.tx, 2)) * 3 + min(g.tiles_x - 1 - w.tx, 2);
    };
    auto step = [&](Walk &w) {
        if (++w.tx == g.tiles_x) { w.tx = 0; if (++w.ty == g.tiles_y) w.ty = 0; }
    };
    // the run's flags, read once (bit k = tile lo + k; runs longer than 64 tiles re-read them)
    unsigned long long fm = 0;
    if (per <= 64)
        for (int t = lo; t < hi; ++t) fm |= (unsigned long long)(f[t] ? 1 : 0) << (t - lo);
    auto varying = [&](int t) { return per <= 64 ? (int)((fm >> (t - lo)) & 1ull) : (int)f[t]; };
    if (tid < 81) rep[tid] = 0x7fffffff;
    __syncthreads();
    Walk w = w0;
    for (int t = lo; t < hi; ++t, step(w)) {
        const int c = cls(w);
        if (!varying(t) && t < *(volatile int *)&rep[c]) atomicMin(&rep[c], t);      // (a stale read only costs an atomic)
    }
    __syncthreads();
    int cnt = 0;
    w = w0;
    for (int t = lo; t < hi; ++t, step(w)) cnt += (varying(t) || rep[cls(w)] == t) ? 1 : 0;
    scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int o = scan[tid] - cnt;
    w = w0;
    for (int t = lo; t < hi; ++t, step(w)) {
        const int rp = rep[cls(w)];
        const bool listed = varying(t) || rp == t;
        if (listed) list[o++] = t;
        map[t] = listed ? -1 : rp;
    }
    if (tid == 1023) counts[launch] = scan[1023];
}

// 16-byte chunk k of a (16 channels x br rows x bc elements of esize bytes) block: tile (tn, ty, tx) <- tile (rn, ry, rx)
struct FillTile { int n, y, x; };
__device__ __forceinline__ void fill_block(char *__restrict__ base, int esize, int C, int c0, int Hh, int Ww, int br, int bc,
                                           FillTile dst, FillTile src, int tid) {
    const int row_chunks = (bc * esize) >> 4;
    const int chunks = 16 * br * row_chunks;
    for (int k = tid; k < chunks; k += 256) {
        const int q = k % row_chunks, r = (k / row_chunks) % br, c = c0 + k / (row_chunks * br);
        const size_t so = ((((size_t)src.n * C + c) * Hh + src.y * br + r) * Ww + src.x * bc) * esize + 16 * q;
        const size_t d_o = ((((size_t)dst.n * C + c) * Hh + dst.y * br + r) * Ww + dst.x * bc) * esize + 16 * q;
        *reinterpret_cast<u32x4 *>(base + d_o) = *reinterpret_cast<const u32x4 *>(base + so);
    }
}

// workgroup (tile, group of 16 channels): an unlisted tile takes its representative's output block -- the full-resolution
// block, the pooled block and the argmax bytes, whichever the launch wrote.  Every row of a block is a multiple of 16 bytes
// (64 or 32 pixels; pooled 32 or 16; argmax 32 or 16 bytes) at a multiple of its own length: 16-byte accesses throughout.
__global__ __launch_bounds__(256) void flat_fill_kernel(const int *__restrict__ map, float *__restrict__ y, float *__restrict__ yp,
                                                        uint8_t *__restrict__ yidx, int C, int H, int W, FlatGeo g, int total) {
    const int t = blockIdx.x;
    const int rp = map[t];
    if (rp < 0 || rp >= total) return;         // a listed tile: the conv launch wrote it
    const int per_img = g.tiles_x * g.tiles_y;
    const int tr = t % per_img, rr = rp % per_img;
    const FillTile dst{t / per_img, tr / g.tiles_x, tr % g.tiles_x}, src{rp / per_img, rr / g.tiles_x, rr % g.tiles_x};
    const int c0 = blockIdx.y * 16, tid = threadIdx.x;
    if (y) fill_block(reinterpret_cast<char *>(y), 4, C, c0, H, W, g.rows, g.cols, dst, src, tid);
    if (yp) fill_block(reinterpret_cast<char *>(yp), 4, C, c0, H >> 1, W >> 1, g.rows >> 1, g.cols >> 1, dst, src, tid);
    if (yidx) fill_block(reinterpret_cast<char *>(yidx), 1, C, c0, H >> 1, W >> 1, g.rows >> 1, g.cols >> 1, dst, src, tid);
}

int geo_of(int H, int W, FlatGeo *g) {
    int rows = 0, cols = 0;
    if (!st3d_wino43_tile_geometry(H, W, &rows, &cols)) return 0;
    *g = FlatGeo{W / cols, H / rows, rows, cols};
    return 1;
}

}  // namespace

// S % 64 == 0: 4 x 64 tiles at S, 4 x 64 or 8 x 32 at S/2 (S/2 is a multiple of 32 and of 8)
extern "C" int st3d_flat_levels(int S) { return (S >= 64 && (S % 64) == 0) ? 3 : 0; }

extern "C" int st3d_flat_tiles(int N, int S, int launch) {
    FlatGeo g;
    if (N <= 0 || st3d_flat_levels(S) == 0 || launch < 0 || launch > 2) return 0;
    const int R = launch == 0 ? S : S / 2;
    if (!geo_of(R, R, &g)) return 0;
    return N * g.tiles_x * g.tiles_y;
}

extern "C" size_t st3d_flat_workspace_bytes(int N, int S) {
    if (N <= 0 || st3d_flat_levels(S) == 0) return 0;
    return (size_t)N * S * S + (size_t)N * (S / 2) * (S / 2) + (size_t)st3d_flat_tiles(N, S, 0) + 2 * (size_t)st3d_flat_tiles(N, S, 1);
}

// V2, the flags and the lists from a V0 plane (N,S,S bytes, non-zero = varying; 8-byte aligned rows)
static int build_from_v0(const uint8_t *v0, int N, int S, int levels, void *workspace, int *list1, int *map1, int *list2, int *map2,
                         int *list3, int *map3, int *counts, hipStream_t s) {
    FlatGeo g1, g2;
    geo_of(S, S, &g1);
    geo_of(S / 2, S / 2, &g2);
    const int t1 = N * g1.tiles_x * g1.tiles_y, t2 = N * g2.tiles_x * g2.tiles_y;
    uint8_t *v2 = reinterpret_cast<uint8_t *>(workspace) + (size_t)N * S * S;
    uint8_t *flags = v2 + (size_t)N * (S / 2) * (S / 2);
    const int n2 = N * (S / 2) * (S / 2) / 4;
    flat_v2_kernel<<<st3d::cdiv(n2, 256), 256, 0, s>>>(v0, S, n2, v2);
    ST3D_LAUNCH_CHECK();
    const int total = t1 + (levels - 1) * t2;
    flat_flags_kernel<<<st3d::cdiv(total, 4), 256, 0, s>>>(v2, S, g1, g2, t1, t2, total, flags);
    ST3D_LAUNCH_CHECK();
    FlatLists out{{list1, list2, list3}, {map1, map2, map3}};
    flat_lists_kernel<<<levels, 1024, 0, s>>>(flags, g1, g2, t1, t2, out, counts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_flat_build(const float *imgs, const float *color, int N, int S, int levels, void *workspace, size_t workspace_bytes,
                               int *list1, int *map1, int *list2, int *map2, int *list3, int *map3, int *counts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(imgs && color && workspace && counts && N > 0);
    ST3D_CHECK_ARG(levels >= 1 && levels <= st3d_flat_levels(S));
    ST3D_CHECK_ARG(((uintptr_t)imgs & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_flat_workspace_bytes(N, S));
    ST3D_CHECK_ARG(list1 && map1 && (levels < 2 || (list2 && map2)) && (levels < 3 || (list3 && map3)));
    hipStream_t s = st3d::as_stream(stream);
    uint8_t *v0 = reinterpret_cast<uint8_t *>(workspace);
    const int n0 = N * S * S / 4;
    flat_v0_kernel<<<st3d::cdiv(n0, 256), 256, 0, s>>>(imgs, color, S, n0, v0);
    ST3D_LAUNCH_CHECK();
    return build_from_v0(v0, N, S, levels, workspace, list1, map1, list2, map2, list3, map3, counts, s);
}

// The lists of st3d_flat_build with V0 taken from a coverage mask instead of the pixels: covered = varying.  They depend on
// the geometry alone, so a caller whose views do not move builds them once; they list a superset of the pixel lists' tiles
// as long as every uncovered pixel holds the colour bit for bit -- the caller's premise (st3d_flat_check_cover tests it).
extern "C" int st3d_flat_build_cover(const uint8_t *cover, int N, int S, int levels, void *workspace, size_t workspace_bytes, int *list1,
                                     int *map1, int *list2, int *map2, int *list3, int *map3, int *counts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(cover && workspace && counts && N > 0);
    ST3D_CHECK_ARG(levels >= 1 && levels <= st3d_flat_levels(S));
    ST3D_CHECK_ARG(((uintptr_t)cover & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_flat_workspace_bytes(N, S));
    ST3D_CHECK_ARG(list1 && map1 && (levels < 2 || (list2 && map2)) && (levels < 3 || (list3 && map3)));
    return build_from_v0(cover, N, S, levels, workspace, list1, map1, list2, map2, list3, map3, counts, st3d::as_stream(stream));
}

namespace {
// one thread per 4 pixels: *bad = 1 where a pixel varies (V0 of the pixels) and the mask does not cover it
__global__ __launch_bounds__(256) void flat_subset_kernel(const uint8_t *__restrict__ v0, const uint8_t *__restrict__ cover, int total4,
                                                          int *__restrict__ bad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const unsigned v = reinterpret_cast<const unsigned *>(v0)[i], c = reinterpret_cast<const unsigned *>(cover)[i];
    bool out = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) out |= ((v >> (8 * k)) & 0xffu) != 0 && ((c >> (8 * k)) & 0xffu) == 0;
    if (out) *bad = 1;              // (every writer writes the same value)
}
}  // namespace

// The premise of st3d_flat_build_cover, tested: *bad (device int) = 1 if any pixel of imgs differs from color outside cover,
// else 0.  Uses the V0 plane of the workspace (which st3d_flat_build_cover leaves alone).
extern "C" int st3d_flat_check_cover(const float *imgs, const float *color, const uint8_t *cover, int N, int S, void *workspace,
                                     size_t workspace_bytes, int *bad, st3d_stream_t stream) {
    ST3D_CHECK_ARG(imgs && color && cover && workspace && bad && N > 0 && st3d_flat_levels(S) > 0);
    ST3D_CHECK_ARG(((uintptr_t)imgs & 15) == 0 && ((uintptr_t)cover & 15) == 0 && ((uintptr_t)workspace & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_flat_workspace_bytes(N, S));
    hipStream_t s = st3d::as_stream(stream);
    uint8_t *v0 = reinterpret_cast<uint8_t *>(workspace);
    const int n0 = N * S * S / 4;
    ST3D_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    flat_v0_kernel<<<st3d::cdiv(n0, 256), 256, 0, s>>>(imgs, color, S, n0, v0);
    ST3D_LAUNCH_CHECK();
    flat_subset_kernel<<<st3d::cdiv(n0, 256), 256, 0, s>>>(v0, cover, n0, bad);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_flat_fill(const int *tile_map, float *y, float *y_pooled, uint8_t *pool_idx, int N, int C, int H, int W,
                              st3d_stream_t stream) {
    ST3D_CHECK_ARG(tile_map && (y || y_pooled) && (!pool_idx || y_pooled));
    ST3D_CHECK_ARG(N > 0 && C > 0 && (C % 16) == 0);
    ST3D_CHECK_ARG((((uintptr_t)y | (uintptr_t)y_pooled | (uintptr_t)pool_idx) & 15) == 0);
    FlatGeo g;
    ST3D_CHECK_ARG(geo_of(H, W, &g));
    const long total = (long)N * g.tiles_x * g.tiles_y;
    ST3D_CHECK_ARG(total < (1L << 31) && C / 16 < 65536);
    flat_fill_kernel<<<dim3((unsigned)total, (unsigned)(C / 16)), 256, 0, st3d::as_stream(stream)>>>(tile_map, y, y_pooled, pool_idx, C, H,
                                                                                                  W, g, (int)total);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
