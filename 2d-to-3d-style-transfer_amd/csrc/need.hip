// need.hip -- which parts of the VGG backward the image gradient's only consumer needs.
//
// The image gradient of the perceptual loss is read by the render backward, and that reads it only at pixels that have a
// fragment: mask (N,S,S), one byte per pixel.  From it, bottom-up, the units of the launches that can skip work:
//   level 0  the 64-pixel row segments of the relu1_1 pass (tap0.hip): the 27 tap planes are gathered over a 3x3 window,
//            so they are needed on dilate(mask, 1); seg (N,S,S/64) = 1 where a segment touches that
//   level 1  the output tiles of the conv1_2 input gradient (wino43.hip, 4 x 64 pixels at W % 64 == 0) that hold an
//            active segment
//   level 2  the output tiles of the conv2_1 input gradient (at S/2: 4 x 64 or 8 x 32 pixels): level 1 un-pools its
//            input, a tile reads the 1-pixel-dilated patch of its output, so the pooled pixels needed are the 2x2 OR of
//            dilate(union of the active level-1 tiles, 1), and a level-2 tile is active when it holds one of them
// Levels 1 and 2 leave as compact ascending lists of tile indices in the launch's own numbering ((n * tiles_y + ty) *
// tiles_x + tx) plus their counts, all in device memory: the host never reads them.  Three small launches: the segment
// map (one thread per segment), one flag per tile of either level (one thread per tile, straight from the segment map)
// and one 1024-thread workgroup per list (ordered prefix-sum compaction of the flags: no atomics, the same list every
// time).  At 8 x 512^2: 32768 segments, 8192 + 2048 tiles.
#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void need_segments_kernel(const uint8_t *__restrict__ mask, int S, int total,
                                                            uint8_t *__restrict__ seg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int segs = S >> 6;
    const int sx = i % segs, y = (i / segs) % S, n = i / (segs * S);
    const uint8_t *m = mask + (size_t)n * S * S;
    unsigned any = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= S) continue;
        const uint8_t *row = m + (size_t)yy * S + 64 * sx;       // 16-byte aligned: S % 64 == 0 and the mask is
        const u32x4 *q = reinterpret_cast<const u32x4 *>(row);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32x4 v = q[k];
            any |= v[0] | v[1] | v[2] | v[3];
        }
        if (sx > 0) any |= row[-1];
        if (sx + 1 < segs) any |= row[64];
    }
    seg[i] = any ? 1 : 0;
}

struct NeedGeo {
    int tiles_x, tiles_y, rows, cols;      // a launch's output tiles: rows x cols pixels each
};

// OR of the segment bytes of rows ya .. yb, segments sa .. sb of image n, all inside the image.  No early exit: the loads
// do not depend on each other and go out back to back.
__device__ __forceinline__ unsigned seg_block_any(const uint8_t *__restrict__ seg, int S, int n, int ya, int yb, int sa, int sb) {
    const int segs = S >> 6;
    unsigned any = 0;
    for (int y = ya; y <= yb; ++y) {
        const uint8_t *row = seg + ((size_t)n * S + y) * segs;
#pragma unroll 4
        for (int s = sa; s <= sb; ++s) any |= row[s];
    }
    return any;
}

// one thread per tile of either level: flags[0 .. total1) = level 1 (the tile holds an active segment), flags[total1 ..) =
// level 2 (pooled resolution): the tile's pixels, doubled, meet the 1-pixel-dilated extent of an active level-1 tile --
// level-1 tile t covers rows t * rows - 1 .. t * rows + rows once dilated, so the level-1 tiles in question form a
// rectangle, and so do their segments
__global__ __launch_bounds__(64) void need_flags_kernel(const uint8_t *__restrict__ seg, int N, int S, NeedGeo g1, NeedGeo g2,
                                                        int total1, int total2, uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= total1 + total2) return;
    const bool second = i >= total1;
    const NeedGeo g = second ? g2 : g1;
    const int t = second ? i - total1 : i;
    const int per_img = g.tiles_x * g.tiles_y;
    const int n = t / per_img, r = t - n * per_img;
    const int ty = r / g.tiles_x, tx = r - ty * g.tiles_x;
    int ta = ty, tb = ty, ua = tx, ub = tx;              // the level-1 tiles whose segments decide
    if (second) {
        const int y0 = 2 * ty * g2.rows, y1 = y0 + 2 * g2.rows - 1;        // full-resolution rows y0 .. y1
        const int x0 = 2 * tx * g2.cols, x1 = x0 + 2 * g2.cols - 1;
        ta = max(0, (y0 - 1) / g1.rows); tb = min(g1.tiles_y - 1, (y1 + 1) / g1.rows);
        ua = max(0, (x0 - 1) / g1.cols); ub = min(g1.tiles_x - 1, (x1 + 1) / g1.cols);
    }
    flags[i] = seg_block_any(seg, S, n, ta * g1.rows, tb * g1.rows + g1.rows - 1, (ua * g1.cols) >> 6,
                             (ub * g1.cols + g1.cols - 1) >> 6) ? 1 : 0;
}

// workgroup l compacts the flags of level l + 1: thread t owns the run [t * per, (t + 1) * per) of tiles, counts its active
// ones, an inclusive scan over the 1024 counts gives its offset, and it writes its run in order
__global__ __launch_bounds__(1024) void need_lists_kernel(const uint8_t *__restrict__ flags, int total1, int total2,
                                                          int *__restrict__ list1, int *__restrict__ list2,
                                                          int *__restrict__ counts) {
    __shared__ int scan[1024];
    const int level = blockIdx.x, tid = threadIdx.x;
    const uint8_t *__restrict__ f = level == 0 ? flags : flags + total1;
    int *__restrict__ list = level == 0 ? list1 : list2;
    const int total = level == 0 ? total1 : total2;
    const int per = (total + 1023) / 1024;
    const int lo = min(total, tid * per), hi = min(total, lo + per);
    int cnt = 0;
    for (int t = lo; t < hi; ++t) cnt += f[t];
    scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    int o = scan[tid] - cnt;
    for (int t = lo; t < hi; ++t)
        if (f[t]) list[o++] = t;
    if (tid == 1023) counts[level] = scan[1023];
}

int geo_of(int H, int W, NeedGeo *g) {
    int rows = 0, cols = 0;
    if (!st3d_wino43_tile_geometry(H, W, &rows, &cols)) return 0;
    *g = NeedGeo{W / cols, H / rows, rows, cols};
    return 1;
}

}  // namespace

extern "C" int st3d_need_levels(int S) {
    NeedGeo g;
    if (S <= 0 || (S % 64) != 0) return 0;
    if (!geo_of(S, S, &g)) return 1;
    if (!geo_of(S / 2, S / 2, &g)) return 2;
    return 3;
}

extern "C" size_t st3d_need_workspace_bytes(int N, int S) {
    NeedGeo g1, g2;
    size_t b = 0;
    if (N <= 0 || st3d_need_levels(S) < 2) return 0;
    geo_of(S, S, &g1);
    b = (size_t)N * g1.tiles_x * g1.tiles_y;
    if (geo_of(S / 2, S / 2, &g2)) b += (size_t)N * g2.tiles_x * g2.tiles_y;
    return b;
}

extern "C" int st3d_need_build(const uint8_t *mask, int N, int S, int levels, uint8_t *seg, void *workspace, size_t workspace_bytes,
                               int *list1, int *list2, int *counts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(mask && seg && N > 0);
    ST3D_CHECK_ARG(levels >= 1 && levels <= st3d_need_levels(S));
    ST3D_CHECK_ARG(((uintptr_t)mask & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(levels < 2 || (list1 && counts && workspace && workspace_bytes >= st3d_need_workspace_bytes(N, S)));
    ST3D_CHECK_ARG(levels < 3 || list2);
    hipStream_t s = st3d::as_stream(stream);
    const int total = N * S * (S / 64);
    need_segments_kernel<<<st3d::cdiv(total, 256), 256, 0, s>>>(mask, S, total, seg);
    ST3D_LAUNCH_CHECK();
    if (levels >= 2) {
        NeedGeo g1, g2;
        geo_of(S, S, &g1);
        g2 = g1;
        if (levels >= 3) geo_of(S / 2, S / 2, &g2);
        const int total1 = N * g1.tiles_x * g1.tiles_y, total2 = levels >= 3 ? N * g2.tiles_x * g2.tiles_y : 0;
        uint8_t *flags = reinterpret_cast<uint8_t *>(workspace);
        need_flags_kernel<<<st3d::cdiv(total1 + total2, 64), 64, 0, s>>>(seg, N, S, g1, g2, total1, total2, flags);
        ST3D_LAUNCH_CHECK();
        need_lists_kernel<<<levels - 1, 1024, 0, s>>>(flags, total1, total2, list1, list2, counts);
        ST3D_LAUNCH_CHECK();
    }
    return ST3D_OK;
}
