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
//
// PER BLOCK (st3d_need_blocks_build).  The rule above hands a whole listed tile, dilated, to the level above, so every level
// grows by a tile.  An F(4x4,3x3) launch computes each aligned 4x4 output block from that block's own 6x6 input patch and
// from nothing else, so need travels per block instead: with need_k the pixels at which the output of list k's launch is
// needed (need_0 = dilate(mask, 1): the relu1_1 pass),
//     B_k = block4(need_k)                          the blocks that have to be right
//     list k = the tiles of the launch's geometry (4 x 64 or 8 x 32 pixels: 1 x 16 or 2 x 8 blocks) that hold one of B_k
//     need_k+1 = dilate(B_k, 1), clipped to the map; through the 2x2 OR where launch k un-pools its input
// An unneeded block of a listed tile may read input nobody wrote and write garbage; no needed block reads that garbage.
// On block bitmaps: B_k+1 = the 3x3 block neighbourhood OR of B_k (same resolution) or, through the un-pool, the OR over
// block rows / columns 2b - 1 .. 2b + 2.  Lists 0 .. 5 = the input gradients of conv1_2, conv2_1, conv2_2, conv3_1, conv3_2,
// conv3_3; conv1_2 and conv2_2 un-pool.  The maps are bit rows, one 64-bit word per 64 blocks of a row, so the ORs are shifts.  Two
// launches: the front one writes the segment map and B_0 (one lane per block, straight from the mask, the wave's ballot is
// the word); then one workgroup per list walks the levels up to its own in LDS, one thread per word, takes each tile's flag
// from the words and compacts as above.
//
// PER STRIP (tile_cols[k] = 16).  The F(4x4,3x3) kernel's four-row geometry gives every tile row of a workgroup step an origin of
// its own (wino43.hip, STRIPS), so list k names strips of 1 x 4 blocks (4 x 16 pixels), (n * strips_y + sy) * strips_x + sx, four
// entries to a step: the strips that hold a block of B_k, ascending within an image, each image padded with -1 to whole steps
// (a step's strips share their image's buffer descriptors), the count in steps.  Need propagation is the same.
#include "common.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void need_segment(const uint8_t *__restrict__ mask, int S, int i, uint8_t *__restrict__ seg) {
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

__global__ __launch_bounds__(256) void need_segments_kernel(const uint8_t *__restrict__ mask, int S, int total,
                                                            uint8_t *__restrict__ seg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < total) need_segment(mask, S, i, seg);
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

constexpr int kLists = ST3D_NEED_MAX_LISTS;
constexpr int kListShift[kLists] = {0, 1, 1, 2, 2, 2};       // the map of list k is (S >> shift)^2
constexpr int kListUnpools[kLists] = {1, 0, 1, 0, 0, 0};     // launch k reads its input through a 2x2 un-pool

struct BlockLevels {
    int nlists;
    int first;                       // workgroup 0 makes list `first` (the kept lists start above the flat-field levels)
    int bw[kLists];                  // blocks per row (and per column) of the map
    int trows[kLists], tcols[kLists];        // a tile in blocks: 1 x 16 or 2 x 8; 1 x 4 = strips, four entries to a step
    int unpools[kLists];
    int N;                           // images
    int total[kLists + 1];           // tiles of list k (all images), then the Gram runs
    int *list[kLists];
    // the Gram backward at relu2_1 (gram.hip): the 64-pixel runs of the (S/2)^2 map that meet need_2 = dilate(B_1, 1), numbered
    // image * runs + run (gram_runs per image, 0 = not asked for), compacted by one more workgroup
    int gram_runs;
    int *gram_list, *gram_count;
};

typedef unsigned long long u64;

// A block map is kept as bit rows: row r = words [r * W, (r + 1) * W), W = ceil(bw / 64), bit i of word j = block column
// 64 j + i; the bits past column bw - 1 are 0.
__device__ __forceinline__ int row_words(int bw) { return (bw + 63) >> 6; }
__device__ __forceinline__ u64 row_tail_mask(int bw, int j) {      // the columns of word j that are inside the map
    const int left = bw - 64 * j;
    return left >= 64 ? ~0ull : (1ull << left) - 1ull;
}

// The front launch: the first seg_wgs workgroups write the segment map (one thread per segment), the others B_0, one lane
// per block and one wave per word: the block is needed when its 6x6 patch (rows / columns 4 b - 1 .. 4 b + 4) holds a mask
// pixel.  Rows and columns past the edge are clamped back INTO the patch, so the 18 loads are unconditional and go out
// together; the wave's ballot is the word.
__global__ __launch_bounds__(256) void need_front_kernel(const uint8_t *__restrict__ mask, int S, int seg_total, int seg_wgs,
                                                         uint8_t *__restrict__ seg, int b0_words, u64 *__restrict__ b0) {
    if ((int)blockIdx.x < seg_wgs) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < seg_total) need_segment(mask, S, i, seg);
        return;
    }
    const int word = (blockIdx.x - seg_wgs) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (word >= b0_words) return;                    // (the whole wave)
    const int bw = S >> 2, W = row_words(bw);
    const int j = word % W, by = (word / W) % bw, n = word / (W * bw);
    const int bx = 64 * j + lane;
    unsigned any = 0;
    if (bx < bw) {
        const uint8_t *m = mask + (size_t)n * S * S + 4 * bx;            // 4-byte aligned: S % 64 == 0, the mask 16-byte aligned
        const int left = bx > 0 ? -1 : 0, right = bx + 1 < bw ? 4 : 3;
#pragma unroll
        for (int r = -1; r <= 4; ++r) {
            const uint8_t *row = m + (size_t)min(max(4 * by + r, 0), S - 1) * S;
            any |= *reinterpret_cast<const unsigned *>(row) | row[left] | row[right];
        }
    }
    const u64 bits = __ballot(any != 0);
    if (lane == 0) b0[word] = bits;
}

// The front launch of the kept lists (st3d_kept_build): K_0 = block4(dilate(cover, 2)), one lane per block and one wave per
// word as above.  The block may change when its 8x8 patch (rows / columns 4 b - 2 .. 4 b + 5: the 6x6 input patch of the
// F(4x4,3x3) block, each pixel of it the output of a 3x3 direct conv) holds a covered pixel.  Clamped like the patch above.
__global__ __launch_bounds__(256) void kept_front_kernel(const uint8_t *__restrict__ cover, int S, int k0_words, u64 *__restrict__ k0) {
    const int word = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (word >= k0_words) return;                    // (the whole wave)
    const int bw = S >> 2, W = row_words(bw);
    const int j = word % W, by = (word / W) % bw, n = word / (W * bw);
    const int bx = 64 * j + lane;
    unsigned any = 0;
    if (bx < bw) {
        const uint8_t *m = cover + (size_t)n * S * S + 4 * bx;
        const int l2 = bx > 0 ? -2 : 0, l1 = bx > 0 ? -1 : 0, r1 = bx + 1 < bw ? 4 : 3, r2 = bx + 1 < bw ? 5 : 3;
#pragma unroll
        for (int r = -2; r <= 5; ++r) {
            const uint8_t *row = m + (size_t)min(max(4 * by + r, 0), S - 1) * S;
            any |= *reinterpret_cast<const unsigned *>(row) | row[l2] | row[l1] | row[r1] | row[r2];
        }
    }
    const u64 bits = __ballot(any != 0);
    if (lane == 0) k0[word] = bits;
}

// every second bit of x (bits 0, 2, .. 62) packed into the low half
__device__ __forceinline__ u64 even_bits(u64 x) {
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
    x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
    x = (x | (x >> 16)) & 0x00000000ffffffffull;
    return x;
}

// OR of word j of the ROWS rows from ra on (those inside 0 .. bw - 1); 0 for a word outside the row.  Row and word are
// clamped into the map and the value dropped afterwards, so the loads do not wait for each other.
template <int ROWS>
__device__ __forceinline__ u64 rows_or(const u64 *__restrict__ m, int bw, int W, int ra, int j) {
    const int jc = min(max(j, 0), W - 1);
    u64 v = 0;
#pragma unroll
    for (int d = 0; d < ROWS; ++d) {
        const int r = ra + d;
        const u64 x = m[min(max(r, 0), bw - 1) * W + jc];
        v |= (r >= 0 && r < bw) ? x : 0ull;
    }
    return (j >= 0 && j < W) ? v : 0ull;
}

// does row `row` hold a block in columns xa .. xb (inside the map, xb - xa < 64)
__device__ __forceinline__ bool cols_any(const u64 *__restrict__ row, int xa, int xb) {
    const int j = xa >> 6, sh = xa & 63, n = xb - xa + 1;
    u64 v = row[j] >> sh;
    if (sh + n > 64) v |= row[j + 1] << (64 - sh);           // (xb is inside the map, so word j + 1 exists)
    return (v & (n >= 64 ? ~0ull : (1ull << n) - 1ull)) != 0;
}

// word j2 of row by of B_k+1 from B_k (cur: bw rows of W words): the 3x3 OR is the OR of three rows, then of the word with
// itself shifted by one either way, the neighbouring words lending the bit that crosses; through the un-pool (up), four
// rows, shifts -1, +1, +2 and every second bit
__device__ __forceinline__ u64 next_level_word(const u64 *__restrict__ cur, int bw, int W, int up, int bw2, int by, int j2) {
    u64 out;
    if (up) {
        u64 g[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = 2 * j2 + h;
            const u64 lo = rows_or<4>(cur, bw, W, 2 * by - 1, j - 1), v = rows_or<4>(cur, bw, W, 2 * by - 1, j);
            const u64 hi = rows_or<4>(cur, bw, W, 2 * by - 1, j + 1);
            g[h] = v | (v << 1) | (lo >> 63) | (v >> 1) | (hi << 63) | (v >> 2) | (hi << 62);
        }
        out = even_bits(g[0]) | (even_bits(g[1]) << 32);
    } else {
        const u64 lo = rows_or<3>(cur, bw, W, by - 1, j2 - 1), v = rows_or<3>(cur, bw, W, by - 1, j2);
        const u64 hi = rows_or<3>(cur, bw, W, by - 1, j2 + 1);
        out = v | (v << 1) | (lo >> 63) | (v >> 1) | (hi << 63);
    }
    return out & row_tail_mask(bw2, j2);
}

// does tile (ty, tx) of image n (of the chunk) hold a block of B_k (maps: bw rows of W words per image; a tile is tr x tc blocks)
__device__ __forceinline__ bool tile_flag(const u64 *__restrict__ maps, int bw, int W, int tr, int tc, int n, int ty, int tx) {
    const u64 *rows = maps + (n * bw + ty * tr) * W;
    bool any = cols_any(rows, tx * tc, tx * tc + tc - 1);
    if (tr == 2) any = cols_any(rows + W, tx * tc, tx * tc + tc - 1) || any;
    return any;
}

// does run (y, sx) of image n meet dilate(B_k, 1): a run is a row segment, rows y - 1 .. y + 1, columns 64 sx - 1 .. 64 sx + 64
// of the map, in blocks 16 sx - 1 .. 16 sx + 16 of at most two block rows
__device__ __forceinline__ bool run_flag(const u64 *__restrict__ maps, int bw, int W, int n, int y, int sx) {
    const int ya = max(0, y - 1) >> 2, yb = min(4 * bw - 1, y + 1) >> 2;
    const int xa = max(0, 16 * sx - 1), xb = min(bw - 1, 16 * sx + 16);
    const u64 *rows = maps + n * bw * W;
    return cols_any(rows + ya * W, xa, xb) || cols_any(rows + yb * W, xa, xb);
}

constexpr int kMapWords = 4096;      // LDS: B_even of a chunk of images; B_odd has at most half the words (kMapWords / 2)
constexpr int kMaxMapWords = 896;    // one image's B_0 at the largest side blocks_fit admits (896: 224 rows x 4 words)

// Workgroup k makes list k, the workgroup behind the lists' own the Gram runs (from B_1), each from B_0 on its own: for a chunk of
// images at a time (as many as kMapWords holds) it walks the levels up to its own in LDS, one thread per word, then thread t
// owns the items [t * per, (t + 1) * per) of the chunk, takes their flags from the bit rows, counts, an ordered scan over the
// 1024 counts (shuffles inside a wave, the 16 wave sums through LDS) gives its offset behind what the chunks before listed,
// and it writes its items in order: no atomics, the same list every time.  (The levels below its own are computed by every
// workgroup that needs them: a few hundred words each, against a launch and a round trip through memory.)
__global__ __launch_bounds__(1024) void need_block_lists_kernel(const u64 *__restrict__ b0, BlockLevels L, int *__restrict__ counts) {
    __shared__ u64 map_even[kMapWords], map_odd[kMapWords / 2];
    __shared__ int wave_sum[16];
    __shared__ int img_first[kMapWords / 16 + 2];        // strips: per image of the chunk, the strips listed before its first
    const int k = blockIdx.x + L.first, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool gram = k == L.nlists;
    int *__restrict__ list = gram ? L.gram_list : L.list[k];
    const int level = gram ? 1 : k;
    const int words0 = L.bw[0] * row_words(L.bw[0]), chunk = kMapWords / words0;
    // the items of an image: rows x cols tiles, or runs
    const int bwk = L.bw[level], Wk = row_words(bwk), tr = gram ? 0 : L.trows[k], tc = gram ? 0 : L.tcols[k];
    const int ncol = gram ? bwk / 16 : bwk / tc, nrow = gram ? 4 * bwk : bwk / tr, per_img = nrow * ncol;
    int listed = 0;
    for (int n0 = 0; n0 < L.N; n0 += chunk) {
        const int nc = min(chunk, L.N - n0);
        for (int i = tid; i < nc * words0; i += 1024) map_even[i] = b0[(size_t)n0 * words0 + i];
        __syncthreads();
        u64 *cur = map_even, *nxt = map_odd;
        for (int lv = 0; lv < level; ++lv) {
            const int bw = L.bw[lv], W = row_words(bw), up = L.unpools[lv];
            const int bw2 = up ? bw / 2 : bw, W2 = row_words(bw2), words2 = bw2 * W2;
            for (int w = tid; w < nc * words2; w += 1024) {
                const int n = w / words2, r = w - n * words2, by = r / W2, j2 = r - by * W2;
                nxt[w] = next_level_word(cur + n * bw * W, bw, W, up, bw2, by, j2);
            }
            __syncthreads();
            u64 *t = cur; cur = nxt; nxt = t;
        }
        const int total = nc * per_img, per = (total + 1023) / 1024;
        const int lo = min(total, tid * per), hi = min(total, lo + per);
        if (!gram && tc == 4) {
            // Strips: at most 16 items per word of B_0, 64 per thread.  The same ordered scan gives every listed strip its rank in
            // the chunk; the thread that owns an image's first item leaves the rank there in img_first, so an image's count is a
            // difference, its padded offset a sum over the images before it, and a strip goes to offset + rank within its image.
            int n = lo / per_img, row = (lo - n * per_img) / ncol, col = lo - n * per_img - row * ncol;
            u64 mask = 0;
            for (int i = 0; lo + i < hi; ++i) {
                mask |= (u64)(tile_flag(cur, bwk, Wk, 1, 4, n, row, col) ? 1 : 0) << i;
                if (++col == ncol) {
                    col = 0;
                    if (++row == nrow) { row = 0; ++n; }
                }
            }
            const int cnt = __popcll(mask);
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(incl, d);
                if (lane >= d) incl += v;
            }
            if (lane == 63) wave_sum[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const int v = wave_sum[w];
                before += w < wave ? v : 0;
                all += v;
            }
            const int rank0 = before + incl - cnt;       // listed strips of the chunk before this thread's items
            for (int m = (lo + per_img - 1) / per_img; m < nc && m * per_img < hi; ++m) {       // the images that start in [lo, hi)
                const int i = m * per_img - lo;
                img_first[m] = rank0 + __popcll(mask & ((1ull << i) - 1ull));       // (i < 64: the item is this thread's)
            }
            if (tid == 0) img_first[nc] = all;
            __syncthreads();
            // the padded offset of image m: whole steps of the images before it (nc <= 256: a short loop of independent reads)
            auto padded_before = [&](int m) {
                int o = 0;
                for (int j = 0; j < m; ++j) o += (img_first[j + 1] - img_first[j] + 3) & ~3;
                return o;
            };
            if (lo < hi) {
                int m = lo / per_img, base = listed + padded_before(m) - img_first[m], r = rank0, next = (m + 1) * per_img;
                for (int i = 0; lo + i < hi; ++i) {
                    if (lo + i == next) { ++m; base = listed + padded_before(m) - img_first[m]; next += per_img; }
                    if (mask >> i & 1ull) list[base + r++] = n0 * per_img + lo + i;
                }
            }
            if (tid < nc) {          // the voids behind image tid's last strip
                const int c = img_first[tid + 1] - img_first[tid], o = listed + padded_before(tid);
                for (int i = c; i < ((c + 3) & ~3); ++i) list[o + i] = -1;
            }
            listed += padded_before(nc);
            __syncthreads();                         // (the maps, wave_sum and img_first are the next chunk's)
            continue;
        }
        // (a chunk has at most 4 items per word of B_0, 16 per thread: the flags of a thread's items fit a mask, and the
        // items are walked by carrying (image, row, column) along instead of dividing each time)
        int n = lo / per_img, row = (lo - n * per_img) / ncol, col = lo - n * per_img - row * ncol;
        unsigned mask = 0;
        for (int i = 0; lo + i < hi; ++i) {
            const bool f = gram ? run_flag(cur, bwk, Wk, n, row, col) : tile_flag(cur, bwk, Wk, tr, tc, n, row, col);
            mask |= (f ? 1u : 0u) << i;
            if (++col == ncol) {
                col = 0;
                if (++row == nrow) { row = 0; ++n; }
            }
        }
        const int cnt = __popc(mask);
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int v = wave_sum[w];
            before += w < wave ? v : 0;
            all += v;
        }
        int o = listed + before + incl - cnt;
        for (int i = 0; lo + i < hi; ++i)
            if (mask >> i & 1u) list[o++] = n0 * per_img + lo + i;
        listed += all;
        __syncthreads();                             // (the maps and wave_sum are the next chunk's)
    }
    if (tid == 0) (gram ? L.gram_count : counts + k)[0] = (!gram && tc == 4) ? listed / 4 : listed;
}

// the sizes the per-block lists cover: one image's B_0 has to fit kMaxMapWords (b0_words(1, S), below; S <= 896)
bool blocks_fit(int S) {
    if (S <= 0 || (S % 64) != 0) return false;
    const size_t bw = (size_t)S / 4;
    return bw * ((bw + 63) / 64) <= (size_t)kMaxMapWords;
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

extern "C" int st3d_need_blocks_lists(int S) {
    if (!blocks_fit(S)) return 0;
    int k = 0;
    while (k < kLists && st3d_wino43_tile_geometry(S >> kListShift[k], S >> kListShift[k], nullptr, nullptr)) ++k;
    return k;
}

extern "C" size_t st3d_need_blocks_tiles(int N, int S, int k) {
    if (N <= 0 || k < 0 || k >= st3d_need_blocks_lists(S)) return 0;
    const size_t bw = (size_t)(S >> kListShift[k]) / 4;
    return (size_t)N * bw * bw / 16;         // 16 blocks per tile in either geometry
}

// the entries list k holds: its tiles, or four strips to each (tile_cols = 16: every image's strips fill whole steps, so the
// padded worst case is the full list)
extern "C" size_t st3d_need_blocks_entries(int N, int S, int k, int tile_cols) {
    return st3d_need_blocks_tiles(N, S, k) * (tile_cols == 16 ? 4 : 1);
}

extern "C" size_t st3d_need_blocks_gram_runs(int N, int S) {
    const int R = S / 2;
    if (N <= 0 || st3d_need_blocks_lists(S) < 2 || (R % 64) != 0) return 0;
    return (size_t)N * R * (R / 64);
}

// workspace: the bit rows of B_0, all images
static size_t b0_words(int N, int S) {
    const size_t bw = (size_t)S / 4;
    return (size_t)N * bw * ((bw + 63) / 64);
}

extern "C" size_t st3d_need_blocks_workspace_bytes(int N, int S) {
    if (N <= 0 || st3d_need_blocks_lists(S) == 0) return 0;
    return b0_words(N, S) * sizeof(u64);
}

// the levels of lists 0 .. nlists - 1 at side S; lists first .. nlists - 1 are made (and must be given)
static int fill_levels(BlockLevels *Lp, int N, int S, int first, int nlists, const int *tile_cols, int *const *lists) {
    BlockLevels &L = *Lp;
    memset(&L, 0, sizeof(L));
    L.nlists = nlists;
    L.first = first;
    L.N = N;
    for (int k = 0; k < nlists; ++k) {
        const int R = S >> kListShift[k];
        int rows = 0, cols = 0;
        st3d_wino43_tile_geometry(R, R, &rows, &cols);
        if (tile_cols && tile_cols[k]) cols = tile_cols[k];
        ST3D_CHECK_ARG(k < first || lists[k]);
        ST3D_CHECK_ARG((cols == 64 && R % 64 == 0) || (cols == 32 && R % 32 == 0) || cols == 16);      // (R % 8 == 0, R % 16 == 0 with it: S % 64 == 0)
        ST3D_CHECK_ARG(k < first || cols != 16 || ((uintptr_t)lists[k] & 15) == 0);
        L.bw[k] = R / 4;
        L.trows[k] = cols == 32 ? 2 : 1;
        L.tcols[k] = cols / 4;
        L.unpools[k] = kListUnpools[k];
        L.total[k] = (int)st3d_need_blocks_tiles(N, S, k);
        L.list[k] = k < first ? nullptr : lists[k];
    }
    return ST3D_OK;
}

extern "C" int st3d_need_blocks_build(const uint8_t *mask, int N, int S, int nlists, const int *tile_cols, uint8_t *seg,
                                      void *workspace, size_t workspace_bytes, int *const *lists, int *counts, int *gram_list,
                                      int *gram_count, st3d_stream_t stream) {
    ST3D_CHECK_ARG(mask && seg && N > 0);
    ST3D_CHECK_ARG(!gram_list || (gram_count && nlists >= 2 && st3d_need_blocks_gram_runs(N, S) > 0));
    ST3D_CHECK_ARG(nlists >= 1 && nlists <= st3d_need_blocks_lists(S));
    ST3D_CHECK_ARG(((uintptr_t)mask & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(lists && counts && workspace && workspace_bytes >= st3d_need_blocks_workspace_bytes(N, S));
    ST3D_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    BlockLevels L;
    ST3D_TRY(fill_levels(&L, N, S, 0, nlists, tile_cols, lists));
    if (gram_list) {
        L.gram_runs = (int)(st3d_need_blocks_gram_runs(N, S) / N);
        L.gram_list = gram_list;
        L.gram_count = gram_count;
    }
    L.total[nlists] = N * L.gram_runs;
    hipStream_t s = st3d::as_stream(stream);
    const int words = (int)b0_words(N, S);
    const int total = N * S * (S / 64), seg_wgs = st3d::cdiv(total, 256);
    u64 *bits = reinterpret_cast<u64 *>(workspace);
    need_front_kernel<<<seg_wgs + st3d::cdiv(words, 4), 256, 0, s>>>(mask, S, total, seg_wgs, seg, words, bits);
    ST3D_LAUNCH_CHECK();
    need_block_lists_kernel<<<nlists + (gram_list ? 1 : 0), 1024, 0, s>>>(bits, L, counts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

// The kept lists of the forward launches (plan.hip, forward()): list k is the forward of the conv whose input gradient need
// list k belongs to -- conv1_2, conv2_1, conv2_2, conv3_1, conv3_2, conv3_3 -- and holds the tiles or strips with an output
// block that may differ between two calls whose images differ on `cover` only:
//     K_0 = block4(dilate(cover, 2))            conv1_1 is per pixel, conv1_2 per block
//     K_k+1 = block4(dilate(K_k, 1)), through the 2x2 OR behind a fused pool
// which from K_0 on is the propagation of the need lists (next_level_word), so the second launch is theirs.  Lists first ..
// nlists - 1 are made, in the formats of st3d_need_blocks_build; counts[k] belongs to list k.
extern "C" int st3d_kept_build(const uint8_t *cover, int N, int S, int first, int nlists, const int *tile_cols, void *workspace,
                               size_t workspace_bytes, int *const *lists, int *counts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(cover && N > 0);
    ST3D_CHECK_ARG(first >= 0 && first < nlists && nlists <= st3d_need_blocks_lists(S));
    ST3D_CHECK_ARG(((uintptr_t)cover & 15) == 0);
    ST3D_CHECK_ARG((long)N * S * S < (1L << 31));
    ST3D_CHECK_ARG(lists && counts && workspace && workspace_bytes >= st3d_need_blocks_workspace_bytes(N, S));
    ST3D_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
    BlockLevels L;
    ST3D_TRY(fill_levels(&L, N, S, first, nlists, tile_cols, lists));
    hipStream_t s = st3d::as_stream(stream);
    const int words = (int)b0_words(N, S);
    u64 *bits = reinterpret_cast<u64 *>(workspace);
    kept_front_kernel<<<st3d::cdiv(words, 4), 256, 0, s>>>(cover, S, words, bits);
    ST3D_LAUNCH_CHECK();
    need_block_lists_kernel<<<nlists - first, 1024, 0, s>>>(bits, L, counts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
