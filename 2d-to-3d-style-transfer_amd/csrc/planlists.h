// planlists.h -- what st3d_plan_create (plan.hip) decides about the plan's lists: how many need, flat-field and kept levels
// there are, the geometry each one walks, and what the two groups of a split call walk.  One pure function of the plan's
// size, the CU count, the route table, what the kernels say they cover and the environment's switches.  Plain C++ with no
// device call, so the stand-alone host test (tests/host/planlists_main.cpp) compiles it with the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/st3d.h"

namespace st3d {

// torchvision vgg19().features layout: module index -> kind
constexpr int kModules = 37;
constexpr int kConvIdx[16] = {0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34};
constexpr int kConvCin[16] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512};
constexpr int kConvCout[16] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512};
constexpr int kPoolIdx[5] = {4, 9, 18, 27, 36};

inline int conv_slot(int module_idx) {
    for (int i = 0; i < 16; ++i)
        if (kConvIdx[i] == module_idx) return i;
    return -1;
}
inline int pool_slot(int module_idx) {
    for (int i = 0; i < 5; ++i)
        if (kPoolIdx[i] == module_idx) return i;
    return -1;
}

// which kernel runs conv slot cs, per direction.  Every input is fixed when the plan is made -- the handle's switches, the
// packs that exist, the layer's channels, the plan's H and W -- so st3d_plan_create fills the table once and every launch
// site reads it; what a call adds is whether the arriving gradient is pooled or already gated
enum : uint8_t { DIRECT, WINO, WINO43 };      // conv.hip, wino.hip F(2x2,3x3), wino43.hip F(4x4,3x3)
struct Route {
    uint8_t fwd = DIRECT;
    bool dgrad_wino = false;    // the input gradient runs on wino.hip ...
    bool dgrad_w43 = false;     // ... and on wino43.hip when its gradient arrives already gated (all F(4x4,3x3) takes)
    // Producer-side ReLU gates (st3d_wino_dgrad_chain): whoever writes a gradient last zeroes it where its tensor's gate
    // is closed, so the Winograd input gradient that consumes it streams one operand per stage
    bool gate_taps = false;     // the style / content terms that join this conv's (unpooled) gradient gate it
    bool gate_dst = false;      // this launch gates the gradient it writes: the launch below is a Winograd one too
};

// ST3D_SPLIT_BATCH when the environment does not set it: SPLIT_FWD, the forward alone (measured, DESIGN.md 6: the
// backward's share cannot be told from the spread between boxes)
#define ST3D_SPLIT_BATCH_DEFAULT 1
enum { SPLIT_FWD = 1, SPLIT_BWD = 2 };
constexpr int kKeepFirst = 3, kKeepMax = 3;      // the kept lists proper: list 3 = conv slot 4 = conv3_1, up to conv3_3

// what the decisions rest on; plan.hip fills it in once.  List k belongs to conv slot k + 1 (conv1_2 .. conv3_3).
struct PlanFacts {
    int B = 0, S = 0, cus = 0;
    int H[16] = {};                 // map height (= width) per conv slot
    Route route[16];
    bool fused_tap0 = false;
    int need_levels = 0, blocks_lists = 0, flat_levels = 0;    // st3d_need_levels(S), st3d_need_blocks_lists(S), st3d_flat_levels(S)
    int geo_rows[ST3D_NEED_MAX_LISTS] = {}, geo_cols[ST3D_NEED_MAX_LISTS] = {};    // st3d_wino43_tile_geometry of list k's map
    bool gram_segs = false;         // st3d_gram_bwd_segs_supported at relu2_1
    size_t gram_runs = 0;           // st3d_need_blocks_gram_runs(B, S)
};

struct PlanDecisions {
    // Need lists of st3d_plan_loss_masked (need.hip).  A launch may only be thinned out when every launch below it is, so
    // the levels count from the bottom: 1 the relu1_1 pass, 2 + the conv1_2 input gradient, 3 + the conv2_1 input gradient
    // -- as many as the size has, the routes allow and ST3D_NEED_DEPTH leaves.  need_blocks: the lists are the per-block
    // ones (st3d_need_blocks_build; ST3D_NEED_BLOCKS=0: the tile-granular ones of st3d_need_build).  They stay thin further
    // up, so the levels go on: 4 + conv2_2, 5 + conv3_1, 6 + conv3_2, 7 + conv3_3, each in the geometry need_cols says
    // (64 / 32 pixels across, 16 = strips; 0 = the kernel's own choice for the map).
    int need_levels = 0;
    bool need_blocks = false;
    int need_cols[ST3D_NEED_MAX_LISTS] = {};
    // the Gram backward at relu2_1 over the 64-pixel runs the conv2_1 input gradient reads (level 3 and up; gram.hip)
    bool need_gram = false;
    // flat-field lists of st3d_plan_loss_flat (flat.hip): how many of conv1_2, conv2_1, conv2_2 run listed -- as many as
    // the size has, run F(4x4,3x3) and ST3D_FLAT_DEPTH leaves
    int flat_levels = 0;
    // Kept lists of st3d_plan_loss_keyed (st3d_kept_build, need.hip): how many of conv3_1, conv3_2, conv3_3 walk, in a call
    // that finds the clean record its own, only the tiles or strips holding an output block that the coverage can change.
    // Bottom-up like the levels above; keep_cols as need_cols (16 = strips).
    int keep_levels = 0;
    int keep_cols[ST3D_NEED_MAX_LISTS] = {};
    // The flat-field levels in such a call: no fill runs, so nothing needs their lists to name one tile per border class,
    // and conv1_2, conv2_1 and conv2_2 may walk their kept lists (lists 0 .. 2) in a finer geometry than the flat-field
    // lists' own.  shallow_cols[k]: 0 = the flat-field list as ever; 32 / 64 tiles, 16 strips (conv2_1 only: the others
    // pool).  keep_first: the lowest list the build makes (kKeepFirst when no shallow level is on).
    int shallow_cols[3] = {};
    int keep_first = kKeepFirst;
    // the split batch: SPLIT_FWD | SPLIT_BWD; and the two-rounds rule with a group's count: which kept lists a group walks,
    // how many need levels it lists
    int split_mode = 0;
    bool grp_kept_on[ST3D_NEED_MAX_LISTS] = {};
    int grp_need_levels = 0;
    bool grp_need_gram = false;
};

// The next value of a comma-separated geometry switch; `cur` walks the string from call to call.
//   ST3D_NEED_TILE (last_repeats): a value without a comma applies to every list.  With commas the caller asks once per
//     list for all six, whether or not the level engages, and the last value repeats.  Unset or empty: the default.  A
//     value of 0, one that does not fit, or the kernel's own geometry all end as need_cols = 0, the kernel's own choice.
//   ST3D_KEEP_TILE (last_repeats): the same, but the caller asks only for the levels its loop reaches -- it breaks at the
//     first level that fails.  0 = the kernel's own geometry (cols0); 16 always fits there.
//   ST3D_KEEP_SHALLOW (!last_repeats): after the last value the rest read as 0, which is off, and so does an empty
//     string; only unset gives the defaults.  16 fits only where the conv has no fused pool.  Considered only when
//     keep_levels >= 1, and an unfit level is skipped, not the end of the loop.
inline int next_cols(const char *&cur, int dflt, bool last_repeats) {
    if (!cur || (last_repeats && !cur[0])) return dflt;
    const int v = atoi(cur);
    if (const char *c = strchr(cur, ',')) cur = c + 1;
    else if (!last_repeats) cur = "";
    return v;
}

// ST3D_NEED_FORCE lifts the two-rounds rule of the need lists and the Gram runs, ST3D_KEEP_FORCE that of the kept and shallow
// lists and of grp_kept_on (tests reach every level at small sizes); neither lifts the other's.
inline PlanDecisions decide_lists(const PlanFacts &f, const char *(*env)(const char *)) {
    PlanDecisions d;
    const int B = f.B, hb = f.B / 2;
    const Route *route = f.route;
    auto flag = [&](const char *name, bool dflt) { const char *e = env(name); return e && e[0] ? e[0] != '0' : dflt; };
    // ST3D_NEED_DEPTH=k / ST3D_FLAT_DEPTH=k / ST3D_KEEP_DEPTH=k: at most k levels (A/B runs; the default is all of them:
    // each measured to pay); a value outside 0 <= k < levels changes nothing
    auto capped = [&](int levels, const char *name) {
        const char *e = env(name);
        return (e && atoi(e) >= 0 && atoi(e) < levels) ? atoi(e) : levels;
    };
    const bool need_force = flag("ST3D_NEED_FORCE", false), keep_force = flag("ST3D_KEEP_FORCE", false);
    // A list pays only where the full launch walks at least two tiles per persistent workgroup, N tiles_x tiles_y >=
    // 2 (CUs / n_ct): below that every workgroup has one tile at the most and a list saves nothing.  channels: the ones
    // that divide the CUs, Cin for an input gradient, Cout for a forward.
    auto two_rounds = [&](int images, int R, int channels) {
        return (long)images * (R / 4) * (R / 4) / 16 >= 2L * (f.cus / std::max(1, channels / 64));
    };
    // the same rule for the relu2_1 Gram backward listed: one workgroup per 64-pixel run, four to a CU
    auto gram_rounds = [&](int images) { return (long)images * (f.H[2] * f.H[2] / 64) >= 2L * 4 * f.cus; };
    // does a map R x R divide into tiles `cols` pixels across (64: 8 x 64, 32: 8 x 32; 16: strips, where the caller says)
    auto fits = [](int cols, int R, bool strips_ok) {
        return (cols == 64 && R % 64 == 0) || (cols == 32 && R % 32 == 0 && R % 8 == 0) || (cols == 16 && strips_ok);
    };
    auto pools = [](int cs) { return pool_slot(kConvIdx[cs] + 2) >= 0; };

    // ---- need: a listed conv1_2 / conv2_1 input gradient is an F(4x4,3x3) launch, so its gradient has to arrive gated
    int need_ok = f.fused_tap0 ? 1 : 0;
    if (need_ok == 1 && route[2].gate_dst && route[1].dgrad_w43) need_ok = 2;
    if (need_ok == 2 && route[2].dgrad_w43) need_ok = 3;
    int need_max = f.need_levels;
    d.need_blocks = need_ok >= 2 && f.blocks_lists >= 2 && flag("ST3D_NEED_BLOCKS", true);
    if (d.need_blocks) {
        // The per-block lists.  Level cs + 1 lists the input gradient of conv slot cs = list cs - 1.  A level above conv2_1, or
        // a geometry other than the kernel's own, engages only under the two-rounds rule.  conv2_2 and conv3_1 .. conv3_3:
        // F(4x4,3x3) launches whose gradient arrives gated (from the launch above, or the taps)
        need_max = 1 + f.blocks_lists;
        for (int cs = 3; cs <= ST3D_NEED_MAX_LISTS && need_ok == cs; ++cs)
            if (route[cs].dgrad_w43 && (cs == 4 ? route[cs].gate_taps : route[cs + 1].gate_dst) &&
                (need_force || two_rounds(B, f.H[cs], kConvCin[cs])))
                need_ok = cs + 1;
        // measured defaults: strips of 4 x 16 pixels on every level but conv3_1, which no geometry finer than
        // 8 x 32 tiles brings under its three rounds.  Strips fit every map the kernel covers.
        static const int kDefaultCols[ST3D_NEED_MAX_LISTS] = {16, 16, 16, 32, 16, 16};
        const char *tile = env("ST3D_NEED_TILE");
        for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) {
            const int R = f.H[k + 1], cols = next_cols(tile, kDefaultCols[k], true);
            const bool on = fits(cols, R, f.geo_rows[k] != 0) && cols != f.geo_cols[k] && (need_force || two_rounds(B, R, kConvCin[k + 1]));
            d.need_cols[k] = on ? cols : 0;
        }
    }
    d.need_levels = capped(std::min(need_ok, need_max), "ST3D_NEED_DEPTH");
    d.need_gram = d.need_blocks && d.need_levels >= 3 && flag("ST3D_NEED_GRAM", true) && route[2].gate_taps && f.gram_segs &&
                  f.gram_runs > 0 && (need_force || gram_rounds(B));

    // ---- flat
    int flat_ok = 0;
    while (flat_ok < 3 && route[flat_ok + 1].fwd == WINO43) ++flat_ok;
    d.flat_levels = capped(std::min(flat_ok, f.flat_levels), "ST3D_FLAT_DEPTH");

    // ---- kept: conv3_1 .. conv3_3 above a full set of flat-field levels, F(4x4,3x3) launches without a pool, under the
    // two-rounds rule with the forward's Cout.  Measured default: strips.
    int keep_ok = 0;
    const char *tile = env("ST3D_KEEP_TILE");
    while (d.flat_levels == 3 && keep_ok < kKeepMax) {
        const int k = kKeepFirst + keep_ok, cs = k + 1, R = f.H[cs];
        if (k >= f.blocks_lists || route[cs].fwd != WINO43 || pools(cs)) break;
        if (!keep_force && !two_rounds(B, R, kConvCout[cs])) break;
        int cols = next_cols(tile, 16, true);
        if (cols == 0) cols = f.geo_cols[k];
        if (!fits(cols, R, true)) break;
        d.keep_cols[k] = cols;
        ++keep_ok;
    }
    d.keep_levels = capped(keep_ok, "ST3D_KEEP_DEPTH");
    // ST3D_KEEP_SHALLOW = a,b,c: the geometry of conv1_2, conv2_1, conv2_2 in clean calls (0 = their flat-field lists);
    // measured default.  Only above a kept conv3_1, and under the same two-rounds rule.
    static const int kDefaultShallow[3] = {32, 16, 32};
    const char *sh = env("ST3D_KEEP_SHALLOW");
    for (int k = 0; k < 3 && d.keep_levels >= 1; ++k) {
        const int cs = k + 1, R = f.H[cs], cols = next_cols(sh, kDefaultShallow[k], false);
        if (!fits(cols, R, !pools(cs)) || (!keep_force && !two_rounds(B, R, kConvCout[cs]))) continue;
        d.shallow_cols[k] = cols;
        if (k < d.keep_first) d.keep_first = k;
    }
    for (int k = d.keep_first; k < 3; ++k) d.keep_cols[k] = d.shallow_cols[k] ? d.shallow_cols[k] : 16;     // (built, not walked)

    // ---- ST3D_SPLIT_BATCH = 0 | 1 | fwd | bwd: clean keyed calls as two groups, in both directions or one (measured
    // default: DESIGN.md 6).  The two-rounds rule once more with a group's count: a list that leaves a group's launch under
    // two tiles per workgroup is not walked by the groups (the launch runs in full, or over its flat-field list), and the
    // need levels stop below the first such launch.
    const char *sb = env("ST3D_SPLIT_BATCH");
    if (sb && sb[0]) d.split_mode = strcmp(sb, "fwd") == 0 ? SPLIT_FWD : strcmp(sb, "bwd") == 0 ? SPLIT_BWD : sb[0] == '1' ? (SPLIT_FWD | SPLIT_BWD) : 0;
    else d.split_mode = ST3D_SPLIT_BATCH_DEFAULT;
    if (B < 4 || d.flat_levels < 1) d.split_mode = 0;
    for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) {
        const bool walked = k < 3 ? d.shallow_cols[k] != 0 : k - kKeepFirst < d.keep_levels;
        d.grp_kept_on[k] = walked && (keep_force || two_rounds(hb, f.H[k + 1], kConvCout[k + 1]));
    }
    d.grp_need_levels = d.need_levels;
    for (int cs = 3; cs <= ST3D_NEED_MAX_LISTS && cs + 1 <= d.grp_need_levels; ++cs)
        if (!need_force && !two_rounds(hb, f.H[cs], kConvCin[cs])) d.grp_need_levels = cs;
    d.grp_need_gram = d.need_gram && (need_force || gram_rounds(hb));
    return d;
}

}  // namespace st3d
