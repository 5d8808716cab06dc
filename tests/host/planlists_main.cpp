// Stand-alone host test of csrc/planlists.h (what st3d_plan_create decides about the plan's lists), compiled and run with the
// host sanitizers by tests/test_planlists_host.py.  No device code, no library: plain C++.
//   1. the switches' parsing rules as direct cases, on facts made up here;
//   2. every line of stdin is one row of facts and switches (tests/golden/plan_decisions.json, flattened by the test):
//      its decision is printed as one JSON line.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>

#include "planlists.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

using namespace st3d;

static std::map<std::string, std::string> g_env;
static const char *env(const char *name) {
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
static PlanDecisions decide(const PlanFacts &f, std::map<std::string, std::string> e) {
    g_env = e;
    return decide_lists(f, env);
}

// a plan whose conv1_2 .. conv3_4 run F(4x4,3x3) in both directions with every gate on, whose kernels cover every list and
// whose own tile geometry is 8 x 64 everywhere
static PlanFacts facts(int B, int S) {
    PlanFacts f;
    f.B = B; f.S = S; f.cus = 256;
    for (int cs = 0, H = S; cs < 16; ++cs) {
        f.H[cs] = H;
        if (pool_slot(kConvIdx[cs] + 2) >= 0) H /= 2;
        if (cs >= 1 && cs <= 7) f.route[cs] = Route{WINO43, true, true, true, cs >= 2};
    }
    f.fused_tap0 = true;
    f.need_levels = 3; f.blocks_lists = 6; f.flat_levels = 3;
    for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) { f.geo_rows[k] = 8; f.geo_cols[k] = 64; }
    f.gram_segs = true;
    f.gram_runs = 64;
    return f;
}

template <int N>
static bool is(const int (&a)[N], std::initializer_list<int> want) {
    int i = 0;
    for (int w : want)
        if (a[i++] != w) return false;
    return i == N;
}

static void rules() {
    const PlanFacts big = facts(8, 512);        // maps 512, 256, 256, 128 x 4
    const std::map<std::string, std::string> force = {{"ST3D_NEED_FORCE", "1"}, {"ST3D_KEEP_FORCE", "1"}};
    auto with = [&](std::map<std::string, std::string> e) { e.insert(force.begin(), force.end()); return e; };
    PlanDecisions d = decide(big, force);
    CHECK(d.need_blocks && d.need_levels == 7 && d.need_gram && d.flat_levels == 3 && d.keep_levels == 3);
    CHECK(is(d.need_cols, {16, 16, 16, 32, 16, 16}) && is(d.shallow_cols, {32, 16, 32}) && d.keep_first == 0);
    CHECK(is(d.keep_cols, {32, 16, 32, 16, 16, 16}) && d.split_mode == ST3D_SPLIT_BATCH_DEFAULT);

    // ---- ST3D_NEED_TILE
    d = decide(big, with({{"ST3D_NEED_TILE", "32"}}));              // no comma: every list
    CHECK(is(d.need_cols, {32, 32, 32, 32, 32, 32}));
    d = decide(big, with({{"ST3D_NEED_TILE", "32,16"}}));           // the last value repeats
    CHECK(is(d.need_cols, {32, 16, 16, 16, 16, 16}));
    d = decide(big, with({{"ST3D_NEED_TILE", "64,32,16,0,16,32"}, {"ST3D_NEED_DEPTH", "3"}}));
    // one value per list for all six, whether or not the level engages; 64 is the kernel's own here and 0 asks for it: both 0
    CHECK(d.need_levels == 3 && is(d.need_cols, {0, 32, 16, 0, 16, 32}));
    d = decide(big, with({{"ST3D_NEED_TILE", "48"}}));              // fits nothing
    CHECK(is(d.need_cols, {0, 0, 0, 0, 0, 0}));
    d = decide(big, with({{"ST3D_NEED_TILE", ""}}));                // empty: the defaults
    CHECK(is(d.need_cols, {16, 16, 16, 32, 16, 16}));
    {
        PlanFacts f = facts(8, 64);             // maps 64, 32, 32, 16 x 4: 64 fits list 0 only, strips only where the kernel has rows
        for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) { f.geo_rows[k] = k < 3 ? 8 : 0; f.geo_cols[k] = k < 3 ? 32 : 0; }
        d = decide(f, with({{"ST3D_NEED_TILE", "64"}}));
        CHECK(is(d.need_cols, {64, 0, 0, 0, 0, 0}));
        d = decide(f, with({{"ST3D_NEED_TILE", "16"}}));
        CHECK(is(d.need_cols, {16, 16, 16, 0, 0, 0}));
    }

    // ---- ST3D_KEEP_TILE: asked only for the levels the loop reaches; it ends at the first level that fails
    d = decide(big, with({{"ST3D_KEEP_TILE", "16,32,64"}}));
    CHECK(d.keep_levels == 3 && d.keep_cols[3] == 16 && d.keep_cols[4] == 32 && d.keep_cols[5] == 64);
    d = decide(big, with({{"ST3D_KEEP_TILE", "32,48,16"}}));
    CHECK(d.keep_levels == 1 && d.keep_cols[3] == 32 && d.keep_cols[4] == 0 && d.keep_cols[5] == 0);
    d = decide(big, with({{"ST3D_KEEP_TILE", "0"}}));               // the kernel's own geometry
    CHECK(d.keep_levels == 3 && d.keep_cols[3] == 64 && d.keep_cols[5] == 64);
    {
        PlanFacts f = big;                      // 16 fits there whatever the kernel says about strips
        for (int k = 0; k < ST3D_NEED_MAX_LISTS; ++k) f.geo_rows[k] = 0;
        d = decide(f, with({{"ST3D_KEEP_TILE", "16"}}));
        CHECK(d.keep_levels == 3 && d.keep_cols[3] == 16 && is(d.need_cols, {0, 0, 0, 32, 0, 0}));
    }
    {
        PlanFacts f = big;                      // conv3_2 not an F(4x4,3x3) forward: the second value is never asked for
        f.route[5].fwd = WINO;
        d = decide(f, with({{"ST3D_KEEP_TILE", "32,48"}}));
        CHECK(d.keep_levels == 1 && d.keep_cols[3] == 32);
    }

    // ---- ST3D_KEEP_SHALLOW
    d = decide(big, with({{"ST3D_KEEP_SHALLOW", "32"}}));           // after the last value: 0, off
    CHECK(is(d.shallow_cols, {32, 0, 0}) && d.keep_first == 0 && is(d.keep_cols, {32, 16, 16, 16, 16, 16}));
    d = decide(big, with({{"ST3D_KEEP_SHALLOW", "16,16,16"}}));     // strips only without a fused pool; the unfit level is skipped
    CHECK(is(d.shallow_cols, {0, 16, 0}) && d.keep_first == 1 && d.keep_cols[0] == 0 && d.keep_cols[1] == 16 && d.keep_cols[2] == 16);
    d = decide(big, with({{"ST3D_KEEP_SHALLOW", "0,0,0"}}));
    CHECK(is(d.shallow_cols, {0, 0, 0}) && d.keep_first == kKeepFirst && is(d.keep_cols, {0, 0, 0, 16, 16, 16}));
    d = decide(big, with({{"ST3D_KEEP_SHALLOW", ""}}));             // set but empty: off, unlike ST3D_NEED_TILE
    CHECK(is(d.shallow_cols, {0, 0, 0}));
    d = decide(big, with({{"ST3D_KEEP_DEPTH", "0"}}));              // only above a kept conv3_1
    CHECK(d.keep_levels == 0 && is(d.shallow_cols, {0, 0, 0}) && d.keep_first == kKeepFirst && !d.grp_kept_on[0] && !d.grp_kept_on[3]);

    // ---- the depth caps hold only for 0 <= value < levels
    for (const char *v : {"7", "8", "-1"}) CHECK(decide(big, with({{"ST3D_NEED_DEPTH", v}})).need_levels == 7);
    for (const char *v : {"3", "-1"}) CHECK(decide(big, with({{"ST3D_FLAT_DEPTH", v}, {"ST3D_KEEP_DEPTH", v}})).keep_levels == 3);
    d = decide(big, with({{"ST3D_NEED_DEPTH", "2"}, {"ST3D_FLAT_DEPTH", "2"}}));
    CHECK(d.need_levels == 2 && !d.need_gram && d.grp_need_levels == 2 && d.flat_levels == 2 && d.keep_levels == 0);
    CHECK(decide(big, with({{"ST3D_KEEP_DEPTH", "2"}})).keep_levels == 2 && decide(big, with({{"ST3D_NEED_DEPTH", "0"}})).need_levels == 0);

    // ---- each force lifts its own rule only (one image at 128^2: no launch walks two rounds)
    const PlanFacts small = facts(1, 128);
    d = decide(small, {});
    CHECK(d.need_levels == 3 && !d.need_gram && is(d.need_cols, {0, 0, 0, 0, 0, 0}) && d.keep_levels == 0 && is(d.shallow_cols, {0, 0, 0}));
    d = decide(small, {{"ST3D_NEED_FORCE", "1"}});
    CHECK(d.need_levels == 7 && d.need_gram && d.grp_need_gram && d.grp_need_levels == 7 && is(d.need_cols, {16, 16, 16, 32, 16, 16}));
    CHECK(d.keep_levels == 0 && is(d.shallow_cols, {0, 0, 0}));
    d = decide(small, {{"ST3D_KEEP_FORCE", "1"}});
    CHECK(d.need_levels == 3 && !d.need_gram && d.keep_levels == 3 && is(d.shallow_cols, {32, 16, 32}) && d.grp_kept_on[0] && d.grp_kept_on[5]);
    // the two-rounds rule at its edge: conv3_1 forward, 128 x 128 map, 256 output channels, 256 CUs: 64 tiles an image against 128
    CHECK(decide(facts(1, 512), {}).keep_levels == 0 && decide(facts(2, 512), {}).keep_levels == 3);
    d = decide(facts(2, 512), {});              // ... and a group of one image walks no kept list
    CHECK(d.split_mode == 0 && !d.grp_kept_on[3]);
    d = decide(facts(4, 512), {});
    CHECK(d.split_mode == SPLIT_FWD && d.grp_kept_on[3]);

    // ---- ST3D_SPLIT_BATCH
    CHECK(decide(big, {{"ST3D_SPLIT_BATCH", "0"}}).split_mode == 0 && decide(big, {{"ST3D_SPLIT_BATCH", "1"}}).split_mode == (SPLIT_FWD | SPLIT_BWD));
    CHECK(decide(big, {{"ST3D_SPLIT_BATCH", "fwd"}}).split_mode == SPLIT_FWD && decide(big, {{"ST3D_SPLIT_BATCH", "bwd"}}).split_mode == SPLIT_BWD);
    CHECK(decide(big, {{"ST3D_SPLIT_BATCH", ""}}).split_mode == ST3D_SPLIT_BATCH_DEFAULT);
    CHECK(decide(facts(3, 512), {{"ST3D_SPLIT_BATCH", "1"}}).split_mode == 0);
    CHECK(decide(big, {{"ST3D_SPLIT_BATCH", "1"}, {"ST3D_FLAT_DEPTH", "0"}}).split_mode == 0);
    // ---- the other switches
    d = decide(big, with({{"ST3D_NEED_BLOCKS", "0"}}));
    CHECK(!d.need_blocks && d.need_levels == 3 && !d.need_gram && is(d.need_cols, {0, 0, 0, 0, 0, 0}));
    d = decide(big, with({{"ST3D_NEED_GRAM", "0"}}));
    CHECK(d.need_levels == 7 && !d.need_gram && !d.grp_need_gram);
}

static int next_int(char *&c) { return (int)strtol(c, &c, 10); }

int main() {
    rules();
    static char line[4096];
    int rows = 0;
    while (fgets(line, sizeof(line), stdin)) {
        char *c = line;
        PlanFacts f;
        f.B = next_int(c); f.S = next_int(c); f.cus = next_int(c);
        for (int &h : f.H) h = next_int(c);
        for (Route &r : f.route) {
            r.fwd = (uint8_t)next_int(c);
            r.dgrad_wino = next_int(c) != 0; r.dgrad_w43 = next_int(c) != 0; r.gate_taps = next_int(c) != 0; r.gate_dst = next_int(c) != 0;
        }
        f.fused_tap0 = next_int(c) != 0;
        f.need_levels = next_int(c); f.blocks_lists = next_int(c); f.flat_levels = next_int(c);
        for (int &v : f.geo_rows) v = next_int(c);
        for (int &v : f.geo_cols) v = next_int(c);
        f.gram_segs = next_int(c) != 0;
        f.gram_runs = (size_t)next_int(c);
        g_env.clear();
        for (int n = next_int(c); n > 0; --n) {
            char name[64], value[64];
            int used = 0;
            CHECK(sscanf(c, " %63s %63s%n", name, value, &used) == 2);
            c += used;
            g_env[name] = value;
        }
        const PlanDecisions d = decide_lists(f, env);
        auto arr = [](const char *name, auto get, int n) {
            printf("\"%s\":[", name);
            for (int i = 0; i < n; ++i) printf("%s%d", i ? "," : "", (int)get(i));
            printf("],");
        };
        printf("{\"need_levels\":%d,\"need_blocks\":%d,", d.need_levels, (int)d.need_blocks);
        arr("need_cols", [&](int k) { return d.need_cols[k]; }, ST3D_NEED_MAX_LISTS);
        printf("\"need_gram\":%d,\"flat_levels\":%d,\"keep_levels\":%d,", (int)d.need_gram, d.flat_levels, d.keep_levels);
        arr("keep_cols", [&](int k) { return d.keep_cols[k]; }, ST3D_NEED_MAX_LISTS);
        arr("shallow_cols", [&](int k) { return d.shallow_cols[k]; }, 3);
        printf("\"keep_first\":%d,\"split_mode\":%d,", d.keep_first, d.split_mode);
        arr("grp_kept_on", [&](int k) { return d.grp_kept_on[k]; }, ST3D_NEED_MAX_LISTS);
        printf("\"grp_need_levels\":%d,\"grp_need_gram\":%d}\n", d.grp_need_levels, (int)d.grp_need_gram);
        ++rows;
    }
    printf("planlists ok %d\n", rows);
    return 0;
}
