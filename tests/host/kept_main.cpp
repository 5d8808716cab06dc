// Stand-alone host test of csrc/epochs.h with the kept depth in the clean record (the forward launches conv3_1 .. conv3_3 of
// st3d_plan_loss_keyed walk their kept lists only while the record vouches for their buffers), compiled and run with the host
// sanitizers by tests/test_kept_host.py.  No device code, no library: plain C++.
#include <stdio.h>
#include <stdlib.h>

#include "epochs.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static const float kWhite[3] = {1.f, 1.f, 1.f}, kTeal[3] = {0.125f, 0.5f, 0.625f};

static void record() {
    st3d::CleanRecord r;
    CHECK(!r.matches(1, 3, 3, kWhite, 16, 3) && !r.matches(1, 3, 3, kWhite, 16, 0));
    // a record made without kept levels vouches for none, and the other way round
    r.set(1, 3, 3, kWhite, 16);
    CHECK(r.kept == 0 && r.matches(1, 3, 3, kWhite, 16) && r.matches(1, 3, 3, kWhite, 16, 0));
    CHECK(!r.matches(1, 3, 3, kWhite, 16, 1) && !r.matches(1, 3, 3, kWhite, 16, 3));
    r.set(1, 3, 3, kWhite, 16, 3);
    CHECK(r.matches(1, 3, 3, kWhite, 16, 3));
    CHECK(!r.matches(1, 3, 3, kWhite, 16) && !r.matches(1, 3, 3, kWhite, 16, 2) && !r.matches(1, 3, 3, kWhite, 16, 4));
    // every other field still decides
    CHECK(!r.matches(2, 3, 3, kWhite, 16, 3) && !r.matches(1, 2, 3, kWhite, 16, 3) && !r.matches(1, 3, 2, kWhite, 16, 3));
    CHECK(!r.matches(1, 3, 3, kTeal, 16, 3) && !r.matches(1, 3, 3, kWhite, 17, 3) && !r.matches(0, 3, 3, kWhite, 16, 3));
    // setting again without a depth forgets it
    r.set(1, 3, 3, kWhite, 16);
    CHECK(!r.matches(1, 3, 3, kWhite, 16, 3) && r.matches(1, 3, 3, kWhite, 16, 0));
    r.set(1, 3, 3, kWhite, 16, 2);
    r.clear();
    CHECK(!r.matches(1, 3, 3, kWhite, 16, 2));
}

// the keyed entry's sequence in miniature: the slot says whether the epoch's lists exist (have_kept is reset by a fresh slot),
// the record whether the call may walk them; `listed` is what forward() decides
struct Mini {
    st3d::EpochSlots<3> slots;
    st3d::CleanRecord clean;
    bool have_kept[3] = {};
    int builds = 0;
    // -> 0 the call ran conv3_x in full, 1 over the kept lists
    int keyed(uint64_t e, int n, const float *rgb, uint64_t w, int keep, bool fail = false) {
        const st3d::CleanRecord held = clean;
        clean.clear();
        bool fresh = false;
        const int slot = slots.take(e, n, &fresh);
        if (fresh) have_kept[slot] = false;
        const bool listed = held.matches(e, n, 3, rgb, w, keep) && keep > 0;
        if (listed && !have_kept[slot]) { ++builds; have_kept[slot] = true; }
        if (fail) { slots.drop(slot); return -1; }
        clean.set(e, n, 3, rgb, w, keep);
        return listed ? 1 : 0;
    }
    void writer() { clean.clear(); }        // st3d_plan_forward, set_content, set_style, an unkeyed loss call
};

static void sequence() {
    Mini m;
    CHECK(m.keyed(1, 3, kWhite, 16, 3) == 0 && m.builds == 0);          // an epoch's first call: in full, no build
    CHECK(m.keyed(1, 3, kWhite, 16, 3) == 1 && m.builds == 1);          // the first clean call builds
    CHECK(m.keyed(1, 3, kWhite, 16, 3) == 1 && m.builds == 1);
    CHECK(m.keyed(2, 3, kWhite, 16, 3) == 0 && m.builds == 1);          // a second epoch
    CHECK(m.keyed(1, 3, kWhite, 16, 3) == 0 && m.builds == 1);          // and back: the buffers hold epoch 2, the lists stay
    CHECK(m.keyed(1, 3, kWhite, 16, 3) == 1 && m.builds == 1);
    CHECK(m.keyed(1, 3, kTeal, 16, 3) == 0);                            // another colour
    CHECK(m.keyed(1, 2, kTeal, 16, 3) == 0);                            // another n: another slot
    CHECK(m.keyed(1, 2, kTeal, 16, 3) == 1 && m.builds == 2);
    m.writer();
    CHECK(m.keyed(1, 2, kTeal, 16, 3) == 0 && m.builds == 2);
    CHECK(m.keyed(1, 2, kTeal, 17, 3) == 0);                            // the weights changed
    CHECK(m.keyed(1, 2, kTeal, 17, 3) == 1);
    CHECK(m.keyed(1, 2, kTeal, 17, 3, true) == -1);                     // a failed call: record cleared, slot dropped
    CHECK(m.keyed(1, 2, kTeal, 17, 3) == 0);
    CHECK(m.keyed(1, 2, kTeal, 17, 3) == 1 && m.builds == 3);           // the dropped slot's lists are built again
    // a geometry that changes every call never builds; nor does a plan without kept levels
    for (uint64_t e = 10; e < 30; ++e) CHECK(m.keyed(e, 3, kWhite, 17, 3) == 0);
    CHECK(m.builds == 3);
    Mini off;
    for (int i = 0; i < 4; ++i) CHECK(off.keyed(1, 3, kWhite, 16, 0) == 0);
    CHECK(off.builds == 0);
    // more epochs than slots, in a cycle: every call is a first call
    for (int round = 0; round < 3; ++round)
        for (uint64_t e = 100; e < 104; ++e) CHECK(m.keyed(e, 3, kWhite, 17, 3) == 0);
}

int main() {
    record();
    sequence();
    printf("kept ok\n");
    return 0;
}
