// Stand-alone host test of csrc/epochs.h (the slot and clean-record bookkeeping of st3d_plan_loss_keyed), compiled and run
// with the host sanitizers by tests/test_epochs_host.py.  No device code, no library: plain C++.
#include <math.h>
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

static void slots() {
    st3d::EpochSlots<3> s;
    bool fresh = false;
    CHECK(s.find(5, 3) == -1 && s.find(0, 3) == -1);
    const int a = s.take(5, 3, &fresh);
    CHECK(fresh && a >= 0 && a < 3 && s.find(5, 3) == a);
    CHECK(s.take(5, 3, &fresh) == a && !fresh);
    CHECK(s.find(5, 2) == -1);                      // another n is another set of lists
    const int a2 = s.take(5, 2, &fresh);
    CHECK(fresh && a2 != a);
    const int b = s.take(6, 3, &fresh);
    CHECK(fresh && b != a && b != a2);
    // all three in use; least recently used is (5, 3).  Touch it, then a fourth epoch evicts (5, 2)
    CHECK(s.take(5, 3, &fresh) == a && !fresh);
    const int c = s.take(7, 3, &fresh);
    CHECK(fresh && c == a2 && s.find(5, 2) == -1 && s.find(5, 3) == a && s.find(6, 3) == b && s.find(7, 3) == c);
    // a dropped slot is the next one taken and holds nothing
    s.drop(b);
    CHECK(s.find(6, 3) == -1);
    CHECK(s.take(8, 1, &fresh) == b && fresh);
    // many epochs in a cycle longer than the slots: every take is fresh, none returns another epoch's slot as a hit
    for (int round = 0; round < 5; ++round)
        for (uint64_t e = 100; e < 104; ++e) {
            const int i = s.take(e, 3, &fresh);
            CHECK(fresh && i >= 0 && i < 3 && s.find(e, 3) == i);
        }
    // two alternating epochs stay put
    const int x = s.take(200, 3, &fresh), y = s.take(201, 3, &fresh);
    for (int round = 0; round < 100; ++round) {
        CHECK(s.take(200, 3, &fresh) == x && !fresh);
        CHECK(s.take(201, 3, &fresh) == y && !fresh);
    }
    // ids beyond 32 bits are told apart
    const uint64_t big = (1ull << 40) + 200;
    CHECK(s.find(big, 3) == -1);
    s.clear();
    CHECK(s.find(200, 3) == -1 && s.find(201, 3) == -1);
}

static void record() {
    st3d::CleanRecord r;
    const float white[3] = {1.f, 1.f, 1.f}, teal[3] = {0.125f, 0.5f, 0.625f};
    CHECK(!r.matches(1, 3, 3, white, 16));          // nothing recorded
    CHECK(!r.matches(0, 0, 0, white, 0));           // epoch 0 never matches, not even the empty record
    r.set(1, 3, 3, white, 16);
    CHECK(r.matches(1, 3, 3, white, 16));
    CHECK(!r.matches(2, 3, 3, white, 16) && !r.matches(1, 2, 3, white, 16) && !r.matches(1, 3, 2, white, 16));
    CHECK(!r.matches(1, 3, 3, teal, 16) && !r.matches(1, 3, 3, white, 17));
    const float one_off[3] = {1.f, 1.f, nextafterf(1.f, 2.f)};
    CHECK(!r.matches(1, 3, 3, one_off, 16));
    r.clear();
    CHECK(!r.matches(1, 3, 3, white, 16));
    // the colour is compared as bits: -0 is not +0, a NaN equals itself
    const float pz[3] = {0.f, 0.f, 0.f}, nz[3] = {0.f, -0.f, 0.f}, nan3[3] = {NAN, 0.f, 0.f};
    r.set(9, 1, 1, pz, 0);
    CHECK(r.matches(9, 1, 1, pz, 0) && !r.matches(9, 1, 1, nz, 0));
    r.set(9, 1, 1, nan3, 0);
    CHECK(r.matches(9, 1, 1, nan3, 0));
    r.set(0, 1, 1, pz, 0);                          // recording epoch 0 records nothing
    CHECK(!r.matches(0, 1, 1, pz, 0));
}

int main() {
    slots();
    record();
    printf("epochs ok\n");
    return 0;
}
