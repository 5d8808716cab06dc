// epochs.h -- host bookkeeping of the keyed loss call (st3d_plan_loss_keyed, plan.hip): which geometry epoch's lists each
// slot holds, and which epoch's background the shallow forward buffers hold.  Plain C++ with no device call, so the
// stand-alone host test (tests/host/epochs_main.cpp) compiles it with the host sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>

namespace st3d {

// N list slots, least recently used first out.  A slot is named by (epoch, n): the same token with another batch size is
// another set of lists.  epoch 0 names no slot.
template <int N>
struct EpochSlots {
    uint64_t epoch[N] = {};
    int n[N] = {};
    uint64_t stamp[N] = {};         // 0 = never used
    uint64_t clock = 0;

    int find(uint64_t e, int count) const {
        if (e == 0) return -1;
        for (int i = 0; i < N; ++i)
            if (stamp[i] != 0 && epoch[i] == e && n[i] == count) return i;
        return -1;
    }
    // the slot of (e, count), marked most recently used; *fresh = it held something else (or nothing) and has been renamed:
    // the caller rebuilds every list of it
    int take(uint64_t e, int count, bool *fresh) {
        int i = find(e, count);
        *fresh = i < 0;
        if (i < 0) {
            i = 0;
            for (int k = 1; k < N; ++k)
                if (stamp[k] < stamp[i]) i = k;
            epoch[i] = e;
            n[i] = count;
        }
        stamp[i] = ++clock;
        return i;
    }
    void drop(int i) { stamp[i] = 0; epoch[i] = 0; n[i] = 0; }
    void clear() { for (int i = 0; i < N; ++i) drop(i); }
};

// What the buffers the flat-field fills write currently hold in their unlisted tiles: the background of `epoch`, filled for
// n images of this colour under this many listed launches and this state of the weights.  epoch 0 = unknown.
// kept: how many forward launches above the flat-field levels the same call ran in full or over their kept lists, bottom-up
// (conv3_1, conv3_2, conv3_3): their buffers hold the epoch's previous call in every tile, so a call that lists that many
// launches may leave the unlisted tiles alone.  A record made under another depth does not match.
struct CleanRecord {
    uint64_t epoch = 0;
    int n = 0, levels = 0, kept = 0;
    uint32_t rgb[3] = {};           // the colour's bits: -0 is not +0, a NaN equals itself
    uint64_t weights = 0;           // st3d_vgg's counter of st3d_vgg_set_conv calls

    void clear() { epoch = 0; }
    void set(uint64_t e, int count, int lv, const float *color, uint64_t w, int kp = 0) {
        epoch = e; n = count; levels = lv; weights = w; kept = kp;
        memcpy(rgb, color, sizeof(rgb));
    }
    bool matches(uint64_t e, int count, int lv, const float *color, uint64_t w, int kp = 0) const {
        uint32_t c[3];
        memcpy(c, color, sizeof(c));
        return e != 0 && epoch == e && n == count && levels == lv && kept == kp && weights == w && c[0] == rgb[0] && c[1] == rgb[1] && c[2] == rgb[2];
    }
};

}  // namespace st3d
