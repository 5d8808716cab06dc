// tilebins.h -- the per-tile LDS pre-aggregation table of the K = 1 gradient scatters (shade.hip, mipmap.hip: texels;
// vcolor.hip: vertices).  A workgroup of 256 lanes is one 16 x 16-pixel tile; every lane brings up to DEPS deposits
// (key, weight) and three channel factors.  Neighbouring pixels hit the same keys, so the contributions are summed per key
// in LDS first and each distinct key of the tile then costs three global atomics instead of three per contribution.
// The table is two pieces, so that only the keys are cleared and only what the tile used is zeroed and flushed:
//   s_key    open addressing on the key (texel or vertex index), SLOTS of them.  The lane whose CAS claimed a slot owns
//            the key.
//   s_id, s_acc  one compact entry per distinct key, ENTRIES = DEPS x 256 of them: after a barrier every owner takes the next
//            entry (one LDS atomic per wave and deposit), zeroes its three sums, notes the key and replaces the slot's
//            key by the entry's number; after the next barrier every lane reads the entry of its slots and deposits.
// acc_t float: float LDS sums + float global atomics.  acc_t unsigned long long: the same binning in 64-bit fixed point
// (det.h; `gout` is then the int64 accumulator array and `dscale` the power-of-two scale): bitwise reproducible whatever
// the order.
#pragma once
#include <type_traits>

#include "det.h"

namespace st3d_tilebins {

constexpr int log2_of(int n) { return n <= 1 ? 0 : 1 + log2_of(n >> 1); }

// a view of the kernel's LDS arrays (ST3D_TILEBINS declares them: separate arrays, as the compiler lays them out best)
template <typename acc_t, int DEPS, int SLOTS, int ENTRIES>
struct TileBins {
    static constexpr bool kFixed = !std::is_same<acc_t, float>::value;
    static_assert((SLOTS & (SLOTS - 1)) == 0, "the probe wraps with a mask");
    // at most DEPS * 256 distinct keys enter, so at least half the slots stay free and the unbounded probe below always
    // finds its key or a free slot: a smaller table could fill up and spin for ever
    static_assert(SLOTS >= 2 * DEPS * 256, "the probe must terminate");
    static_assert(ENTRIES >= DEPS * 256, "every deposit of a tile may be a key of its own");
    static_assert(DEPS >= 1 && DEPS <= 4, "one bit of `valid` and `mine` per deposit");

    int *s_key;
    int *s_id;
    acc_t (*s_acc)[3];
    int *s_count;

    // clears the keys; ends in a barrier.  All 256 lanes call it, after everybody has left the previous pass.
    __device__ __forceinline__ void reset() const {
        for (int e = threadIdx.x; e < SLOTS; e += 256) s_key[e] = -1;
        if (threadIdx.x == 0) *s_count = 0;
        __syncthreads();
    }

    // claim, compact, deposit, flush.  All 256 lanes call it on a reset table; bit c of `valid`: deposit c exists
    // (dep_key[c], dep_w[c] are read only then).  Adds dep_g[ch] * dep_w[c] to gout[dep_key[c] * 3 + ch].  The table is
    // in use until every lane has returned: a barrier of the caller's before the next reset().
    __device__ __forceinline__ void scatter(const int (&dep_key)[DEPS], const float (&dep_w)[DEPS], const float (&dep_g)[3],
                                            unsigned valid, double dscale, float *__restrict__ gout) const {
        const int tid = threadIdx.x;
        int slot[DEPS];
        unsigned mine = 0;               // bit c: this lane's CAS claimed the slot of deposit c
#pragma unroll
        for (int c = 0; c < DEPS; ++c) {
            slot[c] = 0;
            if (valid >> c & 1) {
                const int k = dep_key[c];
                int s = (int)(((unsigned)k * 2654435761u) >> (32 - log2_of(SLOTS)));       // the top bits: < SLOTS
                for (;;) {
                    const int prev = atomicCAS(&s_key[s], -1, k);
                    if (prev == -1) mine |= 1u << c;
                    if (prev == -1 || prev == k) break;
                    s = (s + 1) & (SLOTS - 1);
                }
                slot[c] = s;
            }
        }
        __syncthreads();                 // every key is in: nobody probes any more
#pragma unroll
        for (int c = 0; c < DEPS; ++c) {
            const bool own = mine >> c & 1;
            const unsigned long long owners = __ballot(own);
            if (owners == 0) continue;
            const int lane = tid & 63, leader = __ffsll((long long)owners) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(s_count, __popcll(owners));
            base = __shfl(base, leader);
            if (own) {
                const int e = base + __popcll(owners & ((1ull << lane) - 1ull));
                s_id[e] = dep_key[c];
                s_acc[e][0] = (acc_t)0; s_acc[e][1] = (acc_t)0; s_acc[e][2] = (acc_t)0;
                s_key[slot[c]] = e;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < DEPS; ++c) {
            if (!(valid >> c & 1)) continue;
            const int e = s_key[slot[c]];
            const float w = dep_w[c];
            if constexpr (kFixed) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    atomicAdd(&s_acc[e][ch], (unsigned long long)st3d_det::det_quantise(dep_g[ch] * w, dscale));
            } else {
                atomicAdd(&s_acc[e][0], dep_g[0] * w);
                atomicAdd(&s_acc[e][1], dep_g[1] * w);
                atomicAdd(&s_acc[e][2], dep_g[2] * w);
            }
        }
        __syncthreads();
        const int used = *s_count * 3;
        for (int e = tid; e < used; e += 256) {
            const int entry = e / 3, c = e - entry * 3;
            const acc_t v = s_acc[entry][c];
            if (v == (acc_t)0) continue;
            const int k = s_id[entry];
            if constexpr (kFixed) atomicAdd(reinterpret_cast<unsigned long long *>(gout) + (size_t)k * 3 + c, v);
            else atomicAdd(gout + (size_t)k * 3 + c, v);
        }
    }
};

}  // namespace st3d_tilebins

// the LDS of one table in a kernel, and `name`, its view: 4 * SLOTS + (4 + 3 * sizeof(acc_t)) * ENTRIES + 4 bytes
#define ST3D_TILEBINS(name, acc_t, DEPS, SLOTS, ENTRIES)                                     \
    __shared__ int name##_key[SLOTS];                                                        \
    __shared__ int name##_id[ENTRIES];                                                       \
    __shared__ acc_t name##_acc[ENTRIES][3];                                                 \
    __shared__ int name##_count;                                                             \
    const st3d_tilebins::TileBins<acc_t, DEPS, SLOTS, ENTRIES> name = {name##_key, name##_id, name##_acc, &name##_count}

// the two tables in use.  Texels: four footprint corners per pixel, 36 KB + 4 B of LDS in fixed point, 24 KB + 4 B in float.
// Vertices: the three corners of the pixel's face, 29 KB + 4 B and 20 KB + 4 B.
#define ST3D_TEXEL_BINS(name, acc_t) ST3D_TILEBINS(name, acc_t, 4, 2048, 1024)
#define ST3D_VERTEX_BINS(name, acc_t) ST3D_TILEBINS(name, acc_t, 3, 2048, 768)
