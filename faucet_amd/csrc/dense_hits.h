// dense_hits.h — sparse hits of a per-position pass, resolved densely by the wave that found them.
//
// A per-position kernel of pass 2 tests every position cheaply (a bit of a presence filter, a bit of a plane) and follows a chain of
// DEPENDENT loads at the few that pass.  With a lane per position the chain runs in a divergent branch: the wave pays its whole latency
// once per 64 positions however few lanes are in it.  Here a wave gathers the work masks of the U 64-position words of one round and
// hands the set bits out densely, item t to lane t mod 64: a round of U * 64 positions pays ceil(items / 64) chains.
//
//   DenseItems<U> it(masks);                       masks: wave-uniform (ballots, or plane words every lane loaded alike)
//   DenseBits<U> out;
//   for (int r = 0; r * 64 < it.total(); r++) {    uniform trip count: every lane of the wave stays in the loop through the ballot
//       const int t = r * 64 + lane;
//       bool res = false;
//       if (t < it.total()) { it.item(t, q, bit); res = chain(word q of the round, bit); }
//       out.put(r, __ballot(res));
//   }
//   plane[word u] = out.word(it, u);               the results back at their positions: one word per mask, zeros included
//
// Results that are one bit per item stay in registers: round r's ballot holds the results of items 64 r .. 64 r + 63, and the items of mask u
// are the consecutive ranks cum[u] .. cum[u + 1] - 1, so their result bits are a funnel shift of two ballots, put back at the mask's set bits
// by a prefix count.  No LDS, hence no ordering between lanes to keep.
#pragma once
#include "fgpu_flags.h"

namespace {

template <int U>
struct DenseItems {
    uint64_t m[U];       // the work masks (uniform)
    int cum[U + 1];      // items in the masks before mask u (uniform)
    __device__ __forceinline__ explicit DenseItems(const uint64_t (&masks)[U]) {
        cum[0] = 0;
#pragma unroll
        for (int u = 0; u < U; u++) {
            m[u] = masks[u];
            cum[u + 1] = cum[u] + __popcll(masks[u]);
        }
    }
    __device__ __forceinline__ int total() const { return cum[U]; }
    // item t < total(): which mask holds it (uniform bounds, per-lane t), which bit of it
    __device__ __forceinline__ void item(int t, int& q, int& bit) const {
        q = 0;
        uint64_t mq = m[0];
        int before = 0;
#pragma unroll
        for (int c = 1; c < U; c++)
            if (t >= cum[c]) { q = c; mq = m[c]; before = cum[c]; }
        bit = select_bit(mq, t - before);
    }
};

template <int U>
struct DenseBits {
    uint64_t r[U];       // round c's ballot (uniform); a round of U masks has at most U hand-out rounds
    __device__ __forceinline__ DenseBits() {
#pragma unroll
        for (int c = 0; c < U; c++) r[c] = 0;
    }
    __device__ __forceinline__ void put(int round, uint64_t ballot) {
#pragma unroll
        for (int c = 0; c < U; c++)
            if (c == round) r[c] = ballot;
    }
    // the results of mask u's items at the positions of its set bits; every lane of the wave calls
    __device__ __forceinline__ uint64_t word(const DenseItems<U>& it, int u) const {
        const int r0 = it.cum[u] >> 6, s = it.cum[u] & 63;
        uint64_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < U; c++) {
            if (c == r0) lo = r[c];
            if (c == r0 + 1) hi = r[c];
        }
        const uint64_t packed = (lo >> s) | ((hi << 1) << (63 - s));      // bit i: the result of the mask's i-th item
        const int lane = fd_lane();
        const uint64_t mu = it.m[u];
        const bool mine = ((mu >> lane) & 1ULL) && ((packed >> __popcll(mu & ((1ULL << lane) - 1))) & 1ULL);
        return __ballot(mine);
    }
};

}  // namespace
