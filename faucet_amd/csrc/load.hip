// load.hip — pass 1: the two-filter Bloom load, exact and order-free.
//
// Replaces the loop body of load_two_filters (utils/Bloom.cpp:289-299):
//     for every k-mer window, in processing order:
//         if (bloo1->contains(hA,hB)) bloo2->add(hA,hB); else bloo1->add(hA,hB);
//
// Exact parallel form.  Because an occurrence either finds all of its bits set or
// sets them all, bloo1 before time t is the OR of the bits of all occurrences < t.  Hence
//     occurrence t goes to bloo2  <=>  every one of its bits was first set at a time < t.
// Per batch:
//   k_load_mark   (all windows)     test the carried-in bitmap (bloo1 as it stood before this batch).
//                                   All bits set  -> the occurrence certainly goes to bloo2: set its bits there.
//                                   Otherwise     -> atomicMin(first[bit], t) for the bits not yet in the carry,
//                                                    flag the occurrence as pending.
//   k_load_resolve (pending only)   bit is "set before t" iff it is in the carry or first[bit] < t;
//                                   all bits set before t -> bloo2.
//   k_carry_from_first              carry |= bits whose first-set time is no longer "never" (one sweep of first[]) -- not after
//                                   every batch: the carry may lag (fgpu_stage_load), a sweep closes an EPOCH of batches.
// Both kernels also write the `sure` plane (occurrence routed to bloo2), which the scan of the same reads reuses.
// t is the stream position within the epoch (pack.hip makes position order == processing order); first[] never needs a
// reset because a bit that is still 0 in the carry has first[bit] == 0xFFFFFFFF or a time of the current epoch.
// Multi-GPU shards may ask for times that count through the whole pass instead (FGPU_LOAD_SHARD_TIMES) and re-evaluate
// afterwards what they kept out of bloo2 against the lower ranks' bits (k_load_fixup).
// This unit: the plain pass, the fix-up, presence and the small utilities.  The pass by filter slices is load_slices.hip; the view of the working
// state (Filt), Bloom::add on it, the segment walker and --mercy's state machine, which both use, are load_common.h.
//
// Launch shape: a fixed grid of FGPU_GRID_BLOCKS x 256 threads strides over the stream, lanes = consecutive
// positions (so every per-position plane is written as one 8-byte ballot word per wave) and counters are
// kept in registers until the wave retires: one atomic per wave per kernel instead of one per 64 positions
// (same-address atomics serialise at ~10 ns each; 16 M of them per 10^9 positions cost more than the probes).
//
// Roofline: HBM/Infinity-Cache random access.  Algorithmic bytes per k-mer:
//   L/(L-k+1) bytes of bases + 64 B * n_hash (test-and-set on bloo1) + 64 B * rho * n_hash (set on bloo2).
#include <algorithm>

#include "fgpu_ctx.h"
#include "fgpu_flags.h"
#include "load_common.h"

namespace {

template <int REC>
__global__ void __launch_bounds__(256) k_load_mark(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad,
                                                   uint64_t T, uint64_t n_words, FdParams fp, Filt<REC> f, uint32_t tb,
                                                   uint64_t* __restrict__ pending, uint64_t plane_stride, uint64_t* __restrict__ sure, DevCounters* cnt) {
    unsigned long long n_ok = 0, n_hit = 0, n_pend = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        bool ok = p < T && fd_window_ok(bad, p, fp.k);
        bool pend = false, hit = false;
        uint32_t miss_bits = 0;
        if (ok) {
            n_ok++;
            uint64_t canon = fd_canon(fd_kmer_at(codes, p, fp.k), fp.k);
            uint64_t hA, hB;
            fd_hash_pair(canon, fp.tai_mask, hA, hB);
            // gather both filters' bits of all n_hash positions first (independent loads in flight)
            uint32_t missing = 0, b2_missing = 0;
            uint64_t h = hA;
            for (int i = 0; i < fp.n_hash; i++) {
                const uint2 v = f.load(h);
                if (!((v.x >> (h & 31)) & 1u)) missing |= 1u << i;
                if (!((v.y >> (h & 31)) & 1u)) b2_missing |= 1u << i;
                h = (h + hB) & fp.tai_mask;
            }
            if (!missing) {
                n_hit++;
                hit = true;
                if (b2_missing) {   // a stale 0 only costs a redundant atomic; bits are never cleared
                    h = hA;         // (the loops of this kernel, k_load_resolve, k_load_resolve_sm and k_carry_set stay written out: their code is the measured one)
                    for (int i = 0; i < fp.n_hash; i++) {
                        if (b2_missing & (1u << i)) atomicOr(f.word(h) + 1, 1u << (h & 31));
                        h = (h + hB) & fp.tai_mask;
                    }
                }
            } else {
                pend = true;
                n_pend++;
                miss_bits = missing;
                h = hA;
                for (int i = 0; i < fp.n_hash; i++) {
                    // the next carry is derived afterwards: from first[] by a sweep (k_carry_from_first) or by re-hashing the
                    // occurrences that were not contained (k_carry_set)
                    if (missing & (1u << i)) atomicMin(f.time(h), tb + (uint32_t)p);
                    h = (h + hB) & fp.tai_mask;
                }
            }
        }
        uint64_t pm = __ballot(pend), hm = __ballot(hit);
        // which of the first MISS_PLANES bits were missing from the carry: k_load_resolve starts from that instead of loading the
        // same words again (1.5 of its ~2.5 accesses per pending occurrence)
        uint64_t mm[MISS_PLANES];
#pragma unroll
        for (int i = 0; i < MISS_PLANES; i++) mm[i] = __ballot(pend && ((miss_bits >> i) & 1u));
        if (fd_lane() == 0) {
            pending[p >> 6] = pm;
            sure[p >> 6] = hm;
            if (pm) {
#pragma unroll
                for (int i = 0; i < MISS_PLANES; i++) pending[(i + 1) * plane_stride + (p >> 6)] = mm[i];
            }
        }
    }
    block_add(&cnt->kmers, n_ok);
    block_add(&cnt->to_bloo2, n_hit);
    block_add(&cnt->mark_hits, n_hit);
    block_add(&cnt->mark_pending, n_pend);
}

template <int REC>
__global__ void __launch_bounds__(256) k_load_resolve(const uint64_t* __restrict__ codes, uint64_t T, uint64_t n_words, FdParams fp,
                                                      Filt<REC> f, uint32_t tb,
                                                      const uint64_t* __restrict__ pending, uint64_t plane_stride, uint64_t* __restrict__ sure, DevCounters* cnt,
                                                      uint64_t* __restrict__ fail) {
    // fail != nullptr (read shards, fgpu_load_fixup): MISS_PLANES planes of "bit i of this occurrence was NOT set before it" -- every missing bit
    // is looked at then, not only up to the first that fails; needs n_hash <= MISS_PLANES
    unsigned long long n_pass = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pw = pending[p >> 6];   // wave-uniform: the 64 lanes of a wave cover one word
        if (!pw) {
            if (fail && fd_lane() == 0)
                for (int i = 0; i < MISS_PLANES; i++) fail[i * plane_stride + (p >> 6)] = 0;
            continue;
        }
        uint32_t failed = 0;
        bool pass = false;
        if ((pw >> (p & 63)) & 1ULL) {
            uint32_t missing = 0;                // what k_load_mark saw (the carry does not change between the two kernels)
#pragma unroll
            for (int i = 0; i < MISS_PLANES; i++)
                missing |= (uint32_t)((pending[(i + 1) * plane_stride + (p >> 6)] >> (p & 63)) & 1ULL) << i;
            uint64_t canon = fd_canon(fd_kmer_at(codes, p, fp.k), fp.k);
            uint64_t hA, hB;
            fd_hash_pair(canon, fp.tai_mask, hA, hB);
            pass = true;
            uint64_t h = hA;
            for (int i = 0; i < fp.n_hash; i++) {
                bool in_carry = i < MISS_PLANES ? !((missing >> i) & 1u) : ((f.load(h).x >> (h & 31)) & 1u) != 0;
                if (!in_carry && !(*f.time(h) < tb + (uint32_t)p)) {
                    pass = false;
                    failed |= 1u << i;
                    if (!fail) break;
                }
                h = (h + hB) & fp.tai_mask;
            }
            if (pass) {   // rare: every bit was set earlier in this very batch
                n_pass++;
                h = hA;
                for (int i = 0; i < fp.n_hash; i++) {
                    const uint32_t bit = 1u << (h & 31);
                    if (!(f.word(h)[1] & bit)) atomicOr(f.word(h) + 1, bit);   // a stale 0 only costs a redundant atomic
                    h = (h + hB) & fp.tai_mask;
                }
            }
        }
        const uint64_t sm = __ballot(pass);
        if (fd_lane() == 0 && sm) sure[p >> 6] |= sm;
        if (fail) {
            uint64_t fm[MISS_PLANES];
#pragma unroll
            for (int i = 0; i < MISS_PLANES; i++) fm[i] = __ballot((failed >> i) & 1u);
            if (fd_lane() == 0) {
#pragma unroll
                for (int i = 0; i < MISS_PLANES; i++) fail[i * plane_stride + (p >> 6)] = fm[i];
            }
        }
    }
    block_add(&cnt->to_bloo2, n_pass);
}

// The same resolution with every lane busy.  Only a quarter of the positions are pending, so in the kernel above a wave has ~17
// loads in flight instead of 64, and the loads go to first[] (4 bytes per filter bit: 2 GiB and more), the slowest table of the
// path: the kernel sat at a third of the random-access rate.  Here a wave shares a pool of 64 pending words (LDS, prefix counts,
// bisection -- the scheme of k_scan_flags_sm) and every lane carries one pending occurrence at a time: one first[] load per
// iteration for its next missing bit, and a lane that is done (almost always after the first load: a k-mer that is new in this
// batch set that time itself) takes the next occurrence in the same iteration.  Needs the missing planes to cover all hash
// functions (n_hash <= MISS_PLANES).
struct PendPool {
    unsigned long long m[64];
    unsigned long long miss[MISS_PLANES][64];   // the missing planes of the pool's words: read once per word, not once per occurrence
    int excl[64];
};

template <int REC>
__global__ void __launch_bounds__(256) k_load_resolve_sm(const uint64_t* __restrict__ codes, uint64_t n_words, FdParams fp, Filt<REC> f,
                                                         uint32_t tb, const uint64_t* __restrict__ pending,
                                                         uint64_t plane_stride, unsigned long long* sure, DevCounters* cnt) {
    // Plain LDS objects indexed directly, so that the accesses are ds_read / ds_write: those execute in order for a wave, which is
    // what makes a word written by one lane visible to the lane that reads it next.  (Declared volatile, or reached through a
    // generic pointer, they become FLAT accesses, whose order between the lanes of a wave is NOT guaranteed.)  The wavefront-scope
    // fences around the refill keep the compiler from moving or caching the accesses across it.
    __shared__ PendPool pools[4];
    const int wid = (int)(threadIdx.x >> 6);
    const int lane = fd_lane();
    const uint64_t lt_mask = (1ULL << lane) - 1;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t wv = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_groups = (n_words + 63) / 64;
    uint64_t grp = wv * n_groups / n_waves;
    const uint64_t grp_end = (wv + 1) * n_groups / n_waves;
    unsigned long long n_pass = 0;
    int next = 0, total = 0;
    uint64_t pool_word0 = 0;
    // one occurrence per lane: missing == 0 means the lane is free
    uint64_t hA, hB, item_p;
    uint32_t missing = 0;
    for (;;) {
        uint64_t idle = __ballot(missing == 0);
        while (idle && (next < total || grp < grp_end)) {
            if (next == total) {
                const uint64_t w = grp * 64 + lane;
                const uint64_t m = w < n_words ? pending[w] : 0ULL;
                const int c = __popcll(m);
                int incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                pools[wid].m[lane] = m;
#pragma unroll
                for (int i = 0; i < MISS_PLANES; i++) pools[wid].miss[i][lane] = m ? pending[(i + 1) * plane_stride + w] : 0ULL;
                pools[wid].excl[lane] = incl - c;
                total = __builtin_amdgcn_readlane(incl, 63);
                next = 0;
                pool_word0 = grp * 64;
                grp++;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                continue;
            }
            const int r = __popcll(idle & lt_mask);
            const int avail = total - next;
            if (missing == 0 && r < avail) {
                const int t = next + r;
                int sl = 0;
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (pools[wid].excl[sl + step] <= t) sl += step;
                const uint64_t w = pool_word0 + sl;
                const int bit = select_bit(pools[wid].m[sl], t - pools[wid].excl[sl]);
                item_p = w * 64 + bit;
                uint32_t ms = 0;
#pragma unroll
                for (int i = 0; i < MISS_PLANES; i++) ms |= (uint32_t)((pools[wid].miss[i][sl] >> bit) & 1ULL) << i;
                missing = ms;             // pending => at least one bit was missing
                fd_hash_pair(fd_canon(fd_kmer_at(codes, item_p, fp.k), fp.k), fp.tai_mask, hA, hB);
            }
            next += min(__popcll(idle), avail > 0 ? avail : 0);
            idle = __ballot(missing == 0);
        }
        if (!__ballot(missing != 0)) break;
        if (missing) {
            const uint64_t h = (hA + (uint64_t)__builtin_ctz(missing) * hB) & fp.tai_mask;
            if (!(*f.time(h) < tb + (uint32_t)item_p)) {
                missing = 0;                           // not set before this occurrence: it stays out of bloo2
            } else {
                missing &= missing - 1;
                if (!missing) {                        // rare: every bit was set earlier in this very batch
                    n_pass++;
                    uint64_t hh = hA;
                    for (int i = 0; i < fp.n_hash; i++) {
                        const uint32_t b = 1u << (hh & 31);
                        if (!(f.word(hh)[1] & b)) atomicOr(f.word(hh) + 1, b);
                        hh = (hh + hB) & fp.tai_mask;
                    }
                    atomicOr(&sure[item_p >> 6], 1ULL << (item_p & 63));
                }
            }
        }
    }
    block_add(&cnt->to_bloo2, n_pass);
}

// ---- --mercy: the state machine of load_common.h, one thread per 64-position word for the unambiguous segments that START in it; isJunction
// asks the filter and the first-set times, a run sets all of its bits in bloo2
template <int REC>
__global__ void __launch_bounds__(256) k_load_mercy(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t n_words,
                                                    FdParams fp, Filt<REC> f, uint32_t tb, const uint64_t* __restrict__ sure) {
    MercyCounts c;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x)
        fd_each_segment(bad, w, (uint64_t)fp.k, ~0ULL, [&](uint64_t p, uint64_t len) {
            mercy_segment(sure, p, len, fp.k, c,
                          [&](uint64_t pos, bool extend_rc) {
                              bool junction = false;
                              mercy_each_candidate(codes, pos, extend_rc, fp, [&](int, uint64_t e) {
                                  junction = bloo1_contains_at(f, fd_canon(e, fp.k), tb + (uint32_t)pos, fp);
                                  return !junction;
                              });
                              return junction;
                          },
                          [&](uint64_t q) { filt_set_window<1>(f, codes, q, fp); });
        });
}

// pair[w] = {a[w], b[w]} (b == nullptr: zero) / the reverse / refresh of the carry half after a batch
__global__ void __launch_bounds__(256) k_pair_join(uint2* __restrict__ pair, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                   uint64_t n32) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n32; i += (uint64_t)gridDim.x * blockDim.x)
        pair[i] = make_uint2(a[i], b ? b[i] : 0u);
}
__global__ void __launch_bounds__(256) k_pair_split(const uint2* __restrict__ pair, uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                    uint64_t n32) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n32; i += (uint64_t)gridDim.x * blockDim.x) {
        uint2 v = pair[i];
        a[i] = v.x;
        b[i] = v.y;
    }
}
// the record layout's counterparts: a record starts as {carried-in bloo1 word, empty bloo2 word, ..., 32 times "never"}; lanes = the record's
// 64 words (the unused ones are written too: whole lines, no read-modify-write); at the end the two filter words go back to the .bloom arrays
__global__ void __launch_bounds__(256) k_rec_init(uint32_t* __restrict__ rec, const uint32_t* __restrict__ a, uint64_t n32) {
    const uint64_t total = n32 * REC_WORDS;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t w = (uint32_t)(i & (REC_WORDS - 1));
        if (w >= 48) continue;                             // the fourth line of a record is never read
        rec[i] = w == 0 ? a[i >> 6] : w == 1 ? 0u : 0xFFFFFFFFu;
    }
}
__global__ void __launch_bounds__(256) k_rec_split(const uint32_t* __restrict__ rec, uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint64_t n32) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n32; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint2 v = *(const uint2*)(rec + i * REC_WORDS);
        a[i] = v.x;
        b[i] = v.y;
    }
}
// the sweep: 32 lanes per record read its 32 times (two coalesced lines), a ballot gives the record's "set since the last sweep" word
__global__ void __launch_bounds__(256) k_carry_from_rec(uint32_t* __restrict__ rec, uint64_t n32) {
    const uint64_t total = n32 * 32;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i >> 5;
        const uint32_t t = rec[r * REC_WORDS + 16 + (i & 31)];
        const uint64_t m = __ballot(t != 0xFFFFFFFFu);
        const uint32_t mine = (uint32_t)(fd_lane() < 32 ? m : m >> 32);
        if ((fd_lane() & 31) == 0 && mine) rec[r * REC_WORDS] |= mine;
    }
}

// carry := carry | bits set during the batch.  A bit is set iff its first-set time is no longer "never": one streaming
// pass over first[] (4 bytes per Bloom bit, lanes = consecutive bits, one ballot per 64 bits) replaces one atomicOr per
// newly set bit in the mark kernel.
__global__ void __launch_bounds__(256) k_carry_from_first(uint2* __restrict__ pair, const uint4* __restrict__ first4, uint64_t tai) {
    // 16 bytes per lane (a wave covers 256 consecutive Bloom bits = 1 KiB of first[]); the lane's four "was set" bits are
    // OR-reduced over groups of 16 lanes into one 64-bit word of the carry, which the group's first lane merges in
    const uint64_t n4 = tai / 4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 v = first4[i];
        const uint32_t nib = (v.x != 0xFFFFFFFFu ? 1u : 0u) | (v.y != 0xFFFFFFFFu ? 2u : 0u) | (v.z != 0xFFFFFFFFu ? 4u : 0u) |
                             (v.w != 0xFFFFFFFFu ? 8u : 0u);
        const int g = fd_lane() & 15;
        uint32_t lo = g < 8 ? nib << (4 * g) : 0u, hi = g >= 8 ? nib << (4 * (g - 8)) : 0u;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            lo |= __shfl_xor(lo, o, 64);
            hi |= __shfl_xor(hi, o, 64);
        }
        if (g == 0) {
            const uint64_t w = i >> 3;   // 4 bits per lane: lane i's bits start at Bloom bit 4i = carry word 4i/32
            if (lo) pair[w].x |= lo;
            if (hi) pair[w + 1].x |= hi;
        }
    }
}

// carry |= bits of every occurrence that was NOT contained when met (those are exactly the occurrences that set bits in
// bloo1).  The alternative to the sweep when the filter is large: its cost follows the number of new k-mers of the batch
// (3 test-then-set accesses each), not the size of first[] (32 GiB per sweep for config 4's 2^33-bit filters).
template <int REC>
__global__ void __launch_bounds__(256) k_carry_set(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T,
                                                   uint64_t n_words, FdParams fp, Filt<REC> f, const uint64_t* __restrict__ sure) {
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        if (!(p < T && fd_window_ok(bad, p, fp.k)) || ((sure[p >> 6] >> (p & 63)) & 1ULL)) continue;
        uint64_t hA, hB;
        fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
        uint64_t h = hA;
        for (int i = 0; i < fp.n_hash; i++) {
            const uint32_t bit = 1u << (h & 31);
            if (!(f.word(h)[0] & bit)) atomicOr(f.word(h), bit);
            h = (h + hB) & fp.tai_mask;
        }
    }
}

// Read shards, fgpu_load_fixup: the occurrences the shard's own pass kept out of bloo2, looked at again with the lower shards' bits.
// An occurrence goes to bloo2 iff every one of its bits was set before it: by a lower shard (all of those come earlier in file order: the
// bit is in `prefix`) or earlier in this shard.  Which of its bits were NOT set earlier in this shard the own pass has written down when it
// resolved the occurrence (the `fail` planes of k_load_resolve, FGPU_LOAD_SHARD_PLANES) -- so the question left is whether those bits are all in
// the prefix.  No first-set time is read here: a shard may hold any number of positions (k_load_fixup_times below compares 32-bit times that
// count through the whole shard: at most 2^32 positions, i.e. config 4 from 8 GPUs on -- and costs the own pass nothing, so it stays for those).
__global__ void __launch_bounds__(256) k_load_fixup(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T,
                                                    uint64_t n_words, FdParams fp, const uint32_t* __restrict__ prefix,
                                                    const uint64_t* __restrict__ fail, uint64_t plane_stride, uint32_t* bloo2,
                                                    unsigned long long* sure, DevCounters* cnt) {
    unsigned long long n_pass = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        bool pass = false;
        if (p < T && fd_window_ok(bad, p, fp.k) && !((sure[p >> 6] >> (p & 63)) & 1ULL)) {
            uint32_t failed = 0;
#pragma unroll
            for (int i = 0; i < MISS_PLANES; i++) failed |= (uint32_t)((fail[i * plane_stride + (p >> 6)] >> (p & 63)) & 1ULL) << i;
            if (failed) {                               // (an occurrence outside bloo2 has at least one)
                uint64_t hA, hB;
                fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
                pass = true;
                uint64_t h = hA;
                for (int i = 0; i < fp.n_hash && pass; i++) {
                    if (((failed >> i) & 1u) && !((prefix[h >> 5] >> (h & 31)) & 1u)) pass = false;
                    h = (h + hB) & fp.tai_mask;
                }
                if (pass) {
                    n_pass++;
                    fd_bloom_set(bloo2, hA, hB, fp.tai_mask, fp.n_hash);
                }
            }
        }
        const uint64_t sm = __ballot(pass);   // lanes = the 64 positions of one plane word
        if (fd_lane() == 0 && sm) sure[p >> 6] |= sm;
    }
    block_add(&cnt->to_bloo2, n_pass);
}

// The same question answered from first-set times, for shards of fewer than 2^32 positions (FGPU_LOAD_SHARD_TIMES: the own pass dated every
// occurrence on one clock for the whole shard and resolved with the dense kernel, which costs it nothing; rounds 2-4's form): bit set before t
// <=> in the prefix or first set locally before t.
template <int REC>
__global__ void __launch_bounds__(256) k_load_fixup_times(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T,
                                                          uint64_t n_words, FdParams fp, const uint32_t* __restrict__ prefix,
                                                          Filt<REC> f, uint32_t tb, uint32_t* bloo2, unsigned long long* sure, DevCounters* cnt) {
    unsigned long long n_pass = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        bool pass = false;
        if (p < T && fd_window_ok(bad, p, fp.k) && !((sure[p >> 6] >> (p & 63)) & 1ULL)) {
            uint64_t hA, hB;
            fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
            pass = true;
            uint64_t h = hA;
            for (int i = 0; i < fp.n_hash; i++) {
                if (!((prefix[h >> 5] >> (h & 31)) & 1u) && !(*f.time(h) < tb + (uint32_t)p)) { pass = false; break; }
                h = (h + hB) & fp.tai_mask;
            }
            if (pass) {
                n_pass++;
                fd_bloom_set(bloo2, hA, hB, fp.tai_mask, fp.n_hash);
            }
        }
        const uint64_t sm = __ballot(pass);   // lanes = the 64 positions of one plane word
        if (fd_lane() == 0 && sm) sure[p >> 6] |= sm;
    }
    block_add(&cnt->to_bloo2, n_pass);
}

// multi-GPU helper: OR the bits of every k-mer into a bitmap, no ordering
__global__ void __launch_bounds__(256) k_presence(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad,
                                                  uint64_t T, uint64_t n_words, FdParams fp, uint32_t* bitmap, DevCounters* cnt) {
    unsigned long long n_ok = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        if (!(p < T && fd_window_ok(bad, p, fp.k))) continue;
        n_ok++;
        uint64_t canon = fd_canon(fd_kmer_at(codes, p, fp.k), fp.k);
        uint64_t hA, hB;
        fd_hash_pair(canon, fp.tai_mask, hA, hB);
        fd_bloom_set(bitmap, hA, hB, fp.tai_mask, fp.n_hash);
    }
    block_add(&cnt->kmers, n_ok);
}

// unambiguous segments of length >= minlen (utils/Kmer.cpp:77; ReadScanner.cpp:268).  One thread per 64-position
// word of the bad mask: run starts are found with bit arithmetic, each start measures its run as far as minlen.
__global__ void __launch_bounds__(256) k_count_segments(const uint64_t* __restrict__ bad, uint64_t n_words, int minlen,
                                                        unsigned long long* out) {
    unsigned long long n = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x)
        fd_each_segment(bad, w, (uint64_t)minlen, (uint64_t)minlen, [&](uint64_t, uint64_t) { n++; });
    block_add(out, n);
}

__global__ void __launch_bounds__(256) k_popcount(const uint4* __restrict__ words, uint64_t n16, unsigned long long* out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long acc = 0;
    for (; i < n16; i += stride) {
        uint4 v = words[i];
        acc += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
    }
    wave_add(out, acc);
}

__global__ void __launch_bounds__(256) k_bitmap_or(uint4* __restrict__ dst, const uint4* __restrict__ src, uint64_t n16) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n16; i += stride) {
        uint4 a = dst[i], b = src[i];
        a.x |= b.x; a.y |= b.y; a.z |= b.z; a.w |= b.w;
        dst[i] = a;
    }
}

__global__ void k_probe_hash(const uint64_t* __restrict__ kmers, uint64_t n, FdParams fp, uint64_t* canon, uint64_t* hA, uint64_t* hB) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t c = fd_canon(kmers[i], fp.k);
    uint64_t a, b;
    fd_hash_pair(c, fp.tai_mask, a, b);
    canon[i] = c;
    hA[i] = a;
    hB[i] = b;
}

__global__ void k_probe_contains(const uint32_t* __restrict__ bloom, const uint64_t* __restrict__ canon, uint64_t n, FdParams fp,
                                 unsigned char* out) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fd_bloom_contains_canon(bloom, canon[i], fp.tai_mask, fp.n_hash) ? 1 : 0;
}

}  // namespace

// fgpu_create touches one kernel of every translation unit from a helper thread: the runtime loads a unit's code object at the first use of
// one of its kernels (20-25 ms for the large units), which otherwise lands on the first batch of each pass
void fgpu_touch_load() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)k_popcount);
}

// Forget the kept batches (their buffers are recycled by the next load pass).  keep_going: a new load pass starts.
void fgpu_resident_reset(fgpu_ctx* ctx, bool keep_going) {
    fgpu_adopted_release(ctx, &ctx->adopted);      // blocks that were resident batches' codes / bad (fgpu_load_batch_packed)
    ctx->resident_count = 0;
    ctx->resident_bytes = 0;
    ctx->resident_open = keep_going && ctx->resident_budget > 0;
    ctx->keep_reads = false;                       // (fgpu_load_begin sets it again for a pass with FGPU_LOAD_KEEP_READS)
    ctx->kept_reads_total = ctx->kept_max_read_len = 0;
    ctx->kept_sliced = false;                      // (fgpu_load_slice_keep_reads)
    ctx->offs_unchecked.clear();
}

// The next resident slot, its buffers sized: parts = bytes of {codes, bad, sure, fail, miss} to keep (0: not kept).  The budget arithmetic of
// every pass that keeps batches; the slot is not counted yet -- the caller does that once the batch is in it (*total: what to add to
// resident_bytes).  budgeted = false: the batch's share was counted before (packed blocks, fgpu_packed_acquire).
int fgpu_resident_take(fgpu_ctx* ctx, const uint64_t (&parts)[5], bool budgeted, ResidentBatch** out, uint64_t* total) {
    *total = parts[0] + parts[1] + parts[2] + parts[3] + parts[4];
    if (budgeted && (!ctx->resident_open || ctx->resident_bytes + *total > ctx->resident_budget)) return FGPU_TAKE_NO_BUDGET;
    if (ctx->resident_count == ctx->resident.size()) ctx->resident.push_back(new ResidentBatch());
    ResidentBatch& r = *ctx->resident[ctx->resident_count];
    DevBuf* const bufs[5] = {&r.codes, &r.bad, &r.sure, &r.fail, &r.miss};
    for (int i = 0; i < 5; i++)
        if (parts[i] && fgpu_ensure_b(ctx, bufs[i], parts[i])) return FGPU_TAKE_NO_MEMORY;
    r.packed_codes = r.packed_bad = r.packed_offs = nullptr;
    r.n_reads = 0;
    *out = &r;
    return FGPU_TAKE_OK;
}

// Adopted blocks go back once nothing queued can be reading them
void fgpu_adopted_release(fgpu_ctx* ctx, std::vector<void*>* blocks) {
    if (blocks->empty()) return;
    (void)hipSetDevice(ctx->prm.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (void* p : *blocks) (void)hipFree(p);
    blocks->clear();
}

// Keep the batch's stream and its routed-to-bloo2 plane for the scan pass (data stays in HBM between the passes
// instead of being recomputed by probing); stops silently once the budget is used: the scan then probes as usual.
int fgpu_resident_keep(fgpu_ctx* ctx) {
    if (!ctx->resident_open) return FGPU_OK;
    BatchBufs& bb = *ctx->cur;
    const uint64_t pb = (bb.n_words + FGPU_PADW) * 8;
    // read shards: which bits of an occurrence were not set before it (fgpu_load_fixup)
    const uint64_t parts[5] = {2 * pb, pb, pb, ctx->shard_planes ? MISS_PLANES * pb : 0, 0};
    ResidentBatch* r;
    uint64_t kept;
    // FGPU_LOAD_KEEP_READS: the batch's read offsets beside its planes, charged with them -- a batch that fits only without them is not kept
    const uint64_t ob = ctx->keep_reads ? (bb.n_reads + 1) * 8 : 0;
    int why = ob && ctx->resident_bytes + parts[0] + parts[1] + parts[2] + parts[3] + ob > ctx->resident_budget ? (int)FGPU_TAKE_NO_BUDGET : fgpu_resident_take(ctx, parts, true, &r, &kept);
    if (!why && ob && fgpu_ensure_b(ctx, &r->offs, ob)) why = FGPU_TAKE_NO_MEMORY;
    if (why) {
        if (why == FGPU_TAKE_NO_MEMORY) (void)hipGetLastError();   // out of memory: do without
        ctx->resident_open = false;   // batches pair by index: once one is missing, later ones would not line up
        return FGPU_OK;
    }
    if (ob) {      // (the offsets are the caller's, or a staging set's: valid while this call queues its work)
        FGPU_HIP(hipMemcpyAsync(r->offs.p, bb.d_offs, ob, hipMemcpyDeviceToDevice, ctx->stream));
        r->n_reads = bb.n_reads;
        ctx->kept_reads_total += bb.n_reads;
        kept += ob;
    }
    r->T = bb.T;
    r->n_words = bb.n_words;
    r->tb = ctx->cur_tb;
    FGPU_HIP(hipMemcpyAsync(r->codes.p, bb.codes.p, parts[0], hipMemcpyDeviceToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(r->bad.p, bb.bad.p, pb, hipMemcpyDeviceToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(r->sure.p, bb.sure.p, pb, hipMemcpyDeviceToDevice, ctx->stream));
    if (parts[3]) FGPU_HIP(hipMemcpyAsync(r->fail.p, bb.fail.p, parts[3], hipMemcpyDeviceToDevice, ctx->stream));
    ctx->resident_count++;
    ctx->resident_bytes += kept;
    return FGPU_OK;
}

// The same for a batch that was loaded from a packed block the context has adopted (fgpu_load_batch_packed): the block IS the resident batch's
// codes / bad, only `sure` is kept beside it; charged as a plain batch is (4 bits per stream position).  Beyond the budget, or without memory
// for the plane, the batch is not kept -- the later ones then are not either, as above -- and its block goes back at the end of the pass.
int fgpu_resident_adopt(fgpu_ctx* ctx, const PackedBlock& b, const fgpu_kept_reads* reads) {
    const uint64_t pb = (b.n_words + FGPU_PADW) * 8;
    const uint64_t parts[5] = {0, 0, pb, 0, 0};
    ResidentBatch* r = nullptr;
    uint64_t kept;
    const uint64_t ob = reads ? (reads->n_reads + 1) * 8 : 0;      // fgpu_load_batch_packed_reads: the offsets are adopted (and charged) with the block
    if (reads) ctx->kept_max_read_len = std::max<uint64_t>(ctx->kept_max_read_len, reads->max_read_len);
    if (ctx->resident_open && ctx->resident_bytes + 4 * pb + ob <= ctx->resident_budget) {
        if (fgpu_resident_take(ctx, parts, false, &r, &kept)) {
            (void)hipGetLastError();
            r = nullptr;
        }
    }
    if (!r) {
        ctx->resident_open = false;
        ctx->adopted_done.push_back(b.buf.p);
        if (reads) ctx->adopted_done.push_back(reads->offsets_dev);
        return FGPU_OK;
    }
    FGPU_HIP(hipMemcpyAsync(r->sure.p, ctx->cur->sure.p, pb, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->adopted.push_back(b.buf.p);
    if (reads) {
        ctx->adopted.push_back(reads->offsets_dev);
        r->packed_offs = reads->offsets_dev;
        r->n_reads = reads->n_reads;
        ctx->kept_reads_total += reads->n_reads;
    }
    r->T = b.T;
    r->n_words = b.n_words;
    r->tb = ctx->cur_tb;
    r->packed_codes = b.buf.p;
    r->packed_bad = (uint64_t*)b.buf.p + 2 * (b.n_words + FGPU_PADW);
    ctx->resident_count++;
    ctx->resident_bytes += 4 * pb + ob;
    return FGPU_OK;
}

// carry |= bits set since the last sweep; closes the epoch (times start at 0 again: every bit with a time is now in the carry).  For whichever
// state the open pass has: records, the pair + first[], or -- a sliced pass -- the slice's pair + first[] (one streaming pass over the slice)
int fgpu_load_sweep(fgpu_ctx* ctx) {
    if (ctx->epoch_positions == 0) return FGPU_OK;
    if (ctx->phase == 3) {
        if (ctx->slice_n) FGPU_LAUNCH("slice_carry_update", k_carry_from_first, 4096, 256, ctx->slice_pair, (const uint4*)ctx->slice_first, ctx->slice_n);
    } else if (ctx->rec_layout) {
        FGPU_LAUNCH("carry_update", k_carry_from_rec, 8192, 256, ctx->rec, ctx->prm.tai / 32);
    } else {
        FGPU_LAUNCH("carry_update", k_carry_from_first, 4096, 256, ctx->pair, (const uint4*)ctx->first, ctx->prm.tai);
    }
    ctx->swept_positions += ctx->epoch_positions;
    ctx->epoch_positions = 0;
    return FGPU_OK;
}

// The epoch clock and the sweep policy, shared by the plain pass and the sliced one: see the comment in fgpu_stage_load.  Before a batch: a
// sweep if the 32-bit clock of the epoch would wrap in it.  After it: the batch joins the epoch, and the epoch is closed once it has grown
// to sweep_num / sweep_den of what the carry covers and holds sweep_min positions.
int fgpu_epoch_before_batch(fgpu_ctx* ctx, uint64_t span) {
    if (!ctx->carry_by_set && !ctx->shard_times && ctx->epoch_positions + span >= 0xFFFFFFF0ULL) return fgpu_load_sweep(ctx);
    return FGPU_OK;
}
int fgpu_epoch_after_batch(fgpu_ctx* ctx, uint64_t span) {
    if (ctx->carry_by_set) return FGPU_OK;
    ctx->epoch_positions += span;
    if (ctx->epoch_positions * ctx->sweep_den >= ctx->swept_positions * ctx->sweep_num && ctx->epoch_positions >= ctx->sweep_min) return fgpu_load_sweep(ctx);
    return FGPU_OK;
}

// One batch of the plain pass in the layout of f: mark, resolve, --mercy's runs, the carry by re-hashing
// (codes, bad: the stream's planes of T positions -- the batch in hand's, or a packed block's; pending, sure, fail: the batch in hand's)
template <int REC>
static int load_batch(fgpu_ctx* ctx, const Filt<REC>& f, uint32_t tb, bool keep_fail, const uint64_t* codes, const uint64_t* bad, uint64_t T,
                      uint64_t n_words) {
    BatchBufs& bb = *ctx->cur;
    const uint64_t plane_stride = n_words + FGPU_PADW;
    const unsigned grid = fgpu_grid(n_words * 64, 256);
    static const int resolve_sm = getenv("FGPU_RESOLVE_SM") ? atoi(getenv("FGPU_RESOLVE_SM")) : 4096;
    FGPU_LAUNCH("load_mark", k_load_mark<REC>, grid, 256, codes, bad, T, n_words, ctx->fd, f,
                tb, (uint64_t*)bb.pending.p, plane_stride, (uint64_t*)bb.sure.p, ctx->counters);
    if (ctx->fd.n_hash <= MISS_PLANES && resolve_sm && !keep_fail) {
        const unsigned rgrid = (unsigned)std::min<uint64_t>((n_words + 255) / 256, (uint64_t)std::max(resolve_sm, 64));
        FGPU_LAUNCH("load_resolve", k_load_resolve_sm<REC>, rgrid, 256, codes, n_words, ctx->fd, f, tb,
                    (const uint64_t*)bb.pending.p, plane_stride, (unsigned long long*)bb.sure.p, ctx->counters);
    } else {
        FGPU_LAUNCH("load_resolve", k_load_resolve<REC>, grid, 256, codes, T, n_words, ctx->fd, f, tb,
                    (const uint64_t*)bb.pending.p, plane_stride, (uint64_t*)bb.sure.p, ctx->counters,
                    keep_fail ? (uint64_t*)bb.fail.p : (uint64_t*)nullptr);
    }
    if (ctx->prm.flags & FGPU_FLAG_MERCY)
        FGPU_LAUNCH("load_mercy", k_load_mercy<REC>, fgpu_grid(n_words, 256), 256, codes, bad,
                    n_words, ctx->fd, f, tb, (const uint64_t*)bb.sure.p);
    if (ctx->carry_by_set)
        FGPU_LAUNCH("carry_update", k_carry_set<REC>, grid, 256, codes, bad, T, n_words,
                    ctx->fd, f, (const uint64_t*)bb.sure.p);
    return FGPU_OK;
}

// the layout of the open pass, chosen in one place: fn gets the pass' state as a Filt<1> (records) or a Filt<0> (pair + first[])
template <class Fn>
static int with_layout(fgpu_ctx* ctx, Fn&& fn) {
    if (ctx->rec_layout) return fn(Filt<1>{ctx->rec, nullptr});
    return fn(Filt<0>{(uint32_t*)ctx->pair, ctx->first});
}

int fgpu_stage_load(fgpu_ctx* ctx, const void* codes, const void* bad, uint64_t T, uint64_t n_words) {
    BatchBufs& bb = *ctx->cur;
    if (T == 0) return FGPU_OK;
    const uint64_t plane_stride = n_words + FGPU_PADW;   // plane 0: pending; planes 1..MISS_PLANES: bit i missing from the carry
    int rc = fgpu_ensure_b(ctx, &bb.pending, (MISS_PLANES + 1) * plane_stride * 8);
    if (rc) return rc;
    if ((rc = fgpu_ensure_b(ctx, &bb.sure, plane_stride * 8))) return rc;
    if ((rc = fgpu_util_count_segments(ctx, bad, n_words, ctx->fd.k))) return rc;
    // Times are positions within the current EPOCH = the batches since the last sweep of first[] (k_carry_from_first).  A bit
    // that is still 0 in the carry has first[bit] == never or a time of this epoch, so the carry does not have to be brought up
    // to date after every batch: "set before t" = in the carry or first[bit] < t holds with any carry that is a subset of
    // bloo1 as of the epoch's start.  A lagging carry only sends more occurrences through the resolve kernel, and once the carry
    // holds a few coverages of the genome nearly every k-mer that will ever be in it already is: sweeps are made when an epoch
    // has grown to sweep_num/sweep_den of what the carry already covers (after batches 0, 1, 3, 7 ... of equal batches).
    const uint64_t span = n_words * 64;
    if ((rc = fgpu_epoch_before_batch(ctx, span))) return rc;
    if (ctx->shard_times && ctx->pass_positions + span >= 0xFFFFFFF0ULL) {
        ctx->err = "FGPU_LOAD_SHARD_TIMES: the pass exceeds 2^32 stream positions (FGPU_LOAD_SHARD_PLANES has no such limit)";
        return FGPU_ERR_CAPACITY;
    }
    // FGPU_LOAD_SHARD_TIMES: one clock for the whole pass (sweeps still bring the carry up to date; they just do not restart it)
    const uint32_t tb = ctx->shard_times ? (uint32_t)ctx->pass_positions : ctx->carry_by_set ? 0u : (uint32_t)ctx->epoch_positions;
    // FGPU_LOAD_SHARD_PLANES: the resolve kernel also writes down WHICH bits of an occurrence were not set before it
    const bool keep_fail = ctx->shard_planes && ctx->fd.n_hash <= MISS_PLANES;
    if (keep_fail && (rc = fgpu_ensure_b(ctx, &bb.fail, MISS_PLANES * plane_stride * 8))) return rc;
    ctx->cur_tb = tb;
    ctx->pass_positions += span;
    if ((rc = with_layout(ctx, [&](auto f) { return load_batch(ctx, f, tb, keep_fail, (const uint64_t*)codes, (const uint64_t*)bad, T, n_words); }))) return rc;
    // carry := carry | bits set during this batch -- or later: the carry may lag behind (see fgpu_load_sweep)
    return fgpu_epoch_after_batch(ctx, span);
}

// interleave the carried-in bloo1 with an empty bloo2 at the start of a load pass, split them again at its end
int fgpu_load_pair_begin(fgpu_ctx* ctx) {
    if (ctx->rec_layout) FGPU_LAUNCH("pair_join", k_rec_init, 8192, 256, ctx->rec, (const uint32_t*)ctx->bloo1, ctx->bloom_bytes / 4);
    else FGPU_LAUNCH("pair_join", k_pair_join, 2048, 256, ctx->pair, (const uint32_t*)ctx->bloo1, (const uint32_t*)nullptr, ctx->bloom_bytes / 4);
    return FGPU_OK;
}
// (a sliced pass: bloo1 / bloo2 := the own slice at its place in the tai/8-byte arrays, zero outside it)
int fgpu_load_pair_end(fgpu_ctx* ctx) {
    if (ctx->phase == 3) {
        FGPU_HIP(hipMemsetAsync(ctx->bloo1, 0, ctx->bloom_bytes, ctx->stream));
        FGPU_HIP(hipMemsetAsync(ctx->bloo2, 0, ctx->bloom_bytes, ctx->stream));
        if (ctx->slice_n)
            FGPU_LAUNCH("pair_split", k_pair_split, 2048, 256, (const uint2*)ctx->slice_pair, ctx->bloo1 + ctx->slice_lo / 32,
                        ctx->bloo2 + ctx->slice_lo / 32, ctx->slice_n / 32);
    } else if (ctx->rec_layout) {
        FGPU_LAUNCH("pair_split", k_rec_split, 4096, 256, (const uint32_t*)ctx->rec, ctx->bloo1, ctx->bloo2, ctx->bloom_bytes / 4);
    } else {
        FGPU_LAUNCH("pair_split", k_pair_split, 2048, 256, (const uint2*)ctx->pair, ctx->bloo1, ctx->bloo2, ctx->bloom_bytes / 4);
    }
    return FGPU_OK;
}

int fgpu_stage_fixup(fgpu_ctx* ctx, const uint32_t* prefix) {
    for (uint64_t i = 0; i < ctx->resident_count; i++) {
        ResidentBatch& r = *ctx->resident[i];
        if (!r.T) continue;
        int rc = FGPU_OK;
        if (ctx->shard_planes) {
            FGPU_LAUNCH("load_fixup", k_load_fixup, fgpu_grid(r.n_words * 64, 256), 256, (const uint64_t*)r.codes.p, (const uint64_t*)r.bad.p, r.T, r.n_words,
                        ctx->fd, prefix, (const uint64_t*)r.fail.p, r.n_words + FGPU_PADW, ctx->bloo2, (unsigned long long*)r.sure.p, ctx->counters);
        } else {
            rc = with_layout(ctx, [&](auto f) {
                FGPU_LAUNCH("load_fixup", k_load_fixup_times<decltype(f)::rec>, fgpu_grid(r.n_words * 64, 256), 256, (const uint64_t*)r.codes.p,
                            (const uint64_t*)r.bad.p, r.T, r.n_words, ctx->fd, prefix, f, r.tb, ctx->bloo2, (unsigned long long*)r.sure.p, ctx->counters);
                return FGPU_OK;
            });
        }
        if (rc) return rc;
    }
    return FGPU_OK;
}

int fgpu_stage_presence(fgpu_ctx* ctx) {
    BatchBufs& bb = *ctx->cur;
    if (bb.T == 0) return FGPU_OK;
    int rc;
    if ((rc = fgpu_util_count_segments(ctx, bb.bad.p, bb.n_words, ctx->fd.k))) return rc;
    FGPU_LAUNCH("presence", k_presence, fgpu_grid(bb.n_words * 64, 256), 256, (const uint64_t*)bb.codes.p, (const uint64_t*)bb.bad.p,
                bb.T, bb.n_words, ctx->fd, ctx->bloo1, ctx->counters);
    return FGPU_OK;
}

// ---- small utilities used by api.hip and scan_pure.hip --------------------------------------------
int fgpu_util_count_segments(fgpu_ctx* ctx, const void* bad, uint64_t n_words, int minlen) {
    FGPU_LAUNCH("count_segments", k_count_segments, std::min(fgpu_grid(n_words, 256), 256u), 256, (const uint64_t*)bad, n_words, minlen,
                &ctx->counters->segments);
    return FGPU_OK;
}

int fgpu_util_popcount(fgpu_ctx* ctx, const void* dev, uint64_t nbytes, unsigned long long* dev_out) {
    FGPU_LAUNCH("popcount", k_popcount, 1024, 256, (const uint4*)dev, nbytes / 16, dev_out);
    return FGPU_OK;
}

int fgpu_util_or(fgpu_ctx* ctx, void* dst, const void* src, uint64_t nbytes) {
    FGPU_LAUNCH("bitmap_or", k_bitmap_or, 2048, 256, (uint4*)dst, (const uint4*)src, nbytes / 16);
    return FGPU_OK;
}

int fgpu_util_probe_hash(fgpu_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint64_t* d_canon, uint64_t* d_hA, uint64_t* d_hB) {
    FGPU_LAUNCH("probe_hash", k_probe_hash, fgpu_blocks(n, 256), 256, d_kmers, n, ctx->fd, d_canon, d_hA, d_hB);
    return FGPU_OK;
}

int fgpu_util_probe_contains(fgpu_ctx* ctx, const uint32_t* bloom, const uint64_t* d_canon, uint64_t n, unsigned char* d_out) {
    FGPU_LAUNCH("probe_contains", k_probe_contains, fgpu_blocks(n, 256), 256, bloom, d_canon, n, ctx->fd, d_out);
    return FGPU_OK;
}
