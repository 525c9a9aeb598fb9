// load_common.h — device side of pass 1 that the plain pass (load.hip) and the sliced pass (load_slices.hip) share: the view of the working
// state (three layouts, one interface), Bloom::add / membership on a view, the segment walker and --mercy's candidate enumeration and
// per-segment state machine.
#pragma once
#include "fgpu_device.h"

constexpr int MISS_PLANES = 4;   // planes of "bit i was missing from the carry" kept for k_load_resolve (hash functions beyond are re-tested)
constexpr int MERCY_NT = 4;      // planes of the sliced pass' mercy probe: one per candidate nucleotide

// During a load pass the two filters live INTERLEAVED: pair[w] = {word w of the carried-in bloo1, word w of bloo2}.
// Both filters use the same bit positions (same hashes, same size), so one 8-byte load serves the carry test and
// the test-before-set of bloo2: 3 random loads per k-mer instead of up to 6.  fgpu_load_end splits them again.
//
// Where the working state of a load pass lives.  Three layouts, one algorithm, one interface: owns(h) -- is bit position h kept here --,
// word(h) -> the {bloo1, bloo2} words of h, load(h) both at once, time(h) -> the first-set time of h.
//   REC = 0  `base` = pair[]: {bloo1 word, bloo2 word} interleaved, 8 bytes per 32 filter bits; the first-set times in their own array first[]
//            (4 bytes per filter bit).  Filters up to 2^31 bits: the 8-byte words of config 2 (128 MiB) stay in the Infinity Cache.
//   REC = 1  `base` = 256-byte RECORDS, one per 32 filter bits, aligned: word 0 bloo1, word 1 bloo2, words 16..47 the first-set times of the
//            record's 32 bits (two further lines of the same 256 bytes), the rest unused: FGPU_LOAD_LAYOUT=records (round 5; measured, NOT the
//            default).  The marking kernel is bound by the atomicMin of the times it posts (1.9 per k-mer on configs 4 and 5), and an atomic
//            into the 256-byte block whose first line the kernel has just loaded costs half of one into a separate 32 GiB array -- same three
//            loads, same three atomics per new k-mer, other addresses (scripts/micro/mark_model3.hip: 2^33 bits, 63 % new k-mers 21.8 -> 15.8 ms
//            per 1.34e8 k-mers; blocks of 192 or 160 bytes 17.6 / 18.5: the alignment counts; 2^29 bits 7.6 -> 13.0 ms).  On config 4's reads
//            the kernel gains 14 % (231 -> 203 ms per 25 M reads), config 5's 15 %, and the pass gives it back: a sweep that brings the carry up
//            to date streams the records (20.5 ms against 8.9), a pass begins by writing 48 GiB of them (29 ms) -- profiles/r05_load_layouts.txt,
//            DESIGN.md section 10.  64 GiB instead of 34 at 2^33 bits.
//   Slice    the pair layout of the bit positions [lo, lo + n) alone, indexed by h - lo: first[] 4 bytes per own bit,
//            pair[] 8 bytes per 32 own bits (lo, n multiples of 512: (h - lo) & 31 == h & 31).  The only layout that does not own every h: a
//            position outside the slice touches no memory.
template <int REC>
struct Filt {
    static constexpr int rec = REC;
    uint32_t* base;
    uint32_t* first;
    __device__ __forceinline__ bool owns(uint64_t) const { return true; }
    __device__ __forceinline__ uint32_t* word(uint64_t h) const { return base + (REC ? ((h >> 5) << 6) : ((h >> 5) << 1)); }   // -> {bloo1, bloo2}
    __device__ __forceinline__ uint2 load(uint64_t h) const { return *(const uint2*)word(h); }
    __device__ __forceinline__ uint32_t* time(uint64_t h) const { return REC ? base + ((h >> 5) << 6) + 16 + (h & 31) : first + h; }
};
constexpr uint64_t REC_WORDS = 64;      // 32-bit words per record

struct Slice {
    uint2* pair;
    uint32_t* first;
    uint64_t lo, n;
    __device__ __forceinline__ bool owns(uint64_t h) const { return h - lo < n; }   // (unsigned: h < lo wraps past n)
    __device__ __forceinline__ uint32_t* word(uint64_t h) const { return (uint32_t*)(pair + ((h - lo) >> 5)); }
    __device__ __forceinline__ uint2 load(uint64_t h) const { return pair[(h - lo) >> 5]; }
    __device__ __forceinline__ uint32_t* time(uint64_t h) const { return first + (h - lo); }
};

// The bits of one k-mer, (hA + i hB) mod tai for i < n_hash: fn(i, h) for each in turn until it answers false.  For the kernels' own loops
// that test; the three helpers below are the loop itself, three lines each, written out (through a functor they gave the same compiler report
// but other code in every kernel that uses them).
template <class Fn>
__device__ __forceinline__ void fd_each_bit(uint64_t hA, uint64_t hB, const FdParams& fp, Fn&& fn) {
    uint64_t h = hA;
    for (int i = 0; i < fp.n_hash; i++) {
        if (!fn(i, h)) return;
        h = (h + hB) & fp.tai_mask;
    }
}

// Which of the k-mer's bits does the view own and find unset in its bloo1 (WHICH = 0) or bloo2 (1)?  One bit per hash index; the loads are
// independent (all in flight together).
template <int WHICH, class F>
__device__ __forceinline__ uint32_t filt_missing(const F& f, uint64_t hA, uint64_t hB, const FdParams& fp) {
    uint32_t missing = 0;
    uint64_t h = hA;
    for (int i = 0; i < fp.n_hash; i++) {
        if (f.owns(h) && !((f.word(h)[WHICH] >> (h & 31)) & 1u)) missing |= 1u << i;
        h = (h + hB) & fp.tai_mask;
    }
    return missing;
}

// Bloom::add of one k-mer into the view's bloo1 (WHICH = 0) or bloo2 (1): the own bits whose hash index is in `mask`.  TEST: look before the
// atomic (a stale 0 only costs a redundant atomic; bits are never cleared) -- not where the mask IS the outcome of that test (filt_missing).
template <int WHICH, bool TEST = true, class F>
__device__ __forceinline__ void filt_set(const F& f, uint64_t hA, uint64_t hB, const FdParams& fp, uint32_t mask = ~0u) {
    uint64_t h = hA;
    for (int i = 0; i < fp.n_hash; i++) {
        if ((mask & (1u << i)) && f.owns(h)) {
            const uint32_t bit = 1u << (h & 31);
            if (!TEST || !(f.word(h)[WHICH] & bit)) atomicOr(f.word(h) + WHICH, bit);
        }
        h = (h + hB) & fp.tai_mask;
    }
}
// ... of the k-mer of window q
template <int WHICH, class F>
__device__ __forceinline__ void filt_set_window(const F& f, const uint64_t* __restrict__ codes, uint64_t q, const FdParams& fp) {
    uint64_t hA, hB;
    fd_hash_pair(fd_canon(fd_kmer_at(codes, q, fp.k), fp.k), fp.tai_mask, hA, hB);
    filt_set<WHICH>(f, hA, hB, fp);
}

// TIME-AWARE membership: bloo1 as it stood when occurrence t was processed = bits of the carried-in state or first set at a time <= t.
// On a slice: no OWN bit of the k-mer was unset then ("bit b was set by time t" concerns b alone, so its owner answers it).
template <class F>
__device__ __forceinline__ bool bloo1_contains_at(const F& f, uint64_t canon, uint32_t t, const FdParams& fp) {
    uint64_t hA, hB;
    fd_hash_pair(canon, fp.tai_mask, hA, hB);
    uint64_t h = hA;
    for (int i = 0; i < fp.n_hash; i++) {
        if (f.owns(h) && !((f.load(h).x >> (h & 31)) & 1u) && !(*f.time(h) <= t)) return false;
        h = (h + hB) & fp.tai_mask;
    }
    return true;
}

// The unambiguous segments (runs of good positions) that START in word w of `bad` and are at least minlen long: fn(first position, length).
// A run is measured until it ends or has reached `cap` positions (utils/Kmer.cpp:77 only asks "at least minlen": cap = minlen; --mercy walks
// the whole run: no cap).  Bad padding past the end of the stream terminates the scan.
template <class Fn>
__device__ __forceinline__ void fd_each_segment(const uint64_t* __restrict__ bad, uint64_t w, uint64_t minlen, uint64_t cap, Fn&& fn) {
    const uint64_t good = ~bad[w];
    const uint64_t prev_good = w ? (~bad[w - 1]) >> 63 : 0;
    uint64_t starts = good & ~((good << 1) | prev_good);
    while (starts) {
        const uint64_t p = w * 64 + __builtin_ctzll(starts);
        starts &= starts - 1;
        uint64_t len = 0;
        while (len < cap) {
            const uint64_t v = fd_bits_at(bad, p + len);
            if (v) { len += __builtin_ctzll(v); break; }
            len += 64;
        }
        if (len >= minlen) fn(p, len);
    }
}

// ---- --mercy (utils/Bloom.cpp:300-333) -----------------------------------------------------------------------------
// With mercy the load also adds to bloo2 every run of low-coverage k-mers ("not contained in bloo1 when met") that sits
// between two solid ones, unless the solid k-mer next to the run looks like a junction in bloo1 (isJunction, :249-265).  bloo1
// evolves exactly as without mercy, and which occurrences were "contained" is the `sure` plane of the pass; what is left is a
// small sequential state machine per unambiguous segment plus a few time-aware membership tests (bloo1_contains_at).
//
// The candidates of isJunction(readKmer, bloo1, dir) at window pos (not the first of its segment), as load_two_filters calls it: the cursor
// faces BACKWARD there, so the "real extension" is the reverse complement of the window before, whatever dir says; dir only picks the strand
// the four candidates extend -- the reverse complement at a contained window (the low -> high test), the k-mer itself at any other.
// fn(nt, e) for every candidate e other than the real extension, until it answers false.
template <class Fn>
__device__ __forceinline__ void mercy_each_candidate(const uint64_t* __restrict__ codes, uint64_t pos, bool extend_rc, const FdParams& fp, Fn&& fn) {
    const uint64_t km = fd_kmer_at(codes, pos, fp.k), rc = fd_revcomp(km, fp.k);
    const uint64_t real_ext = ((rc << 2) | (uint64_t)(fd_base_at(codes, pos - 1) ^ 2)) & fp.kmask;
    const uint64_t from = extend_rc ? rc : km;
    for (int nt = 0; nt < MERCY_NT; nt++) {
        const uint64_t e = ((from << 2) | (uint64_t)nt) & fp.kmask;
        if (e != real_ext && !fn(nt, e)) return;
    }
}

// What the state machine did, over the segments a thread has walked (fgpu_diag_slice_mercy reports them; the plain pass drops them)
struct MercyCounts {
    unsigned long long hl_junction = 0, opened = 0, lh_junction = 0, added = 0, kmers = 0;
};

// The state machine over the windows p .. p + len - k of one segment, processed in this order (utils/Bloom.cpp:303).  `sure` says which
// windows were contained; is_junction(pos, extend_rc) answers isJunction at a window, add(q) puts window q's k-mer into bloo2.
template <class IsJunction, class Add>
__device__ __forceinline__ void mercy_segment(const uint64_t* __restrict__ sure, uint64_t p, uint64_t len, int k, MercyCounts& c,
                                              IsJunction&& is_junction, Add&& add) {
    const uint64_t n = len - k + 1;
    bool have_last = false;
    int64_t hv_lo = -1;                     // first window of the current hash_vals run, -1 = empty
    uint64_t sbits = 0;
    for (uint64_t i = 0; i < n; i++) {
        if ((i & 63) == 0) sbits = fd_bits_at(sure, p + i);
        const bool contained = (sbits >> (i & 63)) & 1ULL;
        const uint64_t pos = p + i;         // (a test is only made at i > 0: both kinds need an earlier window of the segment)
        if (contained) {
            have_last = true;
            if (hv_lo >= 0) {               // came from low to high (:311-318)
                if (is_junction(pos, true)) {
                    c.lh_junction++;
                } else {
                    c.added++;
                    for (uint64_t q = p + (uint64_t)hv_lo; q < pos; q++) {
                        c.kmers++;
                        add(q);
                    }
                }
                hv_lo = -1;
            }
        } else if (have_last && hv_lo < 0) {   // came from high to low (:322-326); later low k-mers just join the run
            if (is_junction(pos, false)) {
                c.hl_junction++;
            } else {
                c.opened++;
                hv_lo = (int64_t)i;
            }
        }
    }
}
