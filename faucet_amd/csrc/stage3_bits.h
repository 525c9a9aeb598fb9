// stage3_bits.h — 2-bit strings on the device, 32 bases at a time: what the kernels of stage3_emit.hip and stage3_join.hip share.
// The layout is fgpu_stage3_contigs_take's: A 0, C 1, T 2, G 3, 32 bases per word, the first base in the lowest bits, every string from a
// word of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr uint64_t EMIT_ODD = 0x5555555555555555ULL, EMIT_COMPLEMENT = 0xAAAAAAAAAAAAAAAAULL;

// bases a .. a + 31 of a 2-bit string of `len` bases, base a in the lowest bits; -31 <= a < len.  Fields outside 0 .. len - 1 hold no
// information (the callers mask them); no word behind the string's last one is read.
static __device__ __forceinline__ uint64_t emit_window(const uint64_t* __restrict__ w, uint32_t len, int64_t a) {
    const uint32_t words = (len + 31) >> 5;
    if (a < 0) return w[0] << (2 * (uint32_t)(-a));
    const uint32_t at = (uint32_t)(a >> 5), sh = 2 * ((uint32_t)a & 31);
    const uint64_t lo = at < words ? w[at] : 0;
    if (!sh) return lo;
    const uint64_t hi = at + 1 < words ? w[at + 1] : 0;
    return (lo >> sh) | (hi << (64 - sh));
}
// the reverse complement of 32 bases: the fields in reverse order, each code ^ 2
static __device__ __forceinline__ uint64_t emit_revcomp(uint64_t x) {
    const uint64_t r = __brevll(x);
    return (((r >> 1) & EMIT_ODD) | ((r & EMIT_ODD) << 1)) ^ EMIT_COMPLEMENT;
}
// bases pos .. pos + 31 of the string as it is read (flip: reverse-complemented), pos < len
static __device__ __forceinline__ uint64_t emit_oriented(const uint64_t* __restrict__ w, uint32_t len, bool flip, uint32_t pos) {
    return flip ? emit_revcomp(emit_window(w, len, (int64_t)len - 32 - (int64_t)pos)) : emit_window(w, len, (int64_t)pos);
}
static __device__ __forceinline__ uint64_t emit_low_fields(uint32_t n) { return n >= 32 ? ~0ULL : ((1ULL << (2 * n)) - 1); }

// the last entry e of off[lo .. hi] (ascending) with off[e] <= x, for off[lo] <= x < off[hi]
static __device__ __forceinline__ uint64_t emit_find_in(const uint64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t x) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}
// ... of off[0 .. n] with off[0] = 0, for x < off[n]
static __device__ __forceinline__ uint64_t emit_find(const uint64_t* __restrict__ off, uint64_t n, uint64_t x) { return emit_find_in(off, 0, n, x); }
