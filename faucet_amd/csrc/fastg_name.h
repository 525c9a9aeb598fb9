// fastg_name.h — the name of a contig in the reference's FASTG (Contig::getFastGName, src/Contig.cpp:378-385):
//   "NODE_" << this << "_length_" << getSeq().length() << "_cov_" << getAvgCoverage()
// in integers only, so that a kernel (k_fastg_names, stage3_fastg.hip), the host's rendering and the tests' C++ check (tests/host/fastg_plan_check.cpp)
// share ONE definition.  No HIP is needed to include it.
//   `this`  a heap address in the reference; here "0x" and the contig's index in CleanGraph::tigs in hexadecimal (operator<< of a pointer's shape)
//   the coverage  operator<< of a double: printf's %g, six significant digits, of (double) sum / (double) n (ContigJuncList::getAvgCoverage,
//           utils/ContigJuncList.cpp:162-172).  glibc rounds the DOUBLE's exact decimal expansion, ties to even -- not the rational sum / n:
//           200001 / 200000 is the decimal tie 1.000005, the double next to it is not.  So the double is made first, bit for bit
//           (fgpu_fastg_quotient: the quotient rounded to nearest even at 53 bits, M 2^-s), and its six digits are round(M 10^p / 2^s) in
//           128-bit integers: M 10^15 < 2^103.  Where the exponent would go wrong by taking it from the rational (the double of a quotient a hair
//           under a power of ten), the six digits come to 1000000 and carry.
// sum <= 255 n (the entries are bytes) and 0 < n < 2^32: the average is 0 or lies in [2^-32, 255], which is all the format has to cover.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FGPU_FASTG_HD __host__ __device__
#else
#define FGPU_FASTG_HD
#endif

#define FGPU_FASTG_NAME_STRIDE 64   // bytes per entry of the name table: the name, and its length in the last byte
#define FGPU_FASTG_NAME_MAX 57      // NODE_0x (7) + 16 hex digits + _length_ (8) + 10 digits + _cov_ (5) + 11 (0.000123456, 1.23456e-10)

struct fgpu_u128 { uint64_t hi, lo; };

FGPU_FASTG_HD inline fgpu_u128 fgpu_mul_64x64(uint64_t a, uint64_t b) {
    const uint64_t a0 = a & 0xFFFFFFFFu, a1 = a >> 32, b0 = b & 0xFFFFFFFFu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFu) + (p10 & 0xFFFFFFFFu);
    fgpu_u128 r;
    r.lo = (p00 & 0xFFFFFFFFu) | (mid << 32);
    r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    return r;
}
FGPU_FASTG_HD inline uint32_t fgpu_bit_length(uint64_t v) {
    uint32_t b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// (double) sum / (double) n for 0 < sum < 2^40, 0 < n < 2^32, as the integers of the double: the value is M 2^-s with 2^52 <= M < 2^53
FGPU_FASTG_HD inline void fgpu_fastg_quotient(uint64_t sum, uint32_t n, uint64_t* M, uint32_t* s) {
    const uint32_t t = 54 + fgpu_bit_length(n) - fgpu_bit_length(sum);        // 2^53 < (sum << t) / n < 2^55; 15 <= t <= 85
    fgpu_u128 a;                                                              // sum << t  (< 2^87)
    if (t >= 64) { a.hi = sum << (t - 64); a.lo = 0; }
    else { a.hi = sum >> (64 - t); a.lo = sum << t; }
    const uint32_t limb[4] = {(uint32_t)(a.hi >> 32), (uint32_t)a.hi, (uint32_t)(a.lo >> 32), (uint32_t)a.lo};
    uint64_t rem = 0, q = 0;                                                  // the quotient has fewer than 56 bits: what leaves q's top is zero
    for (int i = 0; i < 4; i++) {
        const uint64_t cur = (rem << 32) | limb[i];
        q = (q << 32) | (cur / n);
        rem = cur % n;
    }
    uint32_t drop = fgpu_bit_length(q) - 53;                                  // 1 or 2 bits behind the 53 that stay
    uint64_t m = q >> drop;
    const uint64_t low = q & ((1ULL << drop) - 1), half = 1ULL << (drop - 1);
    if (low > half || (low == half && (rem != 0 || (m & 1)))) m++;            // to nearest, ties to even; a remainder makes it more than a tie
    if (m == (1ULL << 53)) { m >>= 1; drop++; }
    *M = m;
    *s = t - drop;
}

// printf("%g") of (double) sum / (double) n into out (at most 11 characters, no terminator); returns how many
FGPU_FASTG_HD inline uint32_t fgpu_fastg_g(uint64_t sum, uint32_t n, char* out) {
    if (sum == 0 || n == 0) { out[0] = '0'; return 1; }                       // (n == 0: no list; the callers refuse it)
    int e = 0;                                                                // floor(log10(sum / n)), from the rational
    if (sum >= (uint64_t)n) {
        if (sum >= 10ULL * n) e = 1;
        if (sum >= 100ULL * n) e = 2;
    } else {
        uint64_t scaled = sum;                                                // sum 10^j < 10 n < 2^36
        while (scaled < (uint64_t)n) { scaled *= 10; e--; }
    }
    uint64_t M;
    uint32_t s;
    fgpu_fastg_quotient(sum, n, &M, &s);
    uint64_t p = 1;
    for (int i = 0; i < 5 - e; i++) p *= 10;                                  // 10^(5 - e): 10^3 .. 10^15
    const fgpu_u128 T = fgpu_mul_64x64(M, p);                                 // the six digits are round(T / 2^s), 45 <= s <= 85
    uint64_t D;
    bool above, tie;                                                          // the part cut off: more than a half, exactly a half
    if (s >= 64) {
        const uint32_t r = s - 64;
        D = r ? T.hi >> r : T.hi;
        const uint64_t cut_hi = r ? T.hi & ((1ULL << r) - 1) : 0;
        if (r) {
            const uint64_t half = 1ULL << (r - 1);
            above = cut_hi > half || (cut_hi == half && T.lo != 0);
            tie = cut_hi == half && T.lo == 0;
        } else {
            const uint64_t half = 1ULL << 63;
            above = T.lo > half;
            tie = T.lo == half;
        }
    } else {
        D = (T.hi << (64 - s)) | (T.lo >> s);                                 // (T < 2^103 and s >= 45: fits)
        const uint64_t cut = T.lo & ((1ULL << s) - 1), half = 1ULL << (s - 1);
        above = cut > half;
        tie = cut == half;
    }
    if (above || (tie && (D & 1))) D++;
    if (D >= 1000000) { D = 100000; e++; }                                    // 999999.5 and more: the next decade
    char d[6];
    for (int i = 5; i >= 0; i--) { d[i] = (char)('0' + D % 10); D /= 10; }
    int nd = 6;
    while (nd > 1 && d[nd - 1] == '0') nd--;                                  // %g strips trailing zeros
    uint32_t at = 0;
    if (e < -4) {                                                             // exponent form below 1e-4 (the precision, 6, is never reached from above)
        out[at++] = d[0];
        if (nd > 1) {
            out[at++] = '.';
            for (int i = 1; i < nd; i++) out[at++] = d[i];
        }
        out[at++] = 'e'; out[at++] = '-';
        out[at++] = (char)('0' + (-e) / 10); out[at++] = (char)('0' + (-e) % 10);
    } else if (e >= 0) {
        for (int i = 0; i <= e; i++) out[at++] = d[i];                        // (zeros of the integer part are digits of d)
        if (nd > e + 1) {
            out[at++] = '.';
            for (int i = e + 1; i < nd; i++) out[at++] = d[i];
        }
    } else {
        out[at++] = '0'; out[at++] = '.';
        for (int i = 0; i < -e - 1; i++) out[at++] = '0';
        for (int i = 0; i < nd; i++) out[at++] = d[i];
    }
    return at;
}

// the name without its prime into out (at most FGPU_FASTG_NAME_MAX characters, no terminator); returns how many
FGPU_FASTG_HD inline uint32_t fgpu_fastg_name(uint64_t tig, uint32_t bases, uint64_t cov_sum, uint32_t cov_n, char* out) {
    uint32_t at = 0;
    const char head[] = "NODE_0x", length[] = "_length_", cov[] = "_cov_";
    for (int i = 0; i < 7; i++) out[at++] = head[i];
    int hex = 1;
    while (hex < 16 && (tig >> (4 * hex))) hex++;
    for (int i = hex - 1; i >= 0; i--) out[at++] = "0123456789abcdef"[(tig >> (4 * i)) & 15];
    for (int i = 0; i < 8; i++) out[at++] = length[i];
    int dec = 1;
    for (uint32_t v = bases; v >= 10; v /= 10) dec++;
    uint32_t v = bases;
    for (int i = dec - 1; i >= 0; i--) { out[at + i] = (char)('0' + v % 10); v /= 10; }
    at += dec;
    for (int i = 0; i < 5; i++) out[at++] = cov[i];
    return at + fgpu_fastg_g(cov_sum, cov_n, out + at);
}
