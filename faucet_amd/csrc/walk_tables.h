// walk_tables.h — what the units of pass 2 (scan_walk.hip, scan_table.hip, scan_harvest.hip) share: the junction table and the window table as the
// kernels see them, the planes of a batch, and the small device functions that look a k-mer up in the junction table.
//
// Junction table: open addressing on the CANONICAL k-mer; one slot serves both orientations of the key
// (orientation 0: key == canon, orientation 1: key == revcomp(canon)).
//   jkeys[slot]  = canon | present(orient0) << 62 | present(orient1) << 63 ; empty = ~0
//   jrecs[slot][orient] 16 bytes : dist[5] cov[4] linked(bitmask) pad[6]
//   jstamps[slot][orient]         : creation stamp
#pragma once
#include <cstdlib>

#include "fgpu_ctx.h"

namespace {

constexpr uint64_t J_EMPTY = ~0ULL;
constexpr uint64_t J_KEYMASK = (1ULL << 62) - 1;
constexpr uint32_t U_INF = 0xFFFFFFFFu;
constexpr uint64_t J_PROBE_LIMIT = 1ULL << 14;
// creation stamp = (global piece number << STAMP_SHIFT) | half-step of the visit (STAMP_FAKE for add_fake_junction's record, which
// is created after every half-step of its piece): half-steps run to 2 x windows, so a piece may span up to 2^19 - 1 windows
// (fgpu_stage_scan_walk refuses longer reads with FGPU_ERR_CAPACITY); 44 bits are left for the piece number.
constexpr int STAMP_SHIFT = 20;
constexpr uint64_t STAMP_FAKE = (1ULL << STAMP_SHIFT) - 1;

struct JTable {
    uint64_t* keys;
    uint8_t* recs;
    uint64_t* stamps;
    uint64_t mask;         // capacity - 1
    uint32_t* filter;      // presence filter: one bit per hashed canonical k-mer that owns a slot (2 bits per slot of capacity)
    uint64_t filter_mask;  // filter bits - 1
};

// The 32-bit hash of a canonical k-mer that every table of the walk stage works from: h32 = low half of fd_mix(canon).  It is computed
// ONCE per position and batch (k_need_lookup writes the plane `kh`, 4 bytes per position); the per-window kernels read it back
// instead of extracting, reverse-complementing and mixing the k-mer again (which, measured, was NOT what bounded them: they wait on
// dependent loads and on the window table's atomics -- but it is what lets k_walk_register and k_walk_link work without the k-mers).
__device__ __forceinline__ uint32_t jt_h32(uint64_t canon) { return (uint32_t)fd_mix(canon); }
// junction-table slot (capacities up to 2^32) and filter bit (a multiplicative scramble: other bits than the slot's low ones decide)
__device__ __forceinline__ uint64_t jt_filter_bit_h(const JTable& jt, uint32_t h32) {
    return (((uint64_t)(h32 * 0x9E3779B1u) << 16) ^ (uint64_t)(h32 >> 7)) & jt.filter_mask;
}
__device__ __forceinline__ uint64_t jt_filter_bit(const JTable& jt, uint64_t canon) { return jt_filter_bit_h(jt, jt_h32(canon)); }

struct WTable {
    uint64_t* keys;      // epoch << 56 | h32 << 24 | owner (see wt_register)
    uint32_t* bits;      // presence filter of 2^(32 - fshift) bits in front of the table (zeroed by k_walk_reset_uf of the window two before)
    uint64_t mask;
    uint64_t epoch;      // number of the window (1..255) << 56: entries of any other epoch count as empty slots
    uint32_t fshift;     // 32 - log2(bits of the presence filter)
};

// scheduling window = all pieces whose first window lies in [lo, hi); filled by k_walk_setup
struct WinDesc {
    uint32_t first_piece;   // index in the batch's piece list
    uint32_t n;             // pieces in the window
    uint64_t lo, hi;
};

struct Planes {
    const uint64_t* codes;
    const uint64_t* pm;
    const uint64_t* ps;
    const uint32_t* prefix;
    const uint64_t *ff, *fb, *cf0, *cf1, *cb0, *cb1;
    uint64_t *inF, *inB;
    const uint2* pieces;
    uint64_t* lk;
    const uint64_t* need;
    unsigned long long *sF, *sB;   // junction visits (FGPU_FLAG_RECORD_STOPS), else nullptr
    const uint32_t* kh;            // 32-bit hash of the canonical k-mer of every position inside a piece (k_need_lookup)
    unsigned long long* cr;        // positions at which this batch's walk created a junction record (either facing): the delta of later windows
};

__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- junction table ---------------------------------------------------------------------------
// read-only lookup (snapshot kernels): plain loads
__device__ __forceinline__ uint32_t jt_present_snapshot(const JTable& jt, uint64_t canon) {
    uint64_t s = fd_mix(canon) & jt.mask;
    for (uint64_t n = 0; n <= jt.mask; n++) {
        uint64_t w = jt.keys[s];
        if (w == J_EMPTY) return 0;
        if ((w & J_KEYMASK) == canon) return (uint32_t)(w >> 62);
        s = (s + 1) & jt.mask;
    }
    return 0;
}

// live lookup inside the walk: agent-scope loads (L1 bypass), see DESIGN.md "visibility"
__device__ __forceinline__ bool jt_find_live(const JTable& jt, uint64_t canon, uint64_t& slot, uint32_t& present) {
    uint64_t s = fd_mix(canon) & jt.mask;
    for (uint64_t n = 0; n <= jt.mask; n++) {
        uint64_t w = ld_agent(&jt.keys[s]);
        if (w == J_EMPTY) return false;
        if ((w & J_KEYMASK) == canon) { slot = s; present = (uint32_t)(w >> 62); return true; }
        s = (s + 1) & jt.mask;
    }
    return false;
}

// find or claim the slot of canon; returns false when the table is full.  `w_first` is the (already loaded) key word of the
// home slot, so that the caller can have the record of the home slot in flight at the same time.
__device__ __forceinline__ bool jt_find_or_claim(const JTable& jt, uint64_t canon, uint64_t home, uint64_t w_first, uint64_t& slot,
                                                 uint32_t& present, DevCounters* cnt) {
    uint64_t s = home;
    // The host keeps the table below a quarter full between batches (fgpu_scan_grow); a probe sequence this long means one batch
    // has outgrown it: report "full" now instead of crawling through a saturated table (16 M slots x millions of pieces)
    const uint64_t limit = jt.mask < J_PROBE_LIMIT ? jt.mask : J_PROBE_LIMIT;
    for (uint64_t n = 0; n <= limit; n++) {
        // once some walk has reported the overflow this scan is void: the others stop crawling.  Looked at only on long probe
        // sequences -- a load of that one word from every piece walk queues up in its L2 channel (+8 ms per step, measured)
        if ((n & 255) == 255 && (ld_agent((const uint64_t*)&cnt->error_flags) & 1ULL)) return false;
        uint64_t w = n == 0 ? w_first : ld_agent(&jt.keys[s]);
        if (w == J_EMPTY) {
            unsigned long long old = atomicCAS((unsigned long long*)&jt.keys[s], (unsigned long long)J_EMPTY, (unsigned long long)canon);
            if (old == J_EMPTY) {
                slot = s;
                present = 0;
                return true;
            }
            w = old;
        }
        if ((w & J_KEYMASK) == canon) { slot = s; present = (uint32_t)(w >> 62); return true; }
        s = (s + 1) & jt.mask;
    }
    return false;
}

// which of the windows [64c, 64c + 64) of a piece of nwin windows exist
__device__ __forceinline__ uint64_t chunk_mask(uint32_t nwin, uint32_t c) {
    uint32_t base = c * 64;
    if (base >= nwin) return 0;
    uint32_t rem = nwin - base;
    return rem >= 64 ? ~0ULL : ((1ULL << rem) - 1);
}

// the two bits of a key in the filter of NEW keys (fgpu_scan_import_table; k_refresh_lookup probes it with the same rule): one word, two bits
__device__ __forceinline__ uint64_t delta_word(uint32_t h32, uint64_t bits_mask) {
    return ((((uint64_t)(h32 * 0x9E3779B1u) << 16) ^ (uint64_t)(h32 >> 7)) & bits_mask) >> 5;
}
__device__ __forceinline__ uint32_t delta_bits(uint32_t h32) { return (1u << (h32 & 31)) | (1u << ((h32 >> 22) & 31)); }

struct ExportEntry {   // FGPU_TABLE_ENTRY_BYTES = 32
    uint64_t key;      // oriented k-mer
    uint64_t stamp;
    uint8_t rec[16];
};

// (one copy per unit that launches it: fgpu_scan_reset and the creation-ordered download)
__global__ void __launch_bounds__(256) k_iota_u32(uint32_t* p, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = (uint32_t)i;
}

// ---- the tables of a context, as the kernels take them -------------------------------------------
static inline uint64_t jfilter_bits(fgpu_ctx* ctx) { return ctx->jcap * 2; }
static inline JTable make_jt(fgpu_ctx* ctx) { return JTable{ctx->jkeys, ctx->jrecs, ctx->jstamps, ctx->jcap - 1, ctx->jfilter, jfilter_bits(ctx) - 1}; }
static inline WTable make_wt(fgpu_ctx* ctx, uint64_t epoch, int parity) {
    return WTable{ctx->wkeys, ctx->wbits + parity * ((1ULL << ctx->wbits_log2) / 32), ctx->wcap - 1, epoch << 56, (uint32_t)(32 - ctx->wbits_log2)};
}

}  // namespace
