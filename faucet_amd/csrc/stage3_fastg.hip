// stage3_fastg.hip — Stage 3's graph as text: ContigGraph::printGraph's FASTG written on the device from strings that are joined already
// (fgpu_stage3_fastg; include/faucet_gpu.h has the format and the reference lines).  Which records, in which order and with which neighbours is
// the host's business (CleanGraph::fastg_records, clean_graph.h); fgpu_stage3_raw_graph and fgpu_stage3_graph_fastg (stage3_emit.hip) put the
// two together.  Three kernels, integer and bitwise only:
//   k_fastg_names  one lane per record: "NODE_0x<tig>_length_<bases>_cov_<%g>" (fastg_name.h, the host's definition too) into a table of
//                  FGPU_FASTG_NAME_STRIDE bytes per record, the name's length in the entry's last byte.  A header is put together from the
//                  entries of the record and of its at most four neighbours.
//   k_fastg_sizes  per record the bytes of its two header lines (kept: k_fastg_text's lanes find their place in a record with them) and of its
//                  four lines together; rocPRIM scans the latter.
//   k_fastg_text   one block per FGPU_FASTG_TILE bytes of OUTPUT, one lane per 16 bytes, as k_emit_ascii (stage3_emit.hip) has it: the block looks
//                  up its first record once and keeps the byte offsets of the records its tile can touch in LDS (a record has at least 57 bytes,
//                  so at most 73 of them); a lane whose 16 bytes lie inside a sequence expands 16 codes and stores them at once -- the second
//                  strand from the SAME 2-bit string, reverse-complemented 32 bases at a time (stage3_bits.h) --, a lane on a header or an edge
//                  goes byte by byte.  Every record's string lies in a text of fgpu_stage3_join's layout (FastgRecView): the callers join first,
//                  a single-piece contig too, so one source serves.
#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/rocprim.hpp>
#include <string>

#include "fastg_name.h"
#include "fgpu_ctx.h"
#include "stage3_bits.h"

namespace {

static_assert(sizeof(fgpu_fastg_rec) == 32 && sizeof(fgpu_fastg_info) == 32, "the records as _lib.py and api.py lay them out");
static_assert(FGPU_FASTG_NAME_MAX < FGPU_FASTG_NAME_STRIDE - 1, "a name and its length in one entry");

constexpr uint32_t FASTG_TILE = FGPU_FASTG_TILE;     // 256 lanes x 16 bytes
constexpr uint32_t FASTG_TILE_RECORDS = 128;         // offsets kept per tile; 4096 / 57 + 2 = 73 records can touch one
static_assert(FASTG_TILE == 256 * 16, "one 16-byte store per lane");

struct FastgRecView {                            // a record's 2-bit string: fgpu_fastg_rec over a text in fgpu_stage3_join's layout
    const fgpu_fastg_rec* __restrict__ recs;
    const uint64_t* __restrict__ text;
    __device__ __forceinline__ const uint64_t* words(uint64_t i) const { return text + recs[i].text_word; }
    __device__ __forceinline__ uint32_t len(uint64_t i) const { return recs[i].len; }
};

__global__ void __launch_bounds__(256) k_fastg_names(const fgpu_fastg_rec* __restrict__ recs, uint64_t n, uint8_t* __restrict__ names) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const fgpu_fastg_rec r = recs[i];
    char* entry = (char*)names + i * FGPU_FASTG_NAME_STRIDE;
    entry[FGPU_FASTG_NAME_STRIDE - 1] = (char)fgpu_fastg_name(r.tig, r.len, r.cov_sum, r.cov_n, entry);
}

__device__ __forceinline__ uint32_t fastg_name_len(const uint8_t* __restrict__ names, uint64_t i) { return names[i * FGPU_FASTG_NAME_STRIDE + FGPU_FASTG_NAME_STRIDE - 1]; }

// hdr[2i], hdr[2i + 1]: the bytes of record i's primed and other header line, newline included; bytes[i]: of its four lines (entry n: 0, for the scan's total)
__global__ void __launch_bounds__(256) k_fastg_sizes(const fgpu_fastg_rec* __restrict__ recs, uint64_t n, const uint64_t* __restrict__ nbr_first,
                                                     const uint32_t* __restrict__ nbr, const uint8_t* __restrict__ names, uint32_t* __restrict__ hdr,
                                                     uint64_t* __restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { bytes[n] = 0; return; }
    const uint32_t own = fastg_name_len(names, i);
    uint64_t all = 2ULL * recs[i].len + 2;
    for (uint32_t h = 0; h < 2; h++) {
        const uint64_t a = nbr_first[2 * i + h], b = nbr_first[2 * i + h + 1];
        uint32_t bytes_h = 1 + own + (h == 0 ? 1 : 0) + 1 + 1;            // '>' name ['] ';' newline
        if (b > a) bytes_h += 1 + (uint32_t)(b - a) - 1;                  // ':' and a ',' between two
        for (uint64_t e = a; e < b; e++) {
            const uint32_t v = nbr[e];
            bytes_h += fastg_name_len(names, v & ~FGPU_FASTG_PRIMED) + (v >> 31);
        }
        hdr[2 * i + h] = bytes_h;
        all += bytes_h;
    }
    bytes[i] = all;
}

struct FastgTables {                             // what a header is put together from
    const uint64_t* __restrict__ nbr_first;
    const uint32_t* __restrict__ nbr;
    const uint8_t* __restrict__ names;
    const uint32_t* __restrict__ hdr;
};
struct FastgRecord {                             // what k_fastg_text knows of the record a byte lies in
    uint64_t i, first;                           // its number, its first byte
    const uint64_t* w;
    uint32_t len, h0, h1;                        // bases, bytes of the two header lines
};
__device__ __forceinline__ FastgRecord fastg_record(const FastgRecView& view, const FastgTables& t, uint64_t i, uint64_t first) {
    FastgRecord r;
    r.i = i;
    r.first = first;
    r.w = view.words(i);
    r.len = view.len(i);
    r.h0 = t.hdr[2 * i];
    r.h1 = t.hdr[2 * i + 1];
    return r;
}
__device__ __forceinline__ uint32_t fastg_letter(uint32_t code) { return (0x47544341u >> (8 * code)) & 0xFFu; }       // "ACTG"

// byte j of header line h (0: the primed one) of record i, which has `bytes` bytes
__device__ uint32_t fastg_header_byte(const FastgTables& t, uint64_t i, uint32_t h, uint32_t j, uint32_t bytes) {
    if (j == 0) return '>';
    if (j == bytes - 1) return '\n';
    j -= 1;
    const uint32_t own = fastg_name_len(t.names, i);
    if (j < own) return t.names[i * FGPU_FASTG_NAME_STRIDE + j];
    j -= own;
    if (h == 0) {
        if (j == 0) return '\'';
        j -= 1;
    }
    const uint64_t a = t.nbr_first[2 * i + h], b = t.nbr_first[2 * i + h + 1];
    if (a == b || j == 0) return a == b ? ';' : ':';
    j -= 1;
    for (uint64_t e = a; e < b; e++) {
        const uint32_t v = t.nbr[e];
        const uint64_t r = v & ~FGPU_FASTG_PRIMED;
        const uint32_t name = fastg_name_len(t.names, r);
        if (j < name) return t.names[r * FGPU_FASTG_NAME_STRIDE + j];
        j -= name;
        if (v >> 31) {
            if (j == 0) return '\'';
            j -= 1;
        }
        if (j == 0) return e + 1 == b ? ';' : ',';
        j -= 1;
    }
    return ';';                                  // (not reached: the line's last two bytes are ';' and the newline)
}
// byte `at` of the record's four lines
__device__ __forceinline__ uint32_t fastg_byte(const FastgTables& t, const FastgRecord& r, uint64_t at) {
    if (at < r.h0) return fastg_header_byte(t, r.i, 0, (uint32_t)at, r.h0);
    at -= r.h0;
    if (at < r.len) return fastg_letter((uint32_t)emit_oriented(r.w, r.len, false, (uint32_t)at) & 3);
    if (at == r.len) return '\n';
    at -= (uint64_t)r.len + 1;
    if (at < r.h1) return fastg_header_byte(t, r.i, 1, (uint32_t)at, r.h1);
    at -= r.h1;
    if (at < r.len) return fastg_letter((uint32_t)emit_oriented(r.w, r.len, true, (uint32_t)at) & 3);
    return '\n';
}

__global__ void __launch_bounds__(256) k_fastg_text(FastgRecView view, FastgTables t, uint64_t n, const uint64_t* __restrict__ byte0, uint64_t n_bytes, uint4* __restrict__ out) {
    __shared__ uint64_t first_of[FASTG_TILE_RECORDS];
    __shared__ uint64_t tile_first;
    const uint64_t tile = (uint64_t)blockIdx.x * FASTG_TILE;              // (< n_bytes by the grid)
    if (threadIdx.x == 0) tile_first = emit_find(byte0, n, tile);
    __syncthreads();
    const uint64_t i0 = tile_first;
    for (uint32_t s = threadIdx.x; s < FASTG_TILE_RECORDS; s += 256) first_of[s] = i0 + s <= n ? byte0[i0 + s] : ~0ULL;
    __syncthreads();
    const uint64_t at = tile + 16ULL * threadIdx.x;
    if (at >= n_bytes) return;
    uint32_t lo = 0, hi = FASTG_TILE_RECORDS;                             // first_of[lo] <= at < first_of[hi] (hi = the array's end: no record starts there)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first_of[mid] <= at) lo = mid; else hi = mid;
    }
    FastgRecord r = fastg_record(view, t, i0 + lo, first_of[lo]);
    uint32_t v[4] = {0, 0, 0, 0};
    const uint64_t in = at - r.first, second = (uint64_t)r.h0 + r.len + 1 + r.h1;      // where the second strand begins
    const bool forward = in >= r.h0 && in + 16 <= (uint64_t)r.h0 + r.len, backward = in >= second && in + 16 <= second + r.len;
    if (forward || backward) {                                            // sixteen bases of one strand
        const uint32_t c = (uint32_t)emit_oriented(r.w, r.len, backward, (uint32_t)(in - (backward ? second : r.h0)));
#pragma unroll
        for (int b = 0; b < 16; b++) v[b >> 2] |= fastg_letter((c >> (2 * b)) & 3) << (8 * (b & 3));
    } else {
        for (uint32_t b = 0; b < 16 && at + b < n_bytes; b++) {           // (behind the last byte: zeros, in the buffer's own padding)
            while (lo + 1 < FASTG_TILE_RECORDS && first_of[lo + 1] <= at + b) {
                lo++;
                r = fastg_record(view, t, i0 + lo, first_of[lo]);
            }
            v[b >> 2] |= fastg_byte(t, r, at + b - r.first) << (8 * (b & 3));
        }
    }
    out[at >> 4] = make_uint4(v[0], v[1], v[2], v[3]);
}

struct FastgScratch {                            // device memory of one call, gone when it returns
    void* p = nullptr;
    ~FastgScratch() { if (p) (void)hipFree(p); }
};
inline uint64_t fastg_take(uint64_t& at, uint64_t bytes) {
    const uint64_t here = at;
    at += (bytes + 15) & ~15ULL;
    return here;
}
int fastg_alloc(fgpu_ctx* ctx, void** p, uint64_t bytes, const char* what) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        *p = nullptr;
        ctx->err = std::string("fgpu_stage3_fastg: hipMalloc of ") + std::to_string(bytes) + " bytes (" + what + ") failed: " + hipGetErrorString(e);
        return FGPU_ERR_NOMEM;
    }
    return FGPU_OK;
}

}  // namespace

extern "C" int fgpu_stage3_fastg(fgpu_ctx* ctx, const fgpu_fastg_rec* recs_host, uint64_t n, const uint64_t* nbr_first, const uint32_t* nbr, uint64_t n_nbr,
                                 const uint64_t* text_host, uint64_t text_words, uint64_t* bytes) {
    if (!ctx || !bytes || (n && (!recs_host || !nbr_first)) || (n_nbr && !nbr) || (text_host == nullptr && text_words != 0) || n >= (uint64_t)FGPU_FASTG_PRIMED)
        return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_fastg while a pass is open"; return FGPU_ERR_STATE; }
    *bytes = 0;
    const uint64_t* d_text = nullptr;
    if (!text_host && n) {
        if (!fgpu_s3j_text(ctx, &d_text)) { ctx->err = "fgpu_stage3_fastg without a text: no fgpu_stage3_join whose results are still on the device"; return FGPU_ERR_STATE; }
        text_words = ctx->s3j_totals[0];
    }
    for (uint64_t i = 0; i < n; i++) {           // every word and every table entry the kernels will read lies where they look for it
        const fgpu_fastg_rec& r = recs_host[i];
        if (r.len < 1 || r.len >= (1u << 31) || r.text_word > text_words || ((uint64_t)r.len + 31) / 32 > text_words - r.text_word) {
            ctx->err = "fgpu_stage3_fastg: record " + std::to_string(i) + " reaches past the text, or has no bases or 2^31 and more";
            return FGPU_ERR_ARG;
        }
        if (r.cov_n < 1 || r.cov_sum > 255ULL * r.cov_n) {
            ctx->err = "fgpu_stage3_fastg: record " + std::to_string(i) + " has a coverage summary of no entries, or a sum no list of bytes has";
            return FGPU_ERR_ARG;
        }
    }
    bool csr = !n || nbr_first[0] == 0;
    for (uint64_t i = 0; csr && i < 2 * n; i++) csr = nbr_first[i + 1] >= nbr_first[i] && nbr_first[i + 1] - nbr_first[i] <= 4 && nbr_first[i + 1] <= n_nbr;
    if (!csr || (n ? nbr_first[2 * n] : 0) != n_nbr) {
        ctx->err = "fgpu_stage3_fastg: the neighbour lists are no CSR of 2 n lists of at most four entries over n_nbr entries";
        return FGPU_ERR_ARG;
    }
    for (uint64_t e = 0; e < n_nbr; e++)
        if ((nbr[e] & ~FGPU_FASTG_PRIMED) >= n) {
            ctx->err = "fgpu_stage3_fastg: neighbour entry " + std::to_string(e) + " names a record that is none";
            return FGPU_ERR_ARG;
        }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->s3f_out) { (void)hipFree(ctx->s3f_out); ctx->s3f_out = nullptr; }       // a file nobody took
    ctx->s3f_bytes = 0;
    if (!n) return FGPU_OK;
    int rc;
    size_t scan_bytes = 0;
    FGPU_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    FastgScratch work;
    uint64_t at = 0;
    const uint64_t o_recs = fastg_take(at, n * sizeof(fgpu_fastg_rec)), o_first = fastg_take(at, (2 * n + 1) * 8), o_nbr = fastg_take(at, n_nbr * 4),
                   o_names = fastg_take(at, n * FGPU_FASTG_NAME_STRIDE), o_hdr = fastg_take(at, 2 * n * 4), o_cnt = fastg_take(at, (n + 1) * 8),
                   o_off = fastg_take(at, (n + 1) * 8), o_scan = fastg_take(at, scan_bytes), o_text = fastg_take(at, text_host ? text_words * 8 : 0);
    if ((rc = fastg_alloc(ctx, &work.p, at, "the records"))) return rc;
    char* wb = (char*)work.p;
    fgpu_fastg_rec* d_recs = (fgpu_fastg_rec*)(wb + o_recs);
    uint64_t *d_first = (uint64_t*)(wb + o_first), *d_bytes = (uint64_t*)(wb + o_cnt), *d_byte0 = (uint64_t*)(wb + o_off);
    uint32_t *d_nbr = (uint32_t*)(wb + o_nbr), *d_hdr = (uint32_t*)(wb + o_hdr);
    uint8_t* d_names = (uint8_t*)(wb + o_names);
    FGPU_HIP(hipMemcpyAsync(d_recs, recs_host, n * sizeof(fgpu_fastg_rec), hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_first, nbr_first, (2 * n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n_nbr) FGPU_HIP(hipMemcpyAsync(d_nbr, nbr, n_nbr * 4, hipMemcpyHostToDevice, ctx->stream));
    if (text_host) {
        FGPU_HIP(hipMemcpyAsync(wb + o_text, text_host, text_words * 8, hipMemcpyHostToDevice, ctx->stream));
        d_text = (const uint64_t*)(wb + o_text);
    }
    FGPU_LAUNCH("s3g_names", k_fastg_names, fgpu_blocks(n, 256), 256, (const fgpu_fastg_rec*)d_recs, n, d_names);
    FGPU_LAUNCH("s3g_sizes", k_fastg_sizes, fgpu_blocks(n + 1, 256), 256, (const fgpu_fastg_rec*)d_recs, n, (const uint64_t*)d_first, (const uint32_t*)d_nbr,
                (const uint8_t*)d_names, d_hdr, d_bytes);
    FGPU_HIP(rocprim::exclusive_scan(wb + o_scan, scan_bytes, d_bytes, d_byte0, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t n_bytes = 0;
    FGPU_HIP(hipMemcpyAsync(&n_bytes, d_byte0 + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    void* out = nullptr;
    if ((rc = fastg_alloc(ctx, &out, (n_bytes + 15) & ~15ULL, "the file"))) return rc;      // (whole 16-byte stores)
    ctx->s3f_out = out;                          // (freed with the context from here on)
    const FastgRecView view = {d_recs, d_text};
    const FastgTables tables = {d_first, d_nbr, d_names, d_hdr};
    FGPU_LAUNCH("s3g_text", k_fastg_text, fgpu_blocks(n_bytes, FASTG_TILE), 256, view, tables, n, (const uint64_t*)d_byte0, n_bytes, (uint4*)out);
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    *bytes = ctx->s3f_bytes = n_bytes;
    return FGPU_OK;
}
