// stage3_emit.hip — Stage 3's first product on the device: the contigs of a build, joined, oriented and printed as FASTA where they lie
// (fgpu_stage3_fasta, fgpu_stage3_fasta_take, fgpu_stage3_raw_contigs; include/faucet_gpu.h) -- and its second, the contigs after the first
// cleaning step, printed from the strings fgpu_stage3_join left on the device (fgpu_stage3_fasta_joined, fgpu_stage3_detip,
// fgpu_stage3_graph_take), and likewise after the second step (fgpu_stage3_dechimera), which works on the graph the first one left: the
// context keeps the live graph object (clean_graph.h) between the steps, and nothing of it is made again.  The graph itself as FASTG
// (fgpu_stage3_raw_graph, fgpu_stage3_graph_fastg, at the end of this file) is put together here too: the walk is clean_graph.h's, the kernels
// stage3_fastg.hip's.
//
// What the reference does per record, ContigGraph::printContigs (src/ContigGraph.cpp:1532-1645):
//   ContigJuncList::concatenate's sequence          utils/ContigJuncList.cpp:121   first.substr(0, len - k) + second
//   ContigJuncList::reverse / revcomp_string        utils/ContigJuncList.cpp:98-103, utils/Kmer.cpp:353-359
//   canon_contig                                    utils/Kmer.cpp:345-351         a comparison of strings of LETTERS: A < C < G < T
// Which records, and in which order, is the host's business (raw_plan.cpp).  Four kernels, integer and bitwise only:
//   k_emit_sizes   per record: words of its joined 2-bit string, bytes of its text (">Contig<n>\n" + bases + "\n"); rocPRIM scans them
//   k_emit_join    one lane per WORD of the joined strings: 32 bases cut out of one or two pieces at any base offset by funnel shifts, a
//                  reverse complement 32 bases at a time (bit reversal, pair swap, XOR 1010...: the complement of a code is code ^ 2)
//   k_emit_canon   one wave per record: the first position where the string and its reverse complement differ, 32 x 64 bases per step, found
//                  with a ballot; the ranks of the two letters there decide.  A palindrome never differs and stays.
//   k_emit_ascii   one block per 4 KiB of OUTPUT, one lane per 16 bytes, whatever the records' lengths: the block looks up its first
//                  record once, keeps the byte offsets of the records its tile can touch in LDS, a lane inside a sequence expands 16 codes
//                  and stores 16 bytes at once, a lane on a header or a record's edge goes byte by byte.
// k_emit_canon and k_emit_ascii take a record as (first word, bases, number) from a view: EmitSeqView over k_emit_join's strings, EmitJoinedView over
// fgpu_joined records and any text in the same layout -- a join's text is one, so fgpu_stage3_fasta_joined has no join kernel, and of the
// sizes only the bytes (k_emit_sizes_joined).  Which lists are joined is the host's business again (tips_plan.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <rocprim/rocprim.hpp>
#include <string>
#include <vector>

#include "clean_graph.h"
#include "fgpu_ctx.h"
#include "stage3_bits.h"

namespace {

static_assert(sizeof(fgpu_fasta_seq) == 32 && sizeof(fgpu_raw_info) == 48 && sizeof(fgpu_chimera_info) == 184, "the records as api.py and _lib.py lay them out");
static_assert(sizeof(fgpu_tips_node) == 32 && sizeof(fgpu_tips_contig) == 32 && sizeof(fgpu_tips_info) == 112 && sizeof(fgpu_tips_out) == 136, "... likewise");

constexpr uint32_t EMIT_TILE = 4096;             // bytes of output per block of k_emit_ascii: 256 lanes x 16 bytes
constexpr uint32_t EMIT_TILE_RECORDS = 512;      // offsets kept per tile: a record has at least 11 bytes (">Contig1\n", a base, "\n"), so a tile touches at most 374

__device__ __forceinline__ uint32_t emit_joined_len(const fgpu_fasta_seq& s, int k) { return s.pieces == 2 ? s.len[0] - (uint32_t)k + s.len[1] : s.len[0]; }
__device__ __forceinline__ uint32_t emit_digits(uint32_t v) {
    uint32_t d = 1;
    for (uint32_t p = 10; d < 10 && v >= p; p *= 10) d++;      // (p overflows only behind d == 10, where the loop has ended)
    return d;
}

// What k_emit_canon and k_emit_ascii know of record i: where its 2-bit string begins, its bases and its number.  Two sources:
struct EmitSeqView {                             // fgpu_stage3_fasta: the strings k_emit_join made of the records' pieces
    const fgpu_fasta_seq* __restrict__ seqs;
    const uint64_t* __restrict__ word0;
    const uint64_t* __restrict__ joined;
    int k;
    __device__ __forceinline__ const uint64_t* words(uint64_t i) const { return joined + word0[i]; }
    __device__ __forceinline__ uint32_t len(uint64_t i) const { return emit_joined_len(seqs[i], k); }
    __device__ __forceinline__ uint32_t number(uint64_t i) const { return seqs[i].number; }
};
struct EmitJoinedView {                          // fgpu_stage3_fasta_joined: fgpu_stage3_join's strings where they lie -- already in this layout
    const fgpu_joined* __restrict__ recs;
    const uint32_t* __restrict__ numbers;
    const uint64_t* __restrict__ text;
    __device__ __forceinline__ const uint64_t* words(uint64_t i) const { return text + recs[i].text_word; }
    __device__ __forceinline__ uint32_t len(uint64_t i) const { return recs[i].len; }
    __device__ __forceinline__ uint32_t number(uint64_t i) const { return numbers[i]; }
};

__global__ void __launch_bounds__(256) k_emit_sizes(const fgpu_fasta_seq* __restrict__ seqs, uint64_t n, int k, uint64_t* __restrict__ words, uint64_t* __restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) { words[n] = 0; bytes[n] = 0; return; }      // (the scans' last entry: the totals)
    const fgpu_fasta_seq s = seqs[i];
    const uint32_t len = emit_joined_len(s, k);
    words[i] = (len + 31) >> 5;
    bytes[i] = 8ULL + emit_digits(s.number) + len + 1;
}

__global__ void __launch_bounds__(256) k_emit_sizes_joined(const fgpu_joined* __restrict__ recs, const uint32_t* __restrict__ numbers, uint64_t n, uint64_t* __restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    bytes[i] = i == n ? 0 : 8ULL + emit_digits(numbers[i]) + recs[i].len + 1;      // (entry n: the scan's total)
}

__global__ void __launch_bounds__(256) k_emit_join(const fgpu_fasta_seq* __restrict__ seqs, uint64_t n, int k, const uint64_t* __restrict__ text,
                                                   const uint64_t* __restrict__ word0, uint64_t n_words, uint64_t* __restrict__ joined) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_words) return;
    const uint64_t i = emit_find(word0, n, g);
    const fgpu_fasta_seq s = seqs[i];
    const uint32_t len = emit_joined_len(s, k), pos = (uint32_t)(g - word0[i]) * 32;
    const int last = s.pieces == 2 ? 1 : 0;
    const uint32_t cut = s.pieces == 2 ? s.len[0] - (uint32_t)k : 0;       // bases the first piece gives
    const uint64_t* tail = text + s.text_word[last];
    uint64_t w;
    if (pos >= cut) {
        w = emit_oriented(tail, s.len[last], s.flip[last] != 0, pos - cut);
    } else {
        w = emit_oriented(text + s.text_word[0], s.len[0], s.flip[0] != 0, pos);
        if (pos + 32 > cut) {                                              // the seam falls into this word
            const uint32_t n1 = cut - pos;
            w = (w & emit_low_fields(n1)) | (emit_oriented(tail, s.len[1], s.flip[1] != 0, 0) << (2 * n1));
        }
    }
    joined[g] = w & emit_low_fields(len - pos);
}

template <class View>
__global__ void __launch_bounds__(256) k_emit_canon(View view, uint64_t n, uint8_t* __restrict__ flipped) {
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per record (uniform within the wave)
    if (i >= n) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t len = view.len(i), words = (len + 31) >> 5;
    const uint64_t* w = view.words(i);
    for (uint32_t j0 = 0; j0 < words; j0 += 64) {
        const uint32_t j = j0 + lane;
        uint64_t own = 0, other = 0;
        if (j < words) {
            const uint64_t valid = emit_low_fields(len - 32 * j);
            own = w[j] & valid;
            other = emit_oriented(w, len, true, 32 * j) & valid;
        }
        const uint64_t differ = own ^ other;
        const unsigned long long who = __ballot(differ != 0);
        if (who) {                                                         // (wave-uniform: every lane leaves together)
            if (lane == (uint32_t)(__ffsll((long long)who) - 1)) {
                const uint32_t f = (uint32_t)(__ffsll((long long)differ) - 1) >> 1;
                const uint32_t a = (uint32_t)(own >> (2 * f)) & 3, b = (uint32_t)(other >> (2 * f)) & 3;
                flipped[i] = ((a ^ (a >> 1)) > (b ^ (b >> 1))) ? 1 : 0;    // codes A 0, C 1, T 2, G 3 -> ranks of the letters 0, 1, 3, 2
            }
            return;
        }
    }
    if (lane == 0) flipped[i] = 0;                                         // its own reverse complement
}

struct EmitRecord {                              // what k_emit_ascii knows of the record a byte lies in
    uint64_t first;                              // its first byte
    const uint64_t* w;
    uint32_t len, number, digits;
    bool flip;
};
template <class View>
__device__ __forceinline__ EmitRecord emit_record(const View& view, uint64_t i, const uint8_t* __restrict__ flipped, uint64_t first) {
    EmitRecord r;
    r.first = first;
    r.w = view.words(i);
    r.len = view.len(i);
    r.number = view.number(i);
    r.digits = emit_digits(r.number);
    r.flip = flipped[i] != 0;
    return r;
}
__device__ __forceinline__ uint32_t emit_letter(uint32_t code) { return (0x47544341u >> (8 * code)) & 0xFFu; }       // "ACTG"
__device__ __forceinline__ uint32_t emit_byte(const EmitRecord& r, uint32_t at) {      // byte `at` of the record's text
    if (at < 7) return (uint32_t)">Contig"[at];
    if (at < 7 + r.digits) {
        uint32_t v = r.number;
        for (uint32_t d = 7 + r.digits - 1 - at; d; d--) v /= 10;
        return '0' + v % 10;
    }
    const uint32_t base = at - (8 + r.digits);
    if (at == 7 + r.digits || base >= r.len) return '\n';
    return emit_letter((uint32_t)emit_oriented(r.w, r.len, r.flip, base) & 3);
}

template <class View>
__global__ void __launch_bounds__(256) k_emit_ascii(View view, uint64_t n, const uint64_t* __restrict__ byte0, uint64_t n_bytes, const uint8_t* __restrict__ flipped,
                                                    uint4* __restrict__ out) {
    __shared__ uint64_t first_of[EMIT_TILE_RECORDS];
    __shared__ uint64_t tile_first;
    const uint64_t tile = (uint64_t)blockIdx.x * EMIT_TILE;               // (< n_bytes by the grid)
    if (threadIdx.x == 0) tile_first = emit_find(byte0, n, tile);
    __syncthreads();
    const uint64_t i0 = tile_first;
    for (uint32_t t = threadIdx.x; t < EMIT_TILE_RECORDS; t += 256) first_of[t] = i0 + t <= n ? byte0[i0 + t] : ~0ULL;
    __syncthreads();
    const uint64_t at = tile + 16ULL * threadIdx.x;
    if (at >= n_bytes) return;
    uint32_t lo = 0, hi = EMIT_TILE_RECORDS;                               // first_of[lo] <= at < first_of[hi] (hi = the array's end: no record starts there)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first_of[mid] <= at) lo = mid; else hi = mid;
    }
    EmitRecord r = emit_record(view, i0 + lo, flipped, first_of[lo]);
    uint32_t v[4] = {0, 0, 0, 0};
    const uint64_t in = at - r.first, bases = 8 + r.digits;
    if (in >= bases && in + 16 <= bases + r.len) {                         // sixteen bases of one sequence
        const uint32_t c = (uint32_t)emit_oriented(r.w, r.len, r.flip, (uint32_t)(in - bases));
#pragma unroll
        for (int b = 0; b < 16; b++) v[b >> 2] |= emit_letter((c >> (2 * b)) & 3) << (8 * (b & 3));
    } else {
        for (uint32_t b = 0; b < 16 && at + b < n_bytes; b++) {            // (behind the last byte: zeros, in the buffer's own padding)
            while (lo + 1 < EMIT_TILE_RECORDS && first_of[lo + 1] <= at + b) {
                lo++;
                r = emit_record(view, i0 + lo, flipped, first_of[lo]);
            }
            v[b >> 2] |= emit_byte(r, (uint32_t)(at + b - r.first)) << (8 * (b & 3));
        }
    }
    out[at >> 4] = make_uint4(v[0], v[1], v[2], v[3]);
}

struct EmitScratch {                             // device memory of one call, gone when it returns
    void* p = nullptr;
    ~EmitScratch() { if (p) (void)hipFree(p); }
};
inline uint64_t emit_take(uint64_t& at, uint64_t bytes) {
    const uint64_t here = at;
    at += (bytes + 15) & ~15ULL;
    return here;
}
int emit_alloc(fgpu_ctx* ctx, void** p, uint64_t bytes, const char* what) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        *p = nullptr;
        ctx->err = std::string("fgpu_stage3_fasta: hipMalloc of ") + std::to_string(bytes) + " bytes (" + what + ") failed: " + hipGetErrorString(e);
        return FGPU_ERR_NOMEM;
    }
    return FGPU_OK;
}
void emit_drop(fgpu_ctx* ctx) {                  // a file nobody took
    if (ctx->s3f_out) { (void)hipFree(ctx->s3f_out); ctx->s3f_out = nullptr; }
    ctx->s3f_bytes = 0;
}

}  // namespace

extern "C" int fgpu_stage3_fasta(fgpu_ctx* ctx, const fgpu_fasta_seq* seqs_host, uint64_t n, const uint64_t* text_host, uint64_t text_words, uint64_t* bytes) {
    if (!ctx || !bytes || (n && !seqs_host) || (text_host == nullptr && text_words != 0)) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_fasta while a pass is open"; return FGPU_ERR_STATE; }
    *bytes = 0;
    const int k = ctx->prm.k;
    const uint64_t* d_text = nullptr;
    if (!text_host && n) {
        if (!fgpu_s3b_view(ctx, nullptr, nullptr, &d_text)) { ctx->err = "fgpu_stage3_fasta without a text: no fgpu_stage3_build whose results are still on the device"; return FGPU_ERR_STATE; }
        text_words = ctx->s3b_totals[1];
    }
    for (uint64_t i = 0; i < n; i++) {           // every word the kernels will read lies in the text
        const fgpu_fasta_seq& s = seqs_host[i];
        bool ok = s.pieces == 1 || s.pieces == 2;
        for (int p = 0; ok && p < s.pieces; p++)
            ok = s.len[p] >= 1 && s.len[p] < (1u << 30) && s.text_word[p] <= text_words && ((uint64_t)s.len[p] + 31) / 32 <= text_words - s.text_word[p];
        if (ok && s.pieces == 2) ok = s.len[0] >= (uint32_t)k;
        if (!ok) {
            ctx->err = "fgpu_stage3_fasta: record " + std::to_string(i) + " has a piece outside the text, of no bases or of 2^30 and more, a first piece shorter than k, or pieces other than 1 or 2";
            return FGPU_ERR_ARG;
        }
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    emit_drop(ctx);
    if (!n) return FGPU_OK;
    int rc;
    size_t scan_bytes = 0;
    FGPU_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    EmitScratch work;
    uint64_t at = 0;
    const uint64_t o_seqs = emit_take(at, n * sizeof(fgpu_fasta_seq)), o_cnt = emit_take(at, 2 * (n + 1) * 8), o_off = emit_take(at, 2 * (n + 1) * 8),
                   o_scan = emit_take(at, scan_bytes), o_flip = emit_take(at, n), o_text = emit_take(at, text_host ? text_words * 8 : 0);
    if ((rc = emit_alloc(ctx, &work.p, at, "the records"))) return rc;
    char* wb = (char*)work.p;
    fgpu_fasta_seq* d_seqs = (fgpu_fasta_seq*)(wb + o_seqs);
    uint64_t *d_words = (uint64_t*)(wb + o_cnt), *d_bytes = d_words + (n + 1), *d_word0 = (uint64_t*)(wb + o_off), *d_byte0 = d_word0 + (n + 1);
    uint8_t* d_flip = (uint8_t*)(wb + o_flip);
    FGPU_HIP(hipMemcpyAsync(d_seqs, seqs_host, n * sizeof(fgpu_fasta_seq), hipMemcpyHostToDevice, ctx->stream));
    if (text_host) {
        FGPU_HIP(hipMemcpyAsync(wb + o_text, text_host, text_words * 8, hipMemcpyHostToDevice, ctx->stream));
        d_text = (const uint64_t*)(wb + o_text);
    }
    FGPU_LAUNCH("s3f_sizes", k_emit_sizes, fgpu_blocks(n + 1, 256), 256, (const fgpu_fasta_seq*)d_seqs, n, k, d_words, d_bytes);
    FGPU_HIP(rocprim::exclusive_scan(wb + o_scan, scan_bytes, d_words, d_word0, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    FGPU_HIP(rocprim::exclusive_scan(wb + o_scan, scan_bytes, d_bytes, d_byte0, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t n_words = 0, n_bytes = 0;
    FGPU_HIP(hipMemcpyAsync(&n_words, d_word0 + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&n_bytes, d_byte0 + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    EmitScratch joined;
    if ((rc = emit_alloc(ctx, &joined.p, n_words * 8, "the joined strings"))) return rc;
    void* out = nullptr;
    if ((rc = emit_alloc(ctx, &out, (n_bytes + 15) & ~15ULL, "the file"))) return rc;      // (whole 16-byte stores)
    ctx->s3f_out = out;                          // (freed with the context from here on)
    FGPU_LAUNCH("s3f_join", k_emit_join, fgpu_blocks(n_words, 256), 256, (const fgpu_fasta_seq*)d_seqs, n, k, d_text, (const uint64_t*)d_word0, n_words, (uint64_t*)joined.p);
    const EmitSeqView view = {d_seqs, d_word0, (const uint64_t*)joined.p, k};
    FGPU_LAUNCH("s3f_canon", k_emit_canon<EmitSeqView>, fgpu_blocks(n, 4), 256, view, n, d_flip);
    FGPU_LAUNCH("s3f_ascii", k_emit_ascii<EmitSeqView>, fgpu_blocks(n_bytes, EMIT_TILE), 256, view, n, (const uint64_t*)d_byte0, n_bytes, (const uint8_t*)d_flip, (uint4*)out);
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    *bytes = ctx->s3f_bytes = n_bytes;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_fasta_take(fgpu_ctx* ctx, char* out, uint64_t bytes) {
    if (!ctx) return FGPU_ERR_ARG;
    if (bytes < ctx->s3f_bytes || (ctx->s3f_bytes && !out)) {
        ctx->err = "fgpu_stage3_fasta_take: the buffer is smaller than the bytes fgpu_stage3_fasta gave";
        return FGPU_ERR_ARG;
    }
    if (!ctx->s3f_out) return FGPU_OK;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->s3f_bytes) FGPU_HIP(hipMemcpyAsync(out, ctx->s3f_out, ctx->s3f_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    emit_drop(ctx);
    return FGPU_OK;
}

extern "C" int fgpu_stage3_fasta_joined(fgpu_ctx* ctx, const fgpu_joined* joined_host, const uint32_t* numbers_host, uint64_t n, const uint64_t* text_host,
                                        uint64_t text_words, uint64_t* bytes) {
    if (!ctx || !bytes || (n && (!joined_host || !numbers_host)) || (text_host == nullptr && text_words != 0) || n >= (1ULL << 32)) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_fasta_joined while a pass is open"; return FGPU_ERR_STATE; }
    *bytes = 0;
    const uint64_t* d_text = nullptr;
    if (!text_host && n) {
        if (!fgpu_s3j_text(ctx, &d_text)) { ctx->err = "fgpu_stage3_fasta_joined without a text: no fgpu_stage3_join whose results are still on the device"; return FGPU_ERR_STATE; }
        text_words = ctx->s3j_totals[0];
    }
    for (uint64_t i = 0; i < n; i++) {           // every word the kernels will read lies in the text
        const fgpu_joined& r = joined_host[i];
        if (r.len < 1 || r.len >= (1u << 31) || r.text_word > text_words || ((uint64_t)r.len + 31) / 32 > text_words - r.text_word) {
            ctx->err = "fgpu_stage3_fasta_joined: record " + std::to_string(i) + " reaches past the text, or has no bases or 2^31 and more";
            return FGPU_ERR_ARG;
        }
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    emit_drop(ctx);
    if (!n) return FGPU_OK;
    int rc;
    size_t scan_bytes = 0;
    FGPU_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    EmitScratch work;
    uint64_t at = 0;
    const uint64_t o_recs = emit_take(at, n * sizeof(fgpu_joined)), o_num = emit_take(at, n * 4), o_cnt = emit_take(at, (n + 1) * 8), o_off = emit_take(at, (n + 1) * 8),
                   o_scan = emit_take(at, scan_bytes), o_flip = emit_take(at, n), o_text = emit_take(at, text_host ? text_words * 8 : 0);
    if ((rc = emit_alloc(ctx, &work.p, at, "the records"))) return rc;
    char* wb = (char*)work.p;
    fgpu_joined* d_recs = (fgpu_joined*)(wb + o_recs);
    uint32_t* d_num = (uint32_t*)(wb + o_num);
    uint64_t *d_bytes = (uint64_t*)(wb + o_cnt), *d_byte0 = (uint64_t*)(wb + o_off);
    uint8_t* d_flip = (uint8_t*)(wb + o_flip);
    FGPU_HIP(hipMemcpyAsync(d_recs, joined_host, n * sizeof(fgpu_joined), hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_num, numbers_host, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (text_host) {
        FGPU_HIP(hipMemcpyAsync(wb + o_text, text_host, text_words * 8, hipMemcpyHostToDevice, ctx->stream));
        d_text = (const uint64_t*)(wb + o_text);
    }
    FGPU_LAUNCH("s3f_sizes_joined", k_emit_sizes_joined, fgpu_blocks(n + 1, 256), 256, (const fgpu_joined*)d_recs, (const uint32_t*)d_num, n, d_bytes);
    FGPU_HIP(rocprim::exclusive_scan(wb + o_scan, scan_bytes, d_bytes, d_byte0, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t n_bytes = 0;
    FGPU_HIP(hipMemcpyAsync(&n_bytes, d_byte0 + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    void* out = nullptr;
    if ((rc = emit_alloc(ctx, &out, (n_bytes + 15) & ~15ULL, "the file"))) return rc;      // (whole 16-byte stores)
    ctx->s3f_out = out;                          // (freed with the context from here on)
    const EmitJoinedView view = {d_recs, d_num, d_text};
    FGPU_LAUNCH("s3f_canon_joined", k_emit_canon<EmitJoinedView>, fgpu_blocks(n, 4), 256, view, n, d_flip);
    FGPU_LAUNCH("s3f_ascii_joined", k_emit_ascii<EmitJoinedView>, fgpu_blocks(n_bytes, EMIT_TILE), 256, view, n, (const uint64_t*)d_byte0, n_bytes, (const uint8_t*)d_flip, (uint4*)out);
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    *bytes = ctx->s3f_bytes = n_bytes;
    return FGPU_OK;
}

namespace {

struct EmitBuild {                               // the record arrays of the build and the map, on the host
    std::vector<fgpu_contig> contigs;
    std::vector<fgpu_build_call> calls;
    std::vector<uint64_t> keys;
    std::vector<fgpu_junction> recs;
};
// what fgpu_stage3_raw_contigs and fgpu_stage3_detip ask of the context, and the two record arrays of the build (no text, no list) brought over
int emit_build_records(fgpu_ctx* ctx, const std::string& who, EmitBuild& b) {
    const fgpu_contig* d_contigs = nullptr;
    const fgpu_build_call* d_calls = nullptr;
    if (!fgpu_s3b_view(ctx, &d_contigs, &d_calls, nullptr)) {
        ctx->err = who + ": no fgpu_stage3_build whose results are still on the device (not run, or taken)";
        return FGPU_ERR_ARG;
    }
    if (ctx->s3b_status != 0) {
        ctx->err = who + ": the build stopped with status " + std::to_string(ctx->s3b_status) + " at call " + std::to_string(ctx->s3b_totals[0]) +
                   ": the reference does not return from JunctionMap::buildContigGraph on this map";
        return FGPU_ERR_ARG;
    }
    if (ctx->phase != 0) { ctx->err = who + " while a pass is open"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const uint64_t n_calls = ctx->s3b_totals[0], nj = ctx->s3_count;
    b.contigs.resize(n_calls); b.calls.resize(n_calls); b.keys.resize(nj); b.recs.resize(nj);
    if (n_calls) {
        FGPU_HIP(hipMemcpyAsync(b.contigs.data(), d_contigs, n_calls * sizeof(fgpu_contig), hipMemcpyDeviceToHost, ctx->stream));
        FGPU_HIP(hipMemcpyAsync(b.calls.data(), d_calls, n_calls * sizeof(fgpu_build_call), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nj) {                                    // the map as fgpu_stage3_set_junctions was handed it, in its order
        const uint64_t* d_keys = (const uint64_t*)((const char*)ctx->s3_in.p + 64);
        FGPU_HIP(hipMemcpyAsync(b.keys.data(), d_keys, nj * 8, hipMemcpyDeviceToHost, ctx->stream));
        FGPU_HIP(hipMemcpyAsync(b.recs.data(), d_keys + nj, nj * sizeof(fgpu_junction), hipMemcpyDeviceToHost, ctx->stream));
    }
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}
// the print records of a cleaned graph (clean_graph.h) on the host, and the file made of them on the device
struct EmitPrint {
    std::vector<uint64_t> first;
    std::vector<uint32_t> numbers;
    std::vector<fgpu_join_piece> pieces;
    uint64_t n = 0, n_pieces = 0;
    // printContigs' two passes: a plan status.  Room that suffices unless a contig is copied (a call lies in one contig of the graph, a bubble's
    // back in at most four records); asked again if not
    int of(fgpu_graph::CleanGraph& cg, uint64_t n_calls, fgpu_raw_info& info) {
        first.resize(n_calls + 1); numbers.resize(n_calls); pieces.resize(2 * n_calls);
        int st = FGPU_PLAN_SHORT;
        for (int pass = 0; pass < 2 && st == FGPU_PLAN_SHORT; pass++) {
            if (pass) { first.resize(n + 1); numbers.resize(n); pieces.resize(n_pieces); }
            fgpu_tips_out out;
            memset(&out, 0, sizeof(out));
            out.print_first = first.data(); out.print_number = numbers.data(); out.print_cap = numbers.size();
            out.print_pieces = pieces.data(); out.print_pieces_cap = pieces.size();
            st = cg.print_records(&out, info);
            n = out.n_print; n_pieces = out.n_print_pieces;
        }
        return st;
    }
    // fgpu_stage3_join of the records' lists over the build where it lies, fgpu_stage3_fasta_joined of the joined text where it lies
    int emit(fgpu_ctx* ctx, uint64_t* bytes) {
        std::vector<fgpu_joined> joined(n);
        uint64_t totals[3];
        if (int rc = fgpu_stage3_join(ctx, first.data(), n, pieces.data(), n_pieces, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, joined.data(), totals)) return rc;
        return fgpu_stage3_fasta_joined(ctx, joined.data(), numbers.data(), n, nullptr, 0, bytes);
    }
};
int emit_plan_failed(fgpu_ctx* ctx, const std::string& who, const char* plan, const char* unset, int st) {
    ctx->err = st == FGPU_PLAN_UNSET ? who + ": on this graph " + unset + " (undefined in the reference)"
                                     : who + ": the build's records are not a finished build of the map (" + plan + " status " + std::to_string(st) + ")";
    return FGPU_ERR_STATE;
}

}  // namespace

extern "C" int fgpu_stage3_raw_contigs(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_raw_info* info) {
    if (!ctx || !bytes) return FGPU_ERR_ARG;
    *bytes = 0;
    if (info) memset(info, 0, sizeof(*info));
    EmitBuild b;
    if (int rc = emit_build_records(ctx, "fgpu_stage3_raw_contigs", b)) return rc;
    const uint64_t n_calls = b.contigs.size();
    std::vector<fgpu_fasta_seq> seqs(n_calls);
    uint64_t n = 0;
    fgpu_raw_info inf;
    memset(&inf, 0, sizeof(inf));
    const int st = fgpu_raw_plan(b.keys.data(), b.recs.data(), b.keys.size(), b.contigs.data(), b.calls.data(), n_calls, ctx->prm.k, read_length, seqs.data(), n_calls, &n, &inf);
    if (st != FGPU_PLAN_OK) return emit_plan_failed(ctx, "fgpu_stage3_raw_contigs", "fgpu_raw_plan", "ContigGraph::printContigs reads a contig pointer that was never set", st);
    if (int rc = fgpu_stage3_fasta(ctx, seqs.data(), n, nullptr, 0, bytes)) return rc;
    if (info) *info = inf;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_detip(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_tips_info* info) {
    if (!ctx || !bytes) return FGPU_ERR_ARG;
    *bytes = 0;
    if (info) memset(info, 0, sizeof(*info));
    EmitBuild b;
    if (int rc = emit_build_records(ctx, "fgpu_stage3_detip", b)) return rc;
    const char* unset = "ContigGraph::deleteTipsAndClean or printContigs goes through a pointer that was never set or whose target is gone";
    std::shared_ptr<fgpu_graph::CleanGraph> cg = std::make_shared<fgpu_graph::CleanGraph>();
    fgpu_tips_info inf;
    memset(&inf, 0, sizeof(inf));
    int st = cg->of_build(b.keys.data(), b.recs.data(), b.keys.size(), b.contigs.data(), b.calls.data(), b.contigs.size(), nullptr, ctx->prm.k, read_length);
    if (st == FGPU_PLAN_OK) st = cg->delete_tips_and_clean(inf);
    EmitPrint pr;
    if (st == FGPU_PLAN_OK) st = pr.of(*cg, b.contigs.size(), inf.print);
    if (st != FGPU_PLAN_OK) return emit_plan_failed(ctx, "fgpu_stage3_detip", "fgpu_tips_plan", unset, st);
    ctx->s3t_graph.reset();
    if (int rc = pr.emit(ctx, bytes)) return rc;
    ctx->s3t_graph = cg;                         // alive from here on: the next step works on it, fgpu_stage3_graph_take serialises it
    ctx->s3t_serial = ctx->s3b_serial;
    ctx->s3t_dechimered = false;
    if (info) *info = inf;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_dechimera(fgpu_ctx* ctx, uint64_t* bytes, fgpu_chimera_info* info) {
    if (!ctx || !bytes) return FGPU_ERR_ARG;
    *bytes = 0;
    if (info) memset(info, 0, sizeof(*info));
    const std::string who = "fgpu_stage3_dechimera";
    if (!ctx->s3t_graph) { ctx->err = who + ": no fgpu_stage3_detip whose graph has not been taken"; return FGPU_ERR_STATE; }
    if (ctx->s3t_dechimered) { ctx->err = who + ": the step has run on this graph (fgpu_stage3_detip makes a new one)"; return FGPU_ERR_STATE; }
    if (!ctx->s3b_have || ctx->s3t_serial != ctx->s3b_serial) {
        ctx->err = who + ": the build the graph was made of is no longer on the device (taken, or another build was made)";
        return FGPU_ERR_STATE;
    }
    if (ctx->phase != 0) { ctx->err = who + " while a pass is open"; return FGPU_ERR_STATE; }
    const uint64_t n_calls = ctx->s3b_totals[0];
    std::vector<fgpu_cov_summary> cov(n_calls);
    if (int rc = fgpu_stage3_cov_calls(ctx, nullptr, 0, nullptr, 0, cov.data())) return rc;
    fgpu_graph::CleanGraph& cg = *ctx->s3t_graph;
    fgpu_chimera_info inf;
    memset(&inf, 0, sizeof(inf));
    int st = cg.set_cov(cov.data(), n_calls);
    if (st == FGPU_PLAN_OK) {
        ctx->s3t_dechimered = true;
        st = cg.remove_chimeras_and_clean(inf);
    }
    EmitPrint pr;
    if (st == FGPU_PLAN_OK) st = pr.of(cg, n_calls, inf.print);
    if (st != FGPU_PLAN_OK) {
        ctx->s3t_graph.reset();                  // (a step that stopped half-way left a graph that is nobody's)
        return emit_plan_failed(ctx, who, "fgpu_chimera_plan", "ContigGraph::removeChimerasAndClean or printContigs goes through a pointer that was never set or whose target is gone", st);
    }
    if (int rc = pr.emit(ctx, bytes)) return rc;
    if (info) *info = inf;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_graph_take(fgpu_ctx* ctx, fgpu_tips_out* out) {
    if (!ctx || !out) return FGPU_ERR_ARG;
    out->n_nodes = out->n_contigs = out->n_pieces = out->n_print = out->n_print_pieces = 0;
    if (!ctx->s3t_graph) { ctx->err = "fgpu_stage3_graph_take: no fgpu_stage3_detip whose graph has not been taken"; return FGPU_ERR_STATE; }
    fgpu_tips_out need;
    memset(&need, 0, sizeof(need));
    ctx->s3t_graph->graph_records(&need);        // (no room: how large it is)
    const uint64_t nn = need.n_nodes, nc = need.n_contigs, np = need.n_pieces;
    out->n_nodes = nn; out->n_contigs = nc; out->n_pieces = np;
    if (out->nodes_cap < nn || out->contigs_cap < nc || out->pieces_cap < np || (nn && !out->nodes) || !out->list_first || (nc && !out->contigs) || (np && !out->pieces)) {
        ctx->err = "fgpu_stage3_graph_take: an array is smaller than the graph (n_nodes, n_contigs, n_pieces say how large it is)";
        return FGPU_ERR_ARG;
    }
    fgpu_tips_out fill = *out;                   // (exactly the graph's room, so that nothing behind it is written)
    fill.nodes_cap = nn; fill.contigs_cap = nc; fill.pieces_cap = np;
    const int st = ctx->s3t_graph->graph_records(&fill);
    if (st != FGPU_PLAN_OK) { ctx->err = "fgpu_stage3_graph_take: the graph did not fit the room it asked for"; return FGPU_ERR_INTERNAL; }
    ctx->s3t_graph.reset();
    return FGPU_OK;
}

namespace {

// ContigGraph::printGraph of a graph that knows its coverages: the walk (CleanGraph::fastg_records), fgpu_stage3_join of the records' lists over
// the build where it lies, fgpu_stage3_fastg of the joined text where it lies.  The graph is read only.
int emit_fastg(fgpu_ctx* ctx, const std::string& who, const fgpu_graph::CleanGraph& cg, uint64_t* bytes, fgpu_fastg_info* info) {
    fgpu_graph::FastgPlan plan;
    double t0 = fgpu_host_now();
    const int st = cg.fastg_records(plan);
    ctx->s3g_ms[3] = fgpu_host_now() - t0;
    if (st != FGPU_PLAN_OK)
        return emit_plan_failed(ctx, who, "the FASTG walk's", "ContigGraph::printGraph goes through a pointer that was never set or whose target is gone, or asks a contig for an end it does not have", st);
    const uint64_t n = plan.tig.size();
    t0 = fgpu_host_now();
    std::vector<uint64_t> first(n + 1, 0);
    std::vector<fgpu_join_piece> pieces;
    for (uint64_t r = 0; r < n; r++) {
        const auto& list = cg.tigs[plan.tig[r]].list;
        pieces.insert(pieces.end(), list.begin(), list.end());
        first[r + 1] = pieces.size();
    }
    std::vector<fgpu_joined> joined(n);
    uint64_t totals[3];
    if (int rc = fgpu_stage3_join(ctx, first.data(), n, pieces.data(), pieces.size(), nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, joined.data(), totals)) return rc;
    ctx->s3g_ms[4] = fgpu_host_now() - t0;
    t0 = fgpu_host_now();
    std::vector<fgpu_fastg_rec> recs(n);
    for (uint64_t r = 0; r < n; r++) {
        const fgpu_cov_summary& cov = cg.tigs[plan.tig[r]].cov;
        recs[r] = fgpu_fastg_rec{(uint64_t)plan.tig[r], joined[r].text_word, cov.sum, joined[r].len, cov.n};
    }
    if (int rc = fgpu_stage3_fastg(ctx, recs.data(), n, plan.nbr_first.data(), plan.nbr.data(), plan.nbr.size(), nullptr, 0, bytes)) return rc;
    ctx->s3g_ms[5] = fgpu_host_now() - t0;
    if (info) *info = plan.info;
    return FGPU_OK;
}

}  // namespace

extern "C" int fgpu_diag_fastg_times(fgpu_ctx* ctx, double ms[6]) {
    if (!ctx || !ms) return FGPU_ERR_ARG;
    memcpy(ms, ctx->s3g_ms, sizeof(ctx->s3g_ms));
    return FGPU_OK;
}

extern "C" int fgpu_stage3_raw_graph(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_fastg_info* info) {
    if (!ctx || !bytes) return FGPU_ERR_ARG;
    *bytes = 0;
    if (info) memset(info, 0, sizeof(*info));
    const std::string who = "fgpu_stage3_raw_graph";
    EmitBuild b;
    memset(ctx->s3g_ms, 0, sizeof(ctx->s3g_ms));
    double t0 = fgpu_host_now();
    if (int rc = emit_build_records(ctx, who, b)) return rc;
    ctx->s3g_ms[0] = fgpu_host_now() - t0;
    t0 = fgpu_host_now();
    const uint64_t n_calls = b.contigs.size();
    std::vector<fgpu_cov_summary> cov(n_calls + 1);                  // (one more: an empty build's graph still has to know that it was given them)
    if (int rc = fgpu_stage3_cov_calls(ctx, nullptr, 0, nullptr, 0, cov.data())) return rc;
    ctx->s3g_ms[1] = fgpu_host_now() - t0;
    t0 = fgpu_host_now();
    fgpu_graph::CleanGraph cg;                                       // this call's own: a live graph, if there is one, is another object
    const int st = cg.of_build(b.keys.data(), b.recs.data(), b.keys.size(), b.contigs.data(), b.calls.data(), n_calls, cov.data(), ctx->prm.k, read_length);
    ctx->s3g_ms[2] = fgpu_host_now() - t0;
    if (st != FGPU_PLAN_OK) return emit_plan_failed(ctx, who, "the graph's", "JunctionMap::buildContigGraph leaves a pointer unset", st);
    return emit_fastg(ctx, who, cg, bytes, info);
}

extern "C" int fgpu_stage3_graph_fastg(fgpu_ctx* ctx, uint64_t* bytes, fgpu_fastg_info* info) {
    if (!ctx || !bytes) return FGPU_ERR_ARG;
    *bytes = 0;
    if (info) memset(info, 0, sizeof(*info));
    const std::string who = "fgpu_stage3_graph_fastg";
    if (!ctx->s3t_graph) { ctx->err = who + ": no fgpu_stage3_detip whose graph has not been taken"; return FGPU_ERR_STATE; }
    if (!ctx->s3b_have || ctx->s3t_serial != ctx->s3b_serial) {
        ctx->err = who + ": the build the graph was made of is no longer on the device (taken, or another build was made)";
        return FGPU_ERR_STATE;
    }
    if (ctx->phase != 0) { ctx->err = who + " while a pass is open"; return FGPU_ERR_STATE; }
    fgpu_graph::CleanGraph& cg = *ctx->s3t_graph;
    memset(ctx->s3g_ms, 0, sizeof(ctx->s3g_ms));
    if (!cg.have_cov) {                                              // what fgpu_stage3_dechimera would give it, and gives it again
        const double t0 = fgpu_host_now();
        const uint64_t n_calls = ctx->s3b_totals[0];
        std::vector<fgpu_cov_summary> cov(n_calls);
        if (int rc = fgpu_stage3_cov_calls(ctx, nullptr, 0, nullptr, 0, cov.data())) return rc;
        const int st = cg.set_cov(cov.data(), n_calls);
        if (st != FGPU_PLAN_OK) return emit_plan_failed(ctx, who, "the summaries'", "", st);
        ctx->s3g_ms[1] = fgpu_host_now() - t0;
    }
    return emit_fastg(ctx, who, cg, bytes, info);
}
