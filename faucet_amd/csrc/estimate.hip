// estimate.hip — pass 0: a sketch of the read set that gives -estimated_kmers (F0, distinct canonical k-mers) and -singletons (f1, those
// seen exactly once), the two numbers every run sizes its filters from (src/Faucet.cpp:197-219) and the reference asks a separate tool for.
//
// A valid window (the occurrences of the loop at utils/Bloom.cpp:289: fd_window_ok on the packed stream) is hashed once, h = fd_mix(canon) --
// a bijection, so no two k-mers share an h -- and lands in level min(clz64(h) / 4, 3), cell h & (m - 1), m = 2^r_bits cells per level:
// levels >= l together hold the k-mers whose h has at least 4 l leading zeros, a 16^-l sample of the k-mer space.  A cell has two bits,
// `seen` (hit at least once) and `twice` (hit at least twice, by the same or by different k-mers), both in one 32-bit word as the {bloo1,
// bloo2} pair of load.hip keeps its two filters: 16 cells per word, `seen` in the low half, `twice` in the high half at the same place.
// The planes a pass ends with are a function of the multiset of occurrences alone -- not of order, grid, batching or races -- so the counts
// (cells without `seen`, cells with `seen` and not `twice`, per level) can be checked on the CPU to the last counter.  The arithmetic that
// turns the counts into F0 and f1 is host code: fgpu_estimate_solve, sizing.cpp.  For the same reason the sketches of the shards of a read set merge
// into the sketch of the whole (k_est_merge), which is how pass 0 runs over several GPUs: fgpu_group_estimate_end, group.hip.
#include <string>

#include "fgpu_ctx.h"

namespace {

constexpr int EST_LEVELS = FGPU_EST_LEVELS, EST_SHIFT = FGPU_EST_SHIFT;

// One occurrence per stream position, on the striding grid of the other per-position kernels.  An occurrence ORs `seen`; if the word it gets
// back had `seen` already it was not the first and ORs `twice`.  The plain test in front spares the atomics of settled cells: a stale 0 only
// costs a redundant atomic, a 1 is never stale because bits are never cleared (fd_bloom_set).  Whoever sees `seen` set -- by the load or by
// the atomic's answer -- is not the cell's first occurrence, and exactly one atomic per hit cell is answered without `seen`: `twice` ends up
// set iff the cell was hit at least twice.
__global__ void __launch_bounds__(256) k_est_sketch(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T, uint64_t n_words,
                                                    int k, uint32_t* planes, int r_bits, unsigned long long* kmers) {
    unsigned long long n_ok = 0;
    const uint64_t total = n_words * 64, cell_mask = (1ULL << r_bits) - 1;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        if (!(p < T && fd_window_ok(bad, p, k))) continue;
        n_ok++;
        const uint64_t h = fd_mix(fd_canon(fd_kmer_at(codes, p, k), k));
        const int lz = h ? __clzll((long long)h) : 64;
        const uint64_t level = (uint64_t)min(lz / EST_SHIFT, EST_LEVELS - 1);
        const uint64_t cell = h & cell_mask;
        uint32_t* word = planes + ((level << (r_bits - 4)) + (cell >> 4));
        const uint32_t seen = 1u << (cell & 15), twice = seen << 16;
        uint32_t w = *word;
        if (w & twice) continue;
        if (!(w & seen)) {
            w = atomicOr(word, seen);
            if (!(w & seen)) continue;      // the cell's first occurrence
        }
        if (!(w & twice)) atomicOr(word, twice);
    }
    block_add(kmers, n_ok);
}

// empty[l] = cells of level l without `seen`, once[l] = cells with `seen` and not `twice`, over the 16-byte granules [g0, g1) of the planes
// (a granule is 64 cells of one level: level = granule >> (r_bits - 6), so a range may begin and end inside a level and cross several): the
// planes streamed one granule per lane and step, level by level; out = {empty[4], once[4]}.  Counts add over disjoint ranges: the whole
// range gives a sketch's counts, a rank's slice of a merged sketch its share of them (fgpu_group_estimate_end).
__global__ void __launch_bounds__(256) k_est_count(const uint4* __restrict__ planes, int r_bits, uint64_t g0, uint64_t g1, unsigned long long* out) {
    const uint64_t per_level = 1ULL << (r_bits - 6), stride = (uint64_t)gridDim.x * blockDim.x;
    for (int l = 0; l < EST_LEVELS; l++) {
        const uint64_t lo = max(g0, (uint64_t)l * per_level), hi = min(g1, (uint64_t)(l + 1) * per_level);
        if (lo >= hi) continue;           // (uniform over the grid: no level's block_add is entered by a part of a block)
        unsigned long long n_empty = 0, n_once = 0;
        for (uint64_t i = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += stride) {
            const uint4 v = planes[i];
            n_empty += 64 - (__popc(v.x & 0xFFFFu) + __popc(v.y & 0xFFFFu) + __popc(v.z & 0xFFFFu) + __popc(v.w & 0xFFFFu));
            n_once += __popc(v.x & ~(v.x >> 16) & 0xFFFFu) + __popc(v.y & ~(v.y >> 16) & 0xFFFFu) + __popc(v.z & ~(v.z >> 16) & 0xFFFFu) +
                      __popc(v.w & ~(v.w >> 16) & 0xFFFFu);
        }
        block_add(&out[l], n_empty);
        block_add(&out[EST_LEVELS + l], n_once);
    }
}

// A cell is a counter that saturates at 2 (`seen` alone: 1, `seen` and `twice`: 2 or more), and two sketches of the same r_bits merge by
// saturating addition cell by cell: `seen` and `twice` are ORed, and a cell both sides have seen has been hit twice.  Associative and
// commutative, so any order of merging the sketches of the shards of a read set gives the planes one sketch of all reads ends with.
__device__ __forceinline__ uint32_t est_merge_word(uint32_t a, uint32_t b) { return a | b | ((a & b & 0xFFFFu) << 16); }

// own[i] = merge(own[i], peer[i]) over n granules, one uint4 (64 cells) per lane and step.  Plain loads and stores: the stream orders the
// kernel behind the copy that brought the peer's words and behind the sketch kernels of this context, and nobody else writes this range.
__global__ void __launch_bounds__(256) k_est_merge(uint4* __restrict__ own, const uint4* __restrict__ peer, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 a = own[i], b = peer[i];
        own[i] = make_uint4(est_merge_word(a.x, b.x), est_merge_word(a.y, b.y), est_merge_word(a.z, b.z), est_merge_word(a.w, b.w));
    }
}

}  // namespace

// (see fgpu_touch_load)
void fgpu_touch_estimate() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)k_est_sketch);
}

static_assert(EST_LEVELS == 4 && EST_SHIFT == 4, "fgpu_estimate holds four levels of a 16^-l sample each");

// ---- what fgpu_estimate_end shares with the collective end of the pass (fgpu_group_estimate_end, group.hip)
// the counts of granules [g0, g1) of the open pass' planes and the pass' k-mers into h (host: empty[4], once[4], kmers), behind everything
// the pass has queued; returns once the device has finished it all
int fgpu_estimate_range_counts(fgpu_ctx* ctx, uint64_t g0, uint64_t g1, uint64_t h[2 * FGPU_EST_LEVELS + 1]) {
    unsigned long long* d = (unsigned long long*)ctx->est_counts.p;
    if (g1 > g0) FGPU_LAUNCH("est_count", k_est_count, fgpu_grid(g1 - g0, 256), 256, (const uint4*)ctx->est_planes, ctx->est_r_bits, g0, g1, d);
    FGPU_HIP(hipMemcpyAsync(h, d, (2 * EST_LEVELS + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    return fgpu_pull_counters(ctx);      // waits for the stream; a batch's total_bases that did not match its offsets
}

// the pass is over, and its planes go back.  `later` (or null): the planes are not freed but handed to the caller, who frees them once
// nothing can be reading them any more (a peer's copy out of them may still run: fgpu_group_estimate_end)
void fgpu_estimate_close(fgpu_ctx* ctx, void** later) {
    if (later) *later = ctx->est_planes;
    else (void)hipFree(ctx->est_planes);
    ctx->est_planes = nullptr;
    ctx->phase = 0;
}

// Every block the pass holds goes back (the sketch kernels that read them may still be queued: the stream is waited for first)
void fgpu_estimate_drop_kept(fgpu_ctx* ctx) {
    if (!ctx->est_kept.empty()) {
        (void)hipSetDevice(ctx->prm.device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (PackedBlock& b : ctx->est_kept) (void)hipFree(b.buf.p);
        ctx->est_kept.clear();
    }
    if (!ctx->est_kept_reads.empty() || !ctx->est_taken_reads.empty()) {      // the offsets kept beside them (fgpu_estimate_keep_reads), taken or not
        (void)hipSetDevice(ctx->prm.device);
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        for (fgpu_kept_reads& r : ctx->est_kept_reads) (void)hipFree(r.offsets_dev);
        for (fgpu_kept_reads& r : ctx->est_taken_reads) (void)hipFree(r.offsets_dev);
        ctx->est_kept_reads.clear();
        ctx->est_taken_reads.clear();
    }
    ctx->est_keep_bytes = 0;
}

// level, f0, f1 from the counts, with the words fgpu_estimate_end leaves in the context for a status that is not FGPU_OK
int fgpu_estimate_finish(fgpu_ctx* ctx, fgpu_estimate* e, const char* who) {
    const int rc = fgpu_estimate_solve(e);
    if (rc == FGPU_ERR_CAPACITY) ctx->err = std::string(who) + ": the sketch is too full even at its thinnest level (fewer than an eighth of its cells empty): raise r_bits";
    else if (rc) ctx->err = std::string(who) + ": counts that no sketch gives (internal error)";
    return rc;
}

extern "C" {

int fgpu_estimate_begin(fgpu_ctx* ctx, int32_t r_bits) {
    if (!ctx) return FGPU_ERR_ARG;
    if (r_bits == 0) r_bits = FGPU_EST_DEFAULT_BITS;
    if (r_bits < FGPU_EST_MIN_BITS || r_bits > FGPU_EST_MAX_BITS) { ctx->err = "estimate_begin: r_bits must be 0 (the default, 30) or in 8..34"; return FGPU_ERR_ARG; }
    if (ctx->phase != 0) { ctx->err = "estimate_begin while another pass is open"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    fgpu_estimate_drop_kept(ctx);        // blocks of an earlier pass that nobody took
    ctx->est_keep_asked = ctx->est_keeping = false;
    ctx->est_keep_reads = false;
    ctx->est_batches = 0;
    // 2 bits x 4 levels x 2^r_bits cells = 2^r_bits bytes, for the duration of the pass
    const uint64_t bytes = 1ULL << r_bits;
    hipError_t e = hipMalloc(&ctx->est_planes, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->est_planes = nullptr;
        ctx->err = std::string("hipMalloc of the estimate planes (") + std::to_string(bytes) + " bytes) failed: " + hipGetErrorString(e) + ": lower r_bits";
        return FGPU_ERR_NOMEM;
    }
    int rc = fgpu_ensure(ctx, &ctx->est_counts, (2 * EST_LEVELS + 1) * 8);
    if (!rc && hipMemsetAsync(ctx->est_planes, 0, bytes, ctx->stream) != hipSuccess) { ctx->err = "estimate_begin: clearing the planes failed"; rc = FGPU_ERR_HIP; }
    if (!rc && hipMemsetAsync(ctx->est_counts.p, 0, (2 * EST_LEVELS + 1) * 8, ctx->stream) != hipSuccess) { ctx->err = "estimate_begin: clearing the counts failed"; rc = FGPU_ERR_HIP; }
    // (the packing kernels report a wrong fgpu_reads.total_bases through the context's error flags: read at the end of the pass)
    if (!rc && hipMemsetAsync(&ctx->counters->error_flags, 0, 8, ctx->stream) != hipSuccess) { ctx->err = "estimate_begin: clearing the error flags failed"; rc = FGPU_ERR_HIP; }
    if (rc) {
        (void)hipFree(ctx->est_planes);
        ctx->est_planes = nullptr;
        return rc;
    }
    ctx->est_r_bits = r_bits;
    ctx->phase = 4;
    return FGPU_OK;
}

int fgpu_estimate_batch(fgpu_ctx* ctx, const fgpu_reads* reads) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_batch outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    int rc = fgpu_check_reads(ctx, reads);
    if (rc) return rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    ctx->est_batches++;
    const uint64_t *codes, *bad;
    uint64_t T, n_words;
    PackedBlock blk;
    if (ctx->est_keeping && reads->n_reads) {
        bool no_memory;
        // fgpu_estimate_keep_reads: the batch's (n_reads + 1) offsets are charged with its block, and kept in an allocation of their own
        const uint64_t ob = ctx->est_keep_reads ? (reads->n_reads + 1) * 8 : 0, left = ctx->est_keep_budget - ctx->est_keep_bytes;
        void* offs = nullptr;
        if (ob && ob <= left && hipMalloc(&offs, ob) != hipSuccess) { (void)hipGetLastError(); offs = nullptr; }
        if ((rc = fgpu_stage_pack_keep(ctx, reads, ob && !offs ? 0 : left - ob, &blk, &no_memory))) { if (offs) (void)hipFree(offs); return rc; }
        if (ob && !offs && !blk.buf.p) no_memory = ob <= left;
        if (offs && blk.buf.p) {
            FGPU_HIP(hipMemcpyAsync(offs, ctx->cur->d_offs, ob, hipMemcpyDeviceToDevice, ctx->stream));
            fgpu_kept_reads kr = {offs, reads->n_reads, 0};
            ctx->est_kept_reads.push_back(kr);
            ctx->est_keep_bytes += ob;
        } else if (offs) {
            (void)hipFree(offs);
        }
        if (!blk.buf.p) {   // the batch is not kept, so nothing is: the pass goes on as one that was never asked to keep
            ctx->est_keep_stop_need = 4 * (blk.n_words + FGPU_PADW) * 8 + ob;
            ctx->est_keep_stop_used = ctx->est_keep_bytes;
            ctx->est_keep_stop_blocks = ctx->est_kept.size();
            ctx->est_keep_stop_nomem = no_memory;
            ctx->est_keeping = false;
            fgpu_estimate_drop_kept(ctx);
        }
    } else if ((rc = fgpu_stage_pack(ctx, reads))) {
        return rc;
    }
    if (blk.buf.p) {
        codes = (const uint64_t*)blk.buf.p;
        bad = codes + 2 * (blk.n_words + FGPU_PADW);
        T = blk.T;
        n_words = blk.n_words;
        ctx->est_kept.push_back(blk);
        ctx->est_keep_bytes += 4 * (blk.n_words + FGPU_PADW) * 8;
    } else {
        const BatchBufs& bb = *ctx->cur;
        codes = (const uint64_t*)bb.codes.p;
        bad = (const uint64_t*)bb.bad.p;
        T = bb.T;
        n_words = bb.n_words;
    }
    if (T)
        FGPU_LAUNCH("est_sketch", k_est_sketch, fgpu_grid(n_words * 64, 256), 256, codes, bad, T, n_words, ctx->fd.k, ctx->est_planes, ctx->est_r_bits,
                    (unsigned long long*)ctx->est_counts.p + 2 * EST_LEVELS);
    return fgpu_host_batch_done(ctx, reads);
}

int fgpu_estimate_keep(fgpu_ctx* ctx, uint64_t budget_bytes) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_keep outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    if (ctx->est_batches) { ctx->err = "estimate_keep after the pass' first batch: a pass keeps all of its batches or none"; return FGPU_ERR_STATE; }
    ctx->est_keep_asked = ctx->est_keeping = true;
    ctx->est_keep_budget = budget_bytes;
    ctx->est_keep_bytes = 0;
    return FGPU_OK;
}

int fgpu_estimate_keep_reads(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 4 || !ctx->est_keep_asked) { ctx->err = "estimate_keep_reads comes after estimate_keep, inside its pass"; return FGPU_ERR_STATE; }
    if (ctx->est_batches) { ctx->err = "estimate_keep_reads after the pass' first batch: a pass keeps all of its batches' reads or none"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    FGPU_HIP(hipMemsetAsync(&ctx->counters->max_read_len, 0, 8, ctx->stream));      // the longest read of THIS pass (k_pack_fix: a running maximum)
    ctx->est_keep_reads = true;
    return FGPU_OK;
}

int fgpu_estimate_take_kept_reads(fgpu_ctx* ctx, fgpu_kept_reads* out, uint64_t cap, uint64_t* n_out) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase == 4 || !ctx->est_kept.empty() || !ctx->est_kept_reads.empty()) {
        ctx->err = "estimate_take_kept_reads comes after estimate_end and estimate_take_kept of the same pass";
        return FGPU_ERR_STATE;
    }
    if (n_out) *n_out = ctx->est_taken_reads.size();
    if (!ctx->est_keep_reads) { ctx->err = "estimate_take_kept_reads: the pass did not keep its reads (fgpu_estimate_keep_reads)"; return FGPU_ERR_STATE; }
    if (ctx->est_taken_reads.size() > cap || (!out && !ctx->est_taken_reads.empty())) {
        ctx->err = "estimate_take_kept_reads: room for " + std::to_string(out ? cap : 0) + " entries, the pass kept " + std::to_string(ctx->est_taken_reads.size());
        return FGPU_ERR_ARG;
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    unsigned long long longest = 0;      // (fgpu_estimate_end has waited for the pass' last kernels)
    FGPU_HIP(hipMemcpyAsync(&longest, &ctx->counters->max_read_len, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    for (size_t i = 0; i < ctx->est_taken_reads.size(); i++) {
        out[i] = ctx->est_taken_reads[i];
        out[i].max_read_len = longest;
    }
    ctx->est_taken_reads.clear();
    ctx->est_keep_reads = false;
    return FGPU_OK;
}

int fgpu_estimate_keep_state(fgpu_ctx* ctx, int* keeping, uint64_t* n_blocks, uint64_t* bytes) {
    if (!ctx) return FGPU_ERR_ARG;
    if (keeping) *keeping = ctx->est_keeping ? 1 : 0;
    if (n_blocks) *n_blocks = ctx->est_kept.size();
    if (bytes) *bytes = ctx->est_keep_bytes;
    return FGPU_OK;
}

int fgpu_estimate_take_kept(fgpu_ctx* ctx, fgpu_packed* out, uint64_t cap, uint64_t* n_out) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase == 4) { ctx->err = "estimate_take_kept inside the pass: its blocks are handed out after estimate_end"; return FGPU_ERR_STATE; }
    if (n_out) *n_out = ctx->est_kept.size();
    if (ctx->est_keep_asked && !ctx->est_keeping) {
        ctx->err = "estimate_take_kept: the pass stopped keeping at a batch that needed " + std::to_string(ctx->est_keep_stop_need) + " bytes with " +
                   std::to_string(ctx->est_keep_stop_used) + " bytes held in " + std::to_string(ctx->est_keep_stop_blocks) + " blocks" +
                   (ctx->est_keep_stop_nomem ? ": the device had no memory for its block (budget " : ": beyond the budget of ") +
                   std::to_string(ctx->est_keep_budget) + (ctx->est_keep_stop_nomem ? " bytes)" : " bytes");
        return FGPU_ERR_NOMEM;
    }
    if (ctx->est_kept.size() > cap || (!out && !ctx->est_kept.empty())) {
        ctx->err = "estimate_take_kept: room for " + std::to_string(out ? cap : 0) + " blocks, the pass kept " + std::to_string(ctx->est_kept.size());
        return FGPU_ERR_ARG;
    }
    for (size_t i = 0; i < ctx->est_kept.size(); i++) {
        const PackedBlock& b = ctx->est_kept[i];
        out[i].block_dev = b.buf.p;
        out[i].nbytes = fgpu_packed_bytes(b.n_words);
        out[i].T = b.T;
        out[i].n_reads = b.n_reads;
    }
    ctx->est_kept.clear();
    ctx->est_taken_reads.swap(ctx->est_kept_reads);      // (the blocks are the caller's: their offsets wait for fgpu_estimate_take_kept_reads)
    ctx->est_keep_bytes = 0;
    ctx->est_keep_asked = ctx->est_keeping = false;
    return FGPU_OK;
}

int fgpu_estimate_end(fgpu_ctx* ctx, fgpu_estimate* out) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_end without estimate_begin"; return FGPU_ERR_STATE; }
    (void)hipSetDevice(ctx->prm.device);
    fgpu_estimate e;
    memset(&e, 0, sizeof(e));
    e.r_bits = ctx->est_r_bits;
    e.level = -1;
    uint64_t h[2 * EST_LEVELS + 1];
    int rc = fgpu_estimate_range_counts(ctx, 0, 4ULL << (ctx->est_r_bits - 6), h);
    // the pass is over either way, and its planes go back
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    fgpu_estimate_close(ctx, nullptr);
    if (rc) return rc;
    for (int l = 0; l < EST_LEVELS; l++) {
        e.empty[l] = h[l];
        e.once[l] = h[EST_LEVELS + l];
    }
    e.kmers = h[2 * EST_LEVELS];
    rc = fgpu_estimate_finish(ctx, &e, "estimate_end");
    if (out) *out = e;
    return rc;
}

int fgpu_estimate_planes(fgpu_ctx* ctx, void** dev, uint64_t* nbytes) {
    if (!ctx || !dev) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_planes outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    *dev = ctx->est_planes;
    if (nbytes) *nbytes = 1ULL << ctx->est_r_bits;
    return FGPU_OK;
}

int fgpu_estimate_merge(fgpu_ctx* ctx, const void* peer_dev, uint64_t first_byte, uint64_t nbytes) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_merge outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    const uint64_t bytes = 1ULL << ctx->est_r_bits;
    if (!peer_dev || ((uintptr_t)peer_dev & 15) || (first_byte & 15) || (nbytes & 15) || first_byte > bytes || nbytes > bytes - first_byte) {
        ctx->err = "estimate_merge: a device pointer and a range of whole 16-byte granules inside the planes";
        return FGPU_ERR_ARG;
    }
    if (!nbytes) return FGPU_OK;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    FGPU_LAUNCH("est_merge", k_est_merge, fgpu_grid(nbytes / 16, 256), 256, (uint4*)((char*)ctx->est_planes + first_byte), (const uint4*)peer_dev, nbytes / 16);
    return FGPU_OK;
}

int fgpu_estimate_kmers(fgpu_ctx* ctx, uint64_t* kmers) {
    if (!ctx || !kmers) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_kmers outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    FGPU_HIP(hipMemcpyAsync(kmers, (const unsigned long long*)ctx->est_counts.p + 2 * EST_LEVELS, 8, hipMemcpyDeviceToHost, ctx->stream));
    return fgpu_pull_counters(ctx);      // waits for the stream
}

int fgpu_estimate_download(fgpu_ctx* ctx, void* host, uint64_t nbytes) {
    if (!ctx || !host) return FGPU_ERR_ARG;
    if (ctx->phase != 4) { ctx->err = "estimate_download outside estimate_begin/estimate_end"; return FGPU_ERR_STATE; }
    if (nbytes != 1ULL << ctx->est_r_bits) { ctx->err = "estimate_download: the planes are 2^r_bits bytes"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    FGPU_HIP(hipMemcpyAsync(host, ctx->est_planes, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}

}  // extern "C"
