// scan_harvest.hip — scanInputRead's lists (FGPU_FLAG_RECORD_STOPS): the junction visits that the walk (scan_walk.hip) marked in the planes sF / sB
// become the per-read lists of stops, feed the short pair filter on the device, the long pair filter (pairs.hip) and the host queue.
#include "walk_tables.h"

#include <rocprim/rocprim.hpp>

namespace {
__device__ __forceinline__ uint64_t piece_chunk(const unsigned long long* plane, uint64_t p0, uint32_t nwin, uint32_t c) {
    return fd_bits_at((const uint64_t*)plane, p0 + 64ULL * c) & chunk_mask(nwin, c);
}

// elements of the list of every piece: one per junction visit, or the single fake junction (ReadScanner.cpp:195-200)
__global__ void __launch_bounds__(256) k_stop_count(const uint2* __restrict__ pieces, uint64_t n_pieces, const unsigned long long* sF,
                                                    const unsigned long long* sB, uint32_t* __restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pieces) return;
    const uint2 pc = pieces[i];
    uint32_t n = 0;
    for (uint32_t c = 0; c * 64 < pc.y; c++) n += __popcll(piece_chunk(sF, pc.x, pc.y, c)) + __popcll(piece_chunk(sB, pc.x, pc.y, c));
    count[i] = n ? n : 1u;
}

__global__ void __launch_bounds__(256) k_stop_fill(const uint2* __restrict__ pieces, uint64_t n_pieces, const unsigned long long* sF,
                                                   const unsigned long long* sB, const uint32_t* __restrict__ offset,
                                                   const uint32_t* __restrict__ piece_read, const uint64_t* __restrict__ codes, FdParams fp,
                                                   fgpu_stop* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pieces) return;
    const uint2 pc = pieces[i];
    const uint64_t p0 = pc.x;
    const uint32_t nwin = pc.y, rd = piece_read[i];
    fgpu_stop* o = out + offset[i];
    uint32_t n = 0;
    for (uint32_t c = 0; c * 64 < nwin; c++) {
        const uint64_t wF = piece_chunk(sF, p0, nwin, c), wB = piece_chunk(sB, p0, nwin, c);
        uint64_t any = wF | wB;
        while (any) {
            const int b = __builtin_ctzll(any);
            any &= any - 1;
            const uint32_t q = c * 64 + b;
            if ((wB >> b) & 1ULL) {   // half-step 2q: facing BACKWARD, the extension is the reverse complement of the window before
                fgpu_stop e;
                e.ext = fd_revcomp(fd_kmer_at(codes, p0 + q - 1, fp.k), fp.k);
                e.read = rd;
                e.info = q | (n == 0 ? FGPU_STOP_FIRST : 0u);
                o[n++] = e;
            }
            if ((wF >> b) & 1ULL) {   // half-step 2q+1: facing FORWARD, the extension is the next window
                fgpu_stop e;
                e.ext = fd_kmer_at(codes, p0 + q + 1, fp.k);
                e.read = rd;
                e.info = q | FGPU_STOP_FORWARD | (n == 0 ? FGPU_STOP_FIRST : 0u);
                o[n++] = e;
            }
        }
    }
    if (n == 0) {   // add_fake_junction: middle k-mer facing FORWARD (ReadScanner.cpp:92-104)
        const uint32_t m = (nwin + (uint32_t)fp.k - 1) / 2 - (uint32_t)fp.k / 2;
        fgpu_stop e;
        e.ext = fd_kmer_at(codes, p0 + m + 1, fp.k);
        e.read = rd;
        e.info = m | FGPU_STOP_FORWARD | FGPU_STOP_FIRST | FGPU_STOP_FAKE;
        o[0] = e;
    }
}

// Bloom::addPair(JuncPair) (utils/Bloom.cpp:127-139): the two canonical k-mers, the smaller under seed 0 and the larger under seed 1
struct PairFilterDev {
    uint32_t* bits;
    uint64_t mask;
    int n_hash;
};
__device__ __forceinline__ void pf_add_pair(const PairFilterDev& pf, uint64_t k1, uint64_t k2, int k) {
    const uint64_t e1 = fd_canon(k1, k), e2 = fd_canon(k2, k);
    uint64_t h0 = fd_old_hash(e1 < e2 ? e1 : e2, FD_SEED0) & pf.mask;
    const uint64_t h1 = fd_old_hash(e1 < e2 ? e2 : e1, FD_SEED1) & pf.mask;
    for (int i = 0; i < pf.n_hash; i++) {
        atomicOr(&pf.bits[h0 >> 5], 1u << (h0 & 31));
        h0 = (h0 + h1) & pf.mask;
    }
}

// What scan_forward does with its result list when cleaning is on (src/ReadScanner.cpp:208-225), one thread per valid piece: a list of two
// is paired by facing (an outward-facing pair by first backward / last forward junction, two junctions facing the same way as they stand),
// a longer list pairs every element with the next but one.  Adding is order-free, so the device's order is as good as the file's.
__global__ void __launch_bounds__(256) k_short_pairs(const fgpu_stop* __restrict__ stops, const uint32_t* __restrict__ count,
                                                     const uint32_t* __restrict__ offset, uint64_t n_pieces, PairFilterDev pf, int k) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pieces) return;
    const uint32_t n = count[i];
    const fgpu_stop* s = stops + offset[i];
    if (n == 2) {
        bool have_first_back = false, have_last_fwd = false;
        uint32_t rev_pos = 0, for_pos = 0;
        uint64_t first_back = 0, last_fwd = 0;
        for (int t = 0; t < 2; t++) {
            const uint32_t info = s[t].info, pos = info & FGPU_STOP_POS_MASK;
            if (info & FGPU_STOP_FAKE) continue;
            if (!(info & FGPU_STOP_FORWARD)) {
                if (!have_first_back) { have_first_back = true; first_back = s[t].ext; rev_pos = pos; }
            } else {
                if (!have_last_fwd) { have_last_fwd = true; for_pos = pos; }
                last_fwd = s[t].ext;
            }
        }
        if (have_first_back && have_last_fwd && !(rev_pos > for_pos)) pf_add_pair(pf, first_back, last_fwd, k);
        if (have_first_back != have_last_fwd) pf_add_pair(pf, s[0].ext, s[1].ext, k);
    } else if (n > 2) {
        for (uint32_t t = 0; t + 2 < n; t++) pf_add_pair(pf, s[t].ext, s[t + 2].ext, k);
    }
}
}  // namespace

// (see fgpu_touch_scan_walk)
void fgpu_touch_scan_harvest() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)k_stop_count);
}

// Bring the stops of a walked batch to the host queue (waits for that batch's walk only).
int fgpu_scan_harvest(fgpu_ctx* ctx, BatchBufs* b) {
    for (size_t i = 0; i < ctx->to_harvest.size(); i++)
        if (ctx->to_harvest[i] == b) { ctx->to_harvest.erase(ctx->to_harvest.begin() + i); break; }
    if (!b->stops_pending) return FGPU_OK;
    // ONE wait of the host per harvested batch (round 5; there were three: for the walk's event, for the error flags, for the lists' total):
    // the main stream waits for the walk by itself, and what the host has to see -- the flags of the walk (a walk that went wrong must not hand
    // out lists), how many elements the lists hold -- comes back with one synchronisation.
    if (b->walk_pending) {
        FGPU_HIP(hipStreamWaitEvent(ctx->stream, b->walk_done, 0));
        b->walk_pending = false;
    }
    const bool check = ctx->journal_on && !ctx->in_replay;
    const uint64_t np_count = b->n_pieces;
    uint32_t* count_c = nullptr;
    uint32_t* offset_c = nullptr;
    if (np_count) {
        if (int rc0 = fgpu_ensure_b(ctx, &b->stop_off, (2 * np_count + 2) * 4)) return rc0;
        count_c = (uint32_t*)b->stop_off.p;
        offset_c = count_c + np_count + 1;
        hipLaunchKernelGGL(k_stop_count, dim3(fgpu_blocks(np_count, 256)), dim3(256), 0, ctx->stream, (const uint2*)b->pieces.p, np_count,
                           (const unsigned long long*)b->sF.p, (const unsigned long long*)b->sB.p, count_c);
        size_t tmp_bytes = 0;
        FGPU_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, count_c, offset_c, 0u, np_count, rocprim::plus<uint32_t>(), ctx->stream));
        DevBuf& tmp = ctx->probe_buf;
        if (int rc0 = fgpu_ensure_b(ctx, &tmp, tmp_bytes + 16)) return rc0;
        FGPU_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, count_c, offset_c, 0u, np_count, rocprim::plus<uint32_t>(), ctx->stream));
        FGPU_HIP(hipMemcpyAsync(&ctx->fb_host[4], count_c + np_count - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        FGPU_HIP(hipMemcpyAsync(&ctx->fb_host[5], offset_c + np_count - 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    // (the flags always: the one synchronisation is there anyway whenever the batch has pieces)
    FGPU_HIP(hipMemcpyAsync(&ctx->counters_host->error_flags, &ctx->counters->error_flags, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    if (ctx->counters_host->error_flags & 1ULL) {
        // A walk up to this one outgrew the junction table and dropped records: these lists are wrong, and nothing of them may reach the
        // caller or a pair filter.  The flag is cumulative, so a clean one here means every walk up to this batch was good.
        // Absorbable: replayed on a larger table first (as check_errors decides); inside a replay: scan_replay grows the table and goes again.
        ctx->to_harvest.insert(ctx->to_harvest.begin(), b);
        if (fgpu_overflow_absorbable(ctx)) { ctx->lazy_failed = ctx->capacity_failed = true; return FGPU_INTERNAL_REPLAY; }
        ctx->err = FGPU_TABLE_FULL_MSG;
        return FGPU_ERR_CAPACITY;
    }
    if (check && (ctx->counters_host->error_flags & 4ULL)) { ctx->lazy_failed = true; ctx->to_harvest.insert(ctx->to_harvest.begin(), b); return FGPU_INTERNAL_REPLAY; }
    b->stops_pending = false;
    if (b->seq < ctx->stops_delivered) return FGPU_OK;   // scanned again by a replay: the caller has this batch's lists already
    // the lists come to the host unless their consumers on the device said otherwise (fgpu_scan_short_pairs' lists_to_host; a scan that only
    // feeds the long pair filter on the device, fgpu_scan_long_pairs, hands none out)
    const bool to_host = ctx->short_pf ? ctx->short_pf_lists_to_host : !ctx->lp.mode;
    if (to_host) {
        ctx->stop_queue.emplace_back();
        ctx->stop_queue.back().seq = b->seq;
    } else {
        ctx->stops_delivered = b->seq + 1;                // nobody takes them: the lists end in the device's pair filter
    }
    const uint64_t np = b->n_pieces;
    // the long pair filter takes every batch exactly once, whoever else reads the lists: with lists_to_host a replay harvests the batches the
    // caller has not taken yet again, and a second pass of the check-then-insert loop over them would count and insert twice
    const bool lp_due = b->seq >= ctx->lp_applied_seq;
    if (!np) {
        if (!lp_due) return FGPU_OK;
        const int rc0 = fgpu_long_pairs_batch(ctx, nullptr, 0, b->n_reads);   // (its reads still count as ends of pairs)
        if (!rc0) ctx->lp_applied_seq = b->seq + 1;
        return rc0;
    }
    int rc;
    uint32_t* count = count_c;
    uint32_t* offset = offset_c;
    const uint64_t total = (uint64_t)(uint32_t)ctx->fb_host[4] + (uint64_t)(uint32_t)ctx->fb_host[5];
    if ((rc = fgpu_ensure_b(ctx, &b->stop_out, total * sizeof(fgpu_stop)))) return rc;
    hipLaunchKernelGGL(k_stop_fill, dim3(fgpu_blocks(np, 256)), dim3(256), 0, ctx->stream, (const uint2*)b->pieces.p, np,
                       (const unsigned long long*)b->sF.p, (const unsigned long long*)b->sB.p, (const uint32_t*)offset,
                       (const uint32_t*)b->piece_read.p, (const uint64_t*)b->codes.p, ctx->fd, (fgpu_stop*)b->stop_out.p);
    if (ctx->short_pf)
        hipLaunchKernelGGL(k_short_pairs, dim3(fgpu_blocks(np, 256)), dim3(256), 0, ctx->stream, (const fgpu_stop*)b->stop_out.p, (const uint32_t*)count,
                           (const uint32_t*)offset, np, PairFilterDev{ctx->short_pf, ctx->short_pf_tai - 1, ctx->short_pf_hashes}, ctx->fd.k);
    // scanReads' paired-end loop over the same lists (pairs.hip): check-then-insert in file order, exact, on the device
    if (lp_due) {
        if ((rc = fgpu_long_pairs_batch(ctx, (const fgpu_stop*)b->stop_out.p, total, b->n_reads))) return rc;
        ctx->lp_applied_seq = b->seq + 1;
    }
    if (to_host) {
        StopBatch& sb = ctx->stop_queue.back();
        if (total) {
            size_t best = ctx->stop_pool.size();                       // the smallest free buffer that is large enough
            for (size_t i = 0; i < ctx->stop_pool.size(); i++)
                if (ctx->stop_pool[i].cap >= total && (best == ctx->stop_pool.size() || ctx->stop_pool[i].cap < ctx->stop_pool[best].cap)) best = i;
            if (best < ctx->stop_pool.size()) {
                sb.data = ctx->stop_pool[best].data;
                sb.cap = ctx->stop_pool[best].cap;
                ctx->stop_pool.erase(ctx->stop_pool.begin() + (ptrdiff_t)best);
            } else {
                const size_t cap = (size_t)(total + total / 4);
                FGPU_HIP(hipHostMalloc((void**)&sb.data, cap * sizeof(fgpu_stop)));
                sb.cap = cap;
            }
            FGPU_HIP(hipMemcpyAsync(sb.data, b->stop_out.p, total * sizeof(fgpu_stop), hipMemcpyDeviceToHost, ctx->stream));
            FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        }
        sb.n = total;
    }
    return FGPU_OK;
}
