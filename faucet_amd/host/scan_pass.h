// scan_pass.h — pass 2 on ONE device, for both hosts: the `faucet` command line (faucet_main.cpp) and the patch a maintainer links into the
// reference (integration/faucet_binding.cpp).
//
// ReadScanner::scanReads (src/ReadScanner.cpp:284-359) through the C ABI: the pair consumers are chosen, the batches scanned, both pair filters
// and the pair counts brought back.  scanInputRead's per-read lists feed the pair filters and the pair counts on the device: the short filter's
// adds are order-free (fgpu_scan_short_pairs); the long filter's check-then-insert loop (:317-343) is iterated to the sequential result
// (fgpu_scan_long_pairs), and with --no_cleaning only that loop's two counts are left of it.  Where the device cannot hold the long filter's
// first-set times at 4 bytes per filter bit (--high_cov sizes the filter at E / 2 x 9 bits, src/Faucet.cpp:279-280) the library keeps them per
// batch instead (its sparse state: a note on stderr says so); where not even the filter's BITS fit (FGPU_ERR_NOMEM) the loop runs HERE, over the
// lists the device hands out (pair_loop.h), straight into the caller's bytes -- the reference has no such limit, so neither have the hosts.  Nothing asks the caller to read its input again: a preview of the junction walk that the library cannot
// repair is absorbed inside the library, which scans its own copy of the batches again -- both inputs may be pipes.
// What the hosts do with the junction map afterwards (write_scan_outputs there, gpu_fill_junction_map here) stays with them.
// ShardedRun::scan (shard_host.h) is the same pass over several devices; it has no host loop yet.
// scan_pass_kept is the same pass over the batches pass 1 kept on the device (FGPU_LOAD_KEEP_READS): no scan file is read at all.
// fgpu_diag_long_pairs_state is referred to weakly: a library without it (the tests' CPU stand-in of the ABI) links unchanged and gets no note.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <functional>
#include <vector>

#include "faucet_gpu.h"
#include "pair_loop.h"

#pragma weak fgpu_diag_long_pairs_state
// ... and so are the two entry points of the scan over the batches pass 1 kept (scan_pass_kept): null against a library without them
#pragma weak fgpu_scan_kept_state
#pragma weak fgpu_scan_batch_kept

namespace faucet_host {

// after fgpu_scan_long_pairs has set a filter of `tai` bits up: says on stderr, once per run, when its first-set times are kept per batch
inline void note_long_pairs_state(fgpu_ctx* ctx, uint64_t tai) {
    static std::atomic<bool> said(false);
    uint64_t st[4] = {0, 0, 0, 0};
    if (!fgpu_diag_long_pairs_state || fgpu_diag_long_pairs_state(ctx, st) != FGPU_OK || st[0] != 2) return;
    if (!said.exchange(true))
        fprintf(stderr, "note: the long pair filter (%llu bits) keeps its first-set times per batch (sparse state)\n", (unsigned long long)tai);
}

// a pair filter the scan fills: the caller's tai / 8 bytes (src/Faucet.cpp:266-283).  bits == nullptr: no filter (--no_cleaning, or the
// single-end scan of a caller without one)
struct PairTarget {
    uint8_t* bits;
    uint64_t tai;
    int n_hash;
};

struct ScanPassResult {
    fgpu_scan_stats stats;
    uint64_t empty_count = 0, not_empty_count = 0;     // scanReads' pair counts (paired ends only)
    bool host_loop = false;                            // the paired-end loop ran on the host
    const char* failed = nullptr;                      // the call whose status scan_pass returned (a literal)
    ScanPassResult() { memset(&stats, 0, sizeof(stats)); }
};

typedef std::function<int(const fgpu_reads*)> EachBatch;      // an fgpu status; anything but FGPU_OK ends the feed
// hands the batches of the scan file, in file order, to `each` and returns FGPU_OK or the first status that was not; a feed that fails by
// itself (it cannot split its text, say) names what failed in ScanPassResult::failed
typedef std::function<int(const EachBatch& each)> BatchFeed;

// The same one level up: a batch is something that scans itself (one call of the library, named by `call` when it fails) and says how many
// reads it had -- a batch of text through fgpu_scan_batch, or a batch pass 1 kept through fgpu_scan_batch_kept.
typedef std::function<int(uint64_t* n_reads)> ScanItem;
typedef std::function<int(const ScanItem& item)> EachItem;
typedef std::function<int(const EachItem& each)> ItemFeed;

// FGPU_OK, or the status of the first call that failed (out->failed names it; fgpu_last_error(ctx) has its text).  Once fgpu_scan_begin has
// succeeded the pass is closed with fgpu_scan_end whatever happens in between.
inline int scan_pass_items(fgpu_ctx* ctx, int k, const PairTarget& short_pf, const PairTarget& long_pf, bool paired_ends, const ItemFeed& feed,
                           const char* call, ScanPassResult* out) {
    int rc = FGPU_OK;
#define SCAN_PASS_TRY(call, ...)                                                         \
    do {                                                                                 \
        if ((rc = call(__VA_ARGS__)) != FGPU_OK) { out->failed = #call; return rc; }     \
    } while (0)
    if (short_pf.bits) SCAN_PASS_TRY(fgpu_scan_short_pairs, ctx, short_pf.tai, short_pf.n_hash, 0);
    if (paired_ends) {
        rc = long_pf.bits ? fgpu_scan_long_pairs(ctx, long_pf.tai, long_pf.n_hash, FGPU_LONG_PAIRS_FILTER) : fgpu_scan_long_pairs(ctx, 0, 0, FGPU_LONG_PAIRS_COUNT);
        if (rc == FGPU_ERR_NOMEM && long_pf.bits) {
            fprintf(stderr, "note: the long pair filter (%llu bits) does not fit the device; the paired-end loop runs on the host\n",
                    (unsigned long long)long_pf.tai);
            out->host_loop = true;
            rc = fgpu_scan_long_pairs(ctx, 0, 0, FGPU_LONG_PAIRS_OFF);
            if (rc == FGPU_OK && short_pf.bits) SCAN_PASS_TRY(fgpu_scan_short_pairs, ctx, short_pf.tai, short_pf.n_hash, 1);   // (the lists come to the host)
        }
        if (rc != FGPU_OK) { out->failed = "fgpu_scan_long_pairs"; return rc; }
        if (long_pf.bits && !out->host_loop) note_long_pairs_state(ctx, long_pf.tai);
    }
    HostLongPairs hlp(long_pf.bits, long_pf.tai, long_pf.n_hash, k, true);
    std::vector<fgpu_stop> stops;
    std::vector<uint64_t> batch_reads;          // records per scanned batch: the lists come back by the batch's number
    auto take_lists = [&](bool all) -> int {    // one batch's lists (after a batch call: the batch before it), or all that are left
        for (;;) {
            uint64_t n_stops = 0;
            int64_t seq = -1;
            const int trc = fgpu_scan_take_stops(ctx, stops.data(), stops.size(), &n_stops, &seq);
            if (trc == FGPU_ERR_CAPACITY && seq >= 0) { stops.resize((size_t)(n_stops + n_stops / 4 + 16)); continue; }
            if (trc != FGPU_OK) { out->failed = "fgpu_scan_take_stops"; return trc; }
            if (seq < 0) return FGPU_OK;
            hlp.batch(stops.data(), n_stops, batch_reads[(size_t)seq]);
            if (!all) return FGPU_OK;
        }
    };
    SCAN_PASS_TRY(fgpu_scan_begin, ctx);
    rc = feed([&](const ScanItem& item) -> int {
        uint64_t n_reads = 0;
        const int brc = item(&n_reads);
        if (brc != FGPU_OK) { out->failed = call; return brc; }
        if (!out->host_loop) return FGPU_OK;
        batch_reads.push_back(n_reads);
        return batch_reads.size() > 1 ? take_lists(false) : FGPU_OK;
    });
    const int end_rc = fgpu_scan_end(ctx, &out->stats);
    if (rc != FGPU_OK) { if (!out->failed) out->failed = "the batch feed"; return rc; }
    if (end_rc != FGPU_OK) { out->failed = "fgpu_scan_end"; return end_rc; }
    if (out->host_loop && (rc = take_lists(true)) != FGPU_OK) return rc;
    if (short_pf.bits) SCAN_PASS_TRY(fgpu_scan_short_pairs_download, ctx, short_pf.bits, short_pf.tai / 8);
    if (out->host_loop) {
        out->empty_count = hlp.empty_count;
        out->not_empty_count = hlp.not_empty_count;
    } else if (paired_ends) {
        SCAN_PASS_TRY(fgpu_scan_long_pairs_download, ctx, long_pf.bits, long_pf.bits ? long_pf.tai / 8 : 0, &out->empty_count, &out->not_empty_count);
    }
#undef SCAN_PASS_TRY
    return FGPU_OK;
}

// the batches of the scan file as text: each is scanned by fgpu_scan_batch
inline int scan_pass(fgpu_ctx* ctx, int k, const PairTarget& short_pf, const PairTarget& long_pf, bool paired_ends, const BatchFeed& feed,
                     ScanPassResult* out) {
    return scan_pass_items(ctx, k, short_pf, long_pf, paired_ends, [&](const EachItem& each) -> int {
        return feed([&](const fgpu_reads* r) -> int {
            return each([&](uint64_t* n_reads) -> int {
                *n_reads = r->n_reads;
                return fgpu_scan_batch(ctx, r);
            });
        });
    }, "fgpu_scan_batch", out);
}

// can this library scan the batches pass 1 kept (both entry points are there)?
inline bool scan_kept_linked() { return fgpu_scan_kept_state && fgpu_scan_batch_kept; }

// Pass 2 over the n_batches batches a load pass opened with FGPU_LOAD_KEEP_READS kept (fgpu_scan_kept_state says how many, and that they are
// complete): no input is read.  `progress` (or null) hears the reads scanned so far after every batch.
inline int scan_pass_kept(fgpu_ctx* ctx, int k, const PairTarget& short_pf, const PairTarget& long_pf, bool paired_ends, uint64_t n_batches,
                          const std::function<void(uint64_t reads)>& progress, ScanPassResult* out) {
    if (!scan_kept_linked()) { out->failed = "fgpu_scan_batch_kept (not in this library)"; return FGPU_ERR_STATE; }
    return scan_pass_items(ctx, k, short_pf, long_pf, paired_ends, [&](const EachItem& each) -> int {
        uint64_t reads = 0;
        for (uint64_t i = 0; i < n_batches; i++) {
            uint64_t n = 0;
            const int rc = each([&](uint64_t* n_reads) -> int {
                const int brc = fgpu_scan_batch_kept(ctx, i, &n);
                *n_reads = n;
                return brc;
            });
            if (rc != FGPU_OK) return rc;
            reads += n;
            if (progress) progress(reads);
        }
        return FGPU_OK;
    }, "fgpu_scan_batch_kept", out);
}

}  // namespace faucet_host
