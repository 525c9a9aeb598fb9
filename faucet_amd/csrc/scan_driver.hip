// scan_driver.hip — the host side of pass 2: the extern "C" entry points from fgpu_scan_resident_base to fgpu_scan_import_hint.
//
// No kernel lives here.  The unit holds the order in which the stages of scan_pure.hip / scan_walk.hip / scan_harvest.hip / scan_table.hip are put
// on the streams for one batch, and everything a scan keeps on the host between batches: the batch buffers, the journal and its replay, the
// batches the load pass kept and the batches prepared ahead of their turn, the stop lists, the table hand-over between read shards.  The
// window-span controller it feeds is walk_span.h.  (The context's life cycle, the load pass and the helpers both units need: api.hip.)
#include <cstdio>
#include <algorithm>
#include <string>

#include "fgpu_ctx.h"

// ---- the state checks the entry points share (callers and tests match on the texts) ----------------------------------------------------------
static int need_scan(fgpu_ctx* ctx, const char* who) {
    if (ctx->phase == 2) return FGPU_OK;
    ctx->err = std::string(who) + " outside scan_begin/scan_end";
    return FGPU_ERR_STATE;
}
static int need_none_prepared(fgpu_ctx* ctx, const char* who) {
    if (ctx->prepared.empty()) return FGPU_OK;
    ctx->err = std::string(who) + " while prepared batches are waiting: call fgpu_scan_walk_prepared first";
    return FGPU_ERR_STATE;
}
static int need_real_table(fgpu_ctx* ctx) {
    if (!ctx->hint_in_table) return FGPU_OK;
    ctx->err = "the junction table holds a preview (fgpu_scan_import_hint): import the real table before walking";
    return FGPU_ERR_STATE;
}

// ---- batch buffers ---------------------------------------------------------------------------------------------------------------------------
// a batch's buffers (empty) with its events, made once
static BatchBufs* new_batch(fgpu_ctx* ctx) {
    BatchBufs* b = new BatchBufs();
    ctx->all_batches.push_back(b);
    hipEventCreateWithFlags(&b->pure_done, hipEventDisableTiming);
    hipEventCreateWithFlags(&b->walk_done, hipEventDisableTiming);
    bool all = true;
    for (hipEvent_t& e : b->range_ev) all = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess && all;
    if (!all) {      // without every range event the batch's back half stays one range (scan_range_plan looks at slot 0)
        for (hipEvent_t& e : b->range_ev) { if (e) hipEventDestroy(e); e = nullptr; }
        (void)hipGetLastError();
    }
    return b;
}

static BatchBufs* acquire_batch(fgpu_ctx* ctx) {
    // FIFO over (at least) two BatchBufs, so that the one handed out was last walked two batches ago
    BatchBufs* b;
    // (at most FGPU_DELTA_RING: a batch registers the created-key lists of the FGPU_DELTA_RING - 1 batches before it)
    static const size_t depth = getenv("FGPU_SCAN_BUFFERS") ? (size_t)std::min(FGPU_DELTA_RING, std::max(2, atoi(getenv("FGPU_SCAN_BUFFERS")))) : 2;
    // The buffers handed out are the ones used `depth` batches ago -- NOT the oldest of the pool: a context that has walked a prepared shard
    // keeps dozens of buffers, and a streaming scan that took them first in, first out let its pure stage run as far ahead of the walk as the
    // pool is deep (nothing left to wait for), beyond what the created-key lists cover: keys missing from the snapshot planes, a wrong map
    // (seen at config 4's size, 50 M reads streamed after a 60 M-read prepared shard: 9 887 records too many).  The streaming scan pushes every
    // batch's buffers back at the end of the pool, so the one used `depth` batches ago sits `depth` from the end.
    if (ctx->pool.size() >= depth) {
        const size_t at = ctx->pool.size() - depth;
        b = ctx->pool[at];
        ctx->pool.erase(ctx->pool.begin() + at);
    } else {
        b = new_batch(ctx);
    }
    return b;
}

// after the walk of batch b has been issued: its lists become available (FGPU_FLAG_RECORD_STOPS)
static void note_walked(fgpu_ctx* ctx, BatchBufs* b) {
    if (!ctx->record_stops) return;
    b->stops_pending = true;
    ctx->to_harvest.push_back(b);
}

// The planes of a packed batch, whoever holds them (BatchBufs, JournalBatch, ResidentBatch): their sizes in bytes ...
struct PlaneBytes {
    uint64_t codes, bad, offs;      // offs: 0 where the holder does not keep the read offsets
    uint64_t all() const { return codes + bad + offs; }
};
static PlaneBytes plane_bytes(uint64_t n_words, uint64_t n_reads, bool with_offs) {
    const uint64_t plane = (n_words + FGPU_PADW) * 8;
    return PlaneBytes{2 * plane, plane, with_offs ? (n_reads + 1) * 8 : 0};
}
// ... and the way from one holder to another: room for all of them first, then (copy) codes, bad and, where kept, offsets on the main stream
static int planes_bring(fgpu_ctx* ctx, const PlaneBytes& n, DevBuf* codes, DevBuf* bad, DevBuf* offs, const void* from_codes, const void* from_bad,
                        const void* from_offs, bool copy) {
    int rc;
    if ((rc = fgpu_ensure_b(ctx, codes, n.codes)) || (rc = fgpu_ensure_b(ctx, bad, n.bad)) || (n.offs && (rc = fgpu_ensure_b(ctx, offs, n.offs)))) return rc;
    if (!copy) return FGPU_OK;
    FGPU_HIP(hipMemcpyAsync(codes->p, from_codes, n.codes, hipMemcpyDeviceToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(bad->p, from_bad, n.bad, hipMemcpyDeviceToDevice, ctx->stream));
    if (n.offs) FGPU_HIP(hipMemcpyAsync(offs->p, from_offs, n.offs, hipMemcpyDeviceToDevice, ctx->stream));
    return FGPU_OK;
}

// The batch's stream comes into `b` from the text (reads: packed) or from a batch the load pass kept (kept: its planes copied, nothing packed
// or compared -- fgpu_scan_batch_kept); everything behind that is common.
static int scan_take_kept(fgpu_ctx* ctx, BatchBufs* b, const ResidentBatch* kept) {
    b->T = kept->T; b->n_words = kept->n_words; b->n_reads = kept->n_reads;
    b->d_offs = (const uint64_t*)kept->offs_p();
    if (int rc = planes_bring(ctx, plane_bytes(b->n_words, 0, false), &b->codes, &b->bad, nullptr, kept->codes_p(), kept->bad_p(), nullptr, true)) return rc;
    // the longest read bounds how far a piece reaches (max_piece_span): the text path's packing refills the counter, here the load pass' value
    // seeds it, host copy and device copy (as the replay does from journal_max_read_len), before the first pure stage that needs it
    if (ctx->counters_host->max_read_len < ctx->kept_max_read_len) {
        ctx->kept_seed = ctx->kept_max_read_len;
        ctx->counters_host->max_read_len = ctx->kept_seed;
        FGPU_HIP(hipMemcpyAsync(&ctx->counters->max_read_len, &ctx->kept_seed, 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return FGPU_OK;
}

// ---- what a fresh scan and a replay both start from --------------------------------------------------------------------------------------------
// Host state only (the device's side: fgpu_scan_reset and the counters, at both callers).  A field the scan gains belongs here unless it has to
// survive a replay -- then it is reset in fgpu_scan_begin's own block, which says why.
static void scan_rewind(fgpu_ctx* ctx) {
    memset(&ctx->scan_stats, 0, sizeof(ctx->scan_stats));      // (the replay puts reads_processed back)
    memset(ctx->counters_host, 0, sizeof(DevCounters));
    ctx->scan_windows = 0;
    ctx->scan_pieces_seen = 0;
    ctx->scan_piece_base = 0;
    ctx->scan_imported = 0;
    ctx->delta_next = 0;
    ctx->hint_in_table = false;
    ctx->delta_ready = false;            // (the replay makes every batch's planes from scratch against the table as it stands)
    ctx->span.begin_scan(ctx->prm.walk_window_span);
    ctx->walked_pieces = 0;
    ctx->scan_batch_index = 0;
    for (BatchBufs* b : ctx->to_harvest) b->stops_pending = false;   // lists nobody asked for: an earlier scan's, or a voided walk's
    ctx->to_harvest.clear();
    fgpu_stop_queue_recycle(ctx);
    for (BatchBufs* b : ctx->prepared) ctx->pool.push_back(b);
    ctx->prepared.clear();
}

// ---- one batch's turn in the ordered walk -------------------------------------------------------------------------------------------------------
// Room in the junction table for what the batch may add, the controller's look at the counters, the walk of ctx->cur (= b) issued, its pieces
// counted, its lists queued for the harvest.  counters_host must be fresh with respect to the walks issued so far (the caller's synchronisation:
// the pure stage's piece count, or fgpu_pull_counters between prepared batches).  What the three callers do differently:
enum {
    WALK_TIMED = 1,          // the streaming scan: the walk's issue counts as host_ms[5] (FGPU_DEBUG_HOST)
    WALK_REFRESH = 2,        // a prepared batch: its snapshot planes are made again by the walk stream first (refresh_snapshot)
    WALK_NO_FEEDBACK = 4     // the first prepared batch of a call: no synchronisation precedes it, so neither the table nor the span is looked at (kept as found)
};
static int scan_walk_step(fgpu_ctx* ctx, BatchBufs* b, int how) {
    static const bool dbg_span = getenv("FGPU_DEBUG_SPAN") != nullptr;
    if (!(how & WALK_NO_FEEDBACK)) {
        // records as of the last synchronisation (the previous walk may still be adding some): room for this batch's
        if (int rc = fgpu_scan_reserve(ctx, ctx->counters_host->n_junctions + ctx->scan_imported)) return rc;
        const DevCounters& c = *ctx->counters_host;      // (the walk may lag one batch behind them)
        ctx->span.after_batch(c.followers_seen, c.walked_pieces, c.ko_overflows, ctx->prm.walk_window_span, dbg_span);
    }
    ctx->refresh_snapshot = (how & WALK_REFRESH) != 0;
    const double t_w = fgpu_host_now();
    const int rc = fgpu_stage_scan_walk(ctx, b->n_pieces);
    if (how & WALK_TIMED) ctx->host_ms[5] += fgpu_host_now() - t_w;
    ctx->refresh_snapshot = false;
    ctx->walked_pieces += b->n_pieces;
    if (!rc) note_walked(ctx, b);
    return rc;
}

// ---- the scan's journal: lazy junction tests without a caller-visible fall-back ---------------------------------------------------------
// While a scan evaluates its junction tests lazily the packed form of every batch (codes + bad plane, 3 bits per base; the read offsets when
// scanInputRead's lists are recorded) stays in HBM, up to an eighth of the device memory.  If the walk meets a preview it cannot repair
// (never seen on real input, forced by FGPU_DEBUG_LAZY_FAIL=1) the library itself resets the junction map and scans the
// journal again with every test evaluated: same results, nothing for the caller to do -- ReadScanner::scanReads has no such contract
// either (src/ReadScanner.cpp:284-359).  A scan that outgrows the journal is first brought to a point where everything walked so far is
// known to be good, then goes on with eager tests (which cannot fail that way) and without a journal.
static void journal_recycle(fgpu_ctx* ctx) {
    for (JournalBatch* j : ctx->journal) ctx->journal_pool.push_back(j);
    ctx->journal.clear();
    ctx->journal_bytes = 0;
}

// Reset the junction map and scan every journalled batch again with all junction tests evaluated.  On return everything the journal holds
// has been walked; batches that were only prepared are walked as well (their turn has come: this is only reached from a walk or after one).
static int scan_replay_once(fgpu_ctx* ctx) {
    ctx->in_replay = true;
    ctx->journal_on = false;
    ctx->eager_scan = true;
    ctx->lazy_failed = false;
    int rc = fgpu_sync_all(ctx);
    const uint64_t reads_processed = ctx->scan_stats.reads_processed;      // the journal's batches have been counted: scan_pure_into does not see them again
    scan_rewind(ctx);      // (whatever sync_all said: no list of the voided walks stays where fgpu_scan_take_stops would find it)
    ctx->scan_stats.reads_processed = reads_processed;
    if (!rc) rc = fgpu_scan_reset(ctx);
    if (rc) { ctx->in_replay = false; return rc; }
    {   // what fgpu_diag_late_flags reports of the voided attempt (everything has completed: sync_all above)
        unsigned long long ln[3] = {0, 0, 0};
        if (hipMemcpy(ln, ctx->counters->late_n, sizeof(ln), hipMemcpyDeviceToHost) == hipSuccess)
            for (int i = 0; i < 3; i++) ctx->late_acc[i] += ln[i];
    }
    FGPU_HIP(hipMemsetAsync(ctx->counters, 0, sizeof(DevCounters), ctx->stream));
    // nothing is packed again, so the device's longest-read maximum (how far a piece reaches) comes back from what the journal's batches showed
    FGPU_HIP(hipMemcpyAsync(&ctx->counters->max_read_len, &ctx->journal_max_read_len, 8, hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    memset(&ctx->carried, 0, sizeof(ctx->carried));      // (fgpu_scan_begin leaves it to fgpu_scan_end: kept as found)
    if (ctx->have_import) {   // the table the previous shard handed over comes first again
        if ((rc = fgpu_scan_reserve(ctx, ctx->import_n)) || (rc = fgpu_scan_import_impl(ctx, ctx->import_copy.p, ctx->import_n))) { ctx->in_replay = false; return rc; }
        FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        ctx->scan_imported = ctx->import_n;
        if (ctx->import_has_carried) {
            ctx->carried = ctx->import_carried;
            ctx->scan_piece_base = ctx->import_carried.reads_no_errors;
        }
    }
    for (size_t i = 0; i < ctx->journal.size() && !rc; i++) {
        JournalBatch* j = ctx->journal[i];
        BatchBufs* b = acquire_batch(ctx);
        if (b->stops_pending && (rc = fgpu_scan_harvest(ctx, b))) {   // lists of the replayed batch these buffers held two batches ago
            ctx->pool.push_back(b);      // (FGPU_ERR_CAPACITY: a walk of this replay outgrew the table -- nothing of it applied; scan_replay goes again)
            break;
        }
        if (b->walk_pending) {
            FGPU_HIP(fgpu_sync_event(ctx, b->walk_done));
            b->walk_pending = false;
        }
        b->seq = j->seq;
        ctx->cur = b;
        b->T = j->T; b->n_words = j->n_words; b->n_reads = j->n_reads;
        b->d_offs = (const uint64_t*)j->offs.p;
        if (b->T && (rc = planes_bring(ctx, plane_bytes(b->n_words, 0, false), &b->codes, &b->bad, nullptr, j->codes.p, j->bad.p, nullptr, true))) break;
        uint64_t n_pieces = 0;
        rc = fgpu_stage_scan_pure(ctx, &n_pieces, true);      // (the replay: one range per batch)
        if (!rc) rc = fgpu_check_errors(ctx);
        if (!rc && b->pure_done) FGPU_HIP(hipEventRecord(b->pure_done, ctx->stream));
        if (!rc) rc = scan_walk_step(ctx, b, 0);
        ctx->pool.push_back(b);
    }
    ctx->cur = &ctx->bb_default;
    if (!rc) rc = fgpu_pull_counters(ctx);     // (still in_replay: an overflow of the last walks is reported here, to scan_replay, not flagged for later)
    ctx->in_replay = false;
    ctx->scan_replays++;
    return rc;
}

// ... on a table four times the size where the scan has outgrown it, and again should the replay itself outgrow that
static int scan_replay(fgpu_ctx* ctx) {
    for (int attempt = 0;; attempt++) {
        const bool for_room = ctx->capacity_failed;
        ctx->capacity_failed = false;
        if (for_room) {
            int rc = fgpu_sync_all(ctx);
            if (!rc) rc = fgpu_scan_regrow_empty(ctx, ctx->jcap * 4);
            if (rc) { ctx->lazy_failed = false; return rc; }
            ctx->capacity_replays++;
        }
        int rc = scan_replay_once(ctx);
        // the replay itself ran out of room (its batches are walked with the table kept below a quarter full between them, so this takes a
        // single batch that creates more than three times what the whole table held): once more, larger again.  (Noticed at the end of the
        // replay or where it harvests the lists of a batch it has walked: fgpu_scan_harvest applies none of them once the flag is up.)
        if (rc == FGPU_ERR_CAPACITY && (ctx->counters_host->error_flags & 1ULL) && ctx->jcap < (1ULL << 31) && attempt < 6) {
            ctx->capacity_failed = true;
            continue;
        }
        // The journal still holds every batch of the scan: it stays on, so that a later batch that outgrows the table is absorbed as well (the
        // scan is eager from here on and cannot fail the lazy way again)
        if (!rc && for_room) ctx->journal_on = true;
        return rc;
    }
}

static int journal_add(fgpu_ctx* ctx, BatchBufs* b) {
    if (!ctx->journal_on || ctx->in_replay) return FGPU_OK;
    const PlaneBytes n = plane_bytes(b->n_words, b->n_reads, ctx->record_stops);
    if (ctx->journal_bytes + n.all() > ctx->journal_budget) {
        // no room: everything walked so far is checked (and scanned again if need be), the rest of the scan is eager
        int rc = fgpu_pull_counters(ctx);
        if (rc) return rc;
        BatchBufs* const cur = ctx->cur;
        // the batch being packed has already been folded into the device's longest-read maximum (fgpu_stage_pack) and is not in the journal:
        // the replay restores that maximum from journal_max_read_len, so it has to know this batch's reads too
        ctx->journal_max_read_len = std::max<uint64_t>(ctx->journal_max_read_len, ctx->counters_host->max_read_len);
        if (ctx->lazy_failed && (rc = scan_replay(ctx))) return rc;
        ctx->cur = cur;
        ctx->journal_on = false;
        ctx->eager_scan = true;
        journal_recycle(ctx);
        return FGPU_OK;
    }
    JournalBatch* j;
    if (!ctx->journal_pool.empty()) { j = ctx->journal_pool.back(); ctx->journal_pool.pop_back(); }
    else j = new JournalBatch();
    if (int rc = planes_bring(ctx, n, &j->codes, &j->bad, &j->offs, b->codes.p, b->bad.p, b->d_offs, b->T != 0)) {
        ctx->journal_pool.push_back(j);
        return rc;
    }
    j->T = b->T; j->n_words = b->n_words; j->n_reads = b->n_reads; j->seq = b->seq;
    ctx->journal.push_back(j);
    ctx->journal_bytes += n.all();
    return FGPU_OK;
}

// one_range: the batch is prepared ahead of its turn -- nothing walks it beside its own pure stage, so its back half is not cut into ranges
static int scan_pure_into(fgpu_ctx* ctx, BatchBufs* b, const fgpu_reads* reads, bool one_range = false, const ResidentBatch* kept = nullptr) {
    if (b->stops_pending) {   // the buffers still hold the visit planes of an earlier batch: bring its lists to the host first
        int hrc = fgpu_scan_harvest(ctx, b);
        if (hrc) return hrc;      // (FGPU_INTERNAL_REPLAY: that batch's walk went wrong; the caller replays and comes back)
    }
    b->seq = ctx->scan_batch_seq++;
    ctx->cur = b;
    const double t_a = fgpu_host_now();
    if (b->walk_pending) {   // the walk stream may still be reading this batch's planes
        FGPU_HIP(fgpu_sync_event(ctx, b->walk_done));
        b->walk_pending = false;
    }
    const double t_b = fgpu_host_now();
    ctx->host_ms[0] += t_b - t_a;
    int rc = kept ? scan_take_kept(ctx, b, kept) : fgpu_stage_pack(ctx, reads);
    ctx->host_ms[1] += fgpu_host_now() - t_b;
    if (!rc) rc = journal_add(ctx, b);
    uint64_t n_pieces = 0;
    ctx->scan_take_kept = kept;
    if (!rc) rc = fgpu_stage_scan_pure(ctx, &n_pieces, one_range);   // ends with the batch's only synchronisation (piece count)
    ctx->scan_take_kept = nullptr;
    if (!rc) ctx->journal_max_read_len = std::max<uint64_t>(ctx->journal_max_read_len, ctx->counters_host->max_read_len);
    if (!rc) rc = fgpu_check_errors(ctx);
    if (!rc) ctx->scan_stats.reads_processed += b->n_reads;
    if (!rc && b->pure_done) FGPU_HIP(hipEventRecord(b->pure_done, ctx->stream));
    if (!rc && reads) rc = fgpu_host_batch_done(ctx, reads);
    return rc;
}

// every non-empty batch of the last load pass is resident with its read offsets (fgpu_scan_kept_state)
static bool kept_complete(const fgpu_ctx* ctx) {
    if (!ctx->keep_reads || ctx->phase == 1 || ctx->phase == 3 || ctx->resident_count != ctx->pass_batches) return false;
    for (uint64_t i = 0; i < ctx->resident_count; i++)
        if (!ctx->resident[i]->n_reads) return false;      // (a block adopted without its offsets: fgpu_load_batch_packed in such a pass)
    return true;
}

// kept batch i of the last load pass for a scan call `who`: after a plain pass every batch has to be there (fgpu_scan_kept_state); after a
// sliced pass that keeps reads a rank holds offsets for the batches it packed or adopted them for, and is asked batch by batch
static int kept_batch_at(fgpu_ctx* ctx, const char* who, uint64_t i, const ResidentBatch** out) {
    const std::string w(who);
    if (ctx->kept_sliced ? !ctx->keep_reads : !kept_complete(ctx)) {
        ctx->err = w + ": the last load pass did not keep every batch with its reads (FGPU_LOAD_KEEP_READS, all batches inside the resident budget of " +
                   std::to_string(ctx->resident_budget) + " bytes; " + std::to_string(ctx->resident_count) + " of " + std::to_string(ctx->pass_batches) + " batches are resident)";
        return FGPU_ERR_STATE;
    }
    if (i >= ctx->resident_count) { ctx->err = w + ": no such batch (empty batches keep nothing)"; return FGPU_ERR_ARG; }
    if (!ctx->resident[i]->n_reads) {
        ctx->err = w + ": batch " + std::to_string(i) + " is resident without its read offsets (packed by another rank: fgpu_load_slice_adopt_reads brings them)";
        return FGPU_ERR_STATE;
    }
    *out = ctx->resident[i];
    return FGPU_OK;
}

// pure stage + ordered walk of one batch, from its text (reads) or from a kept batch
static int scan_batch_from(fgpu_ctx* ctx, const fgpu_reads* reads, const ResidentBatch* kept) {
    int rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->lazy_failed && (rc = scan_replay(ctx))) return rc;      // an earlier walk met a preview it could not repair: scan again, eagerly
    BatchBufs* b = acquire_batch(ctx);
    rc = scan_pure_into(ctx, b, reads, false, kept);          // main stream; overlaps the previous batch's walk on the walk stream
    if (rc == FGPU_INTERNAL_REPLAY) {            // noticed while the buffers' previous lists were fetched: replay, then this batch from the start
        ctx->cur = &ctx->bb_default;
        ctx->pool.insert(ctx->pool.begin(), b);
        if ((rc = scan_replay(ctx))) return rc;
        b = acquire_batch(ctx);
        rc = scan_pure_into(ctx, b, reads, false, kept);
    }
    if (!rc && ctx->lazy_failed) {
        // noticed at this batch's own synchronisation: the batch is in the journal (prepared lazily); the replay scans it with the others
        ctx->cur = &ctx->bb_default;
        ctx->pool.push_back(b);
        return scan_replay(ctx);
    }
    if (!rc) rc = scan_walk_step(ctx, b, WALK_TIMED);      // counters as of the pure stage's synchronisation
    ctx->cur = &ctx->bb_default;
    ctx->pool.push_back(b);
    return rc;
}

// the pure stage of one batch ahead of its walk, from its text (reads) or from a kept batch: the batch joins the prepared ones
static int scan_prepare_from(fgpu_ctx* ctx, const fgpu_reads* reads, const ResidentBatch* kept) {
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    BatchBufs* b;
    if (!ctx->pool.empty()) { b = ctx->pool.front(); ctx->pool.erase(ctx->pool.begin()); }
    else b = new_batch(ctx);
    int rc = scan_pure_into(ctx, b, reads, true, kept);
    ctx->cur = &ctx->bb_default;
    if (rc == FGPU_INTERNAL_REPLAY) {   // (only after walks of this scan: prepare-only scans never get here)
        ctx->pool.insert(ctx->pool.begin(), b);
        if ((rc = scan_replay(ctx))) return rc;
        return scan_prepare_from(ctx, reads, kept);
    }
    if (rc) { ctx->pool.push_back(b); return rc; }
    b->planes_gen = ctx->hint_in_table ? ctx->hint_gen : 0;      // what this batch's snapshot planes speak of
    b->cand_gen = 0;
    ctx->prepared.push_back(b);
    return FGPU_OK;
}

extern "C" {

int fgpu_scan_resident_base(fgpu_ctx* ctx, uint64_t first_batch) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "scan_resident_base while a pass is open: between the load pass and fgpu_scan_begin"; return FGPU_ERR_STATE; }
    ctx->scan_resident_base = first_batch;
    return FGPU_OK;
}

int fgpu_scan_begin(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "scan_begin while another pass is open"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    int rc = fgpu_bg_join(ctx);      // the walk's streams and events (made beside pass 1, fgpu_create)
    if (rc) return rc;
    if ((rc = fgpu_offs_check_report(ctx))) return rc;
    if ((rc = fgpu_scan_alloc(ctx))) return rc;
    if ((rc = fgpu_scan_reset(ctx))) return rc;
    ctx->fixup_ready = false;   // the load pass' counters go with this reset
    FGPU_HIP(hipMemsetAsync(ctx->counters, 0, sizeof(DevCounters), ctx->stream));
    // ---- what only a fresh scan resets: a replay is the same scan going on, and keeps all of this ----
    // the journal itself, and whether the scan is lazy (the replay turns it eager)
    journal_recycle(ctx);
    ctx->journal_on = !(ctx->prm.flags & FGPU_FLAG_EAGER_FLAGS) && !ctx->eager_runtime;
    ctx->eager_scan = ctx->lazy_failed = ctx->capacity_failed = false;
    ctx->have_import = false;             // (the replay imports the kept table again)
    ctx->journal_max_read_len = 0;        // (the replay restores the device's maximum from it)
    // the numbering of batches and what the caller and the long pair filter have taken of them: the replayed batches keep their numbers
    ctx->scan_batch_seq = 0;
    ctx->stops_delivered = 0;
    ctx->lp_applied_seq = 0;
    ctx->dl_keys_n = 0;
    // diagnostics that speak of the whole scan, voided attempts included: late junction tests, host waits, refreshes and links of prepared batches
    ctx->late_acc[0] = ctx->late_acc[1] = ctx->late_acc[2] = 0;
    ctx->host_waits = 0;
    ctx->host_wait_ms = 0;
    ctx->wait_sites.clear();
    ctx->delta_keys = ctx->refresh_full = ctx->refresh_delta = ctx->refresh_mismatch = 0;
    ctx->sparse_links = ctx->full_links = 0;
    // the previews of a scan are numbered from 1 (prepared batches remember which one their planes speak of): kept as found
    ctx->hint_gen = 0;
    ctx->hint_n = ctx->hint_max_seq = 0;
    // the pair filters: a scan starts with empty ones, a replay's harvest applies only lists they have not seen (lp_applied_seq, stops_delivered)
    if (ctx->short_pf) FGPU_HIP(hipMemsetAsync(ctx->short_pf, 0, ctx->short_pf_tai / 8, ctx->stream));
    if ((rc = fgpu_long_pairs_reset(ctx))) return rc;
    // the environment switches read once per scan
    ctx->dbg_stall_us = getenv("FGPU_DEBUG_WALK_STALL_US") ? std::min(100000, std::max(0, atoi(getenv("FGPU_DEBUG_WALK_STALL_US")))) : 0;
    ctx->dbg_delta_check = getenv("FGPU_DEBUG_DELTA_CHECK") != nullptr;
    ctx->no_sparse_link = getenv("FGPU_NO_SPARSE_LINK") != nullptr;      // measurement aid: no candidate planes, every window of a prepared batch linked in full
    // ranges of the pure stage's back half (scan_pure.hip): n >= 8 forces 2^n positions per range (tests), 0 one range per batch -- the schedule
    // before there were ranges, also what FGPU_NO_OVERLAP=1 runs (the walk follows on the same stream); anything else: the default policy
    ctx->scan_range_log2 = -1;
    if (const char* e = getenv("FGPU_SCAN_RANGE_LOG2")) {
        char* end = nullptr;
        const long n = strtol(e, &end, 10);
        if (end == e || *end || (n != 0 && (n < 8 || n > 40))) {      // (empty, not a number, 1..7, beyond 2^40: no silent meaning)
            ctx->err = std::string("FGPU_SCAN_RANGE_LOG2=") + e + ": 0 (one range per batch) or 8..40 (ranges of 2^n positions)";
            return FGPU_ERR_ARG;
        }
        ctx->scan_range_log2 = (int)n;
    }
    if (fgpu_walk_no_overlap()) ctx->scan_range_log2 = 0;
    // ---- and what a replay starts from as well (last: a scan_begin that fails above leaves the previous scan's lists where they were) ----
    scan_rewind(ctx);
    ctx->cur = &ctx->bb_default;
    ctx->phase = 2;
    return FGPU_OK;
}

int fgpu_scan_kept_state(fgpu_ctx* ctx, int* complete, uint64_t* n_batches, uint64_t* n_reads, uint64_t* bytes) {
    if (!ctx) return FGPU_ERR_ARG;
    if (complete) *complete = kept_complete(ctx) ? 1 : 0;
    if (n_batches) *n_batches = ctx->resident_count;
    if (n_reads) *n_reads = ctx->kept_reads_total;
    if (bytes) *bytes = ctx->resident_bytes;
    return FGPU_OK;
}

int fgpu_scan_kept_range(fgpu_ctx* ctx, uint64_t lo, uint64_t hi, uint64_t max_read_len, int* complete) {
    if (!ctx || !complete) return FGPU_ERR_ARG;
    *complete = 0;
    if (ctx->phase != 0) { ctx->err = "scan_kept_range while a pass is open: between the load pass and fgpu_scan_begin"; return FGPU_ERR_STATE; }
    if (lo > hi) { ctx->err = "scan_kept_range: batches [lo, hi) with lo <= hi"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->stream) FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    if (int rc = fgpu_offs_check_report(ctx)) return rc;
    if (!ctx->keep_reads || hi > ctx->resident_count || (!ctx->kept_sliced && !kept_complete(ctx))) return FGPU_OK;
    for (uint64_t i = lo; i < hi; i++)
        if (!ctx->resident[i]->n_reads) return FGPU_OK;
    ctx->kept_max_read_len = std::max<uint64_t>(ctx->kept_max_read_len, max_read_len);      // the longest read of the PASS, over all ranks
    *complete = 1;
    return FGPU_OK;
}

int fgpu_scan_batch_kept(fgpu_ctx* ctx, uint64_t i, uint64_t* n_reads_out) {
    if (!ctx) return FGPU_ERR_ARG;
    int rc;
    if ((rc = need_scan(ctx, "scan_batch_kept")) || (rc = need_none_prepared(ctx, "scan_batch_kept")) || (rc = need_real_table(ctx))) return rc;
    const ResidentBatch* kept = nullptr;
    if ((rc = kept_batch_at(ctx, "scan_batch_kept", i, &kept))) return rc;
    if (n_reads_out) *n_reads_out = kept->n_reads;
    return scan_batch_from(ctx, nullptr, kept);
}

int fgpu_scan_batch(fgpu_ctx* ctx, const fgpu_reads* reads) {
    if (!ctx) return FGPU_ERR_ARG;
    int rc;
    if ((rc = need_scan(ctx, "scan_batch")) || (rc = need_none_prepared(ctx, "scan_batch")) || (rc = need_real_table(ctx))) return rc;
    if ((rc = fgpu_check_reads(ctx, reads))) return rc;
    return scan_batch_from(ctx, reads, nullptr);
}

int fgpu_scan_prepare(fgpu_ctx* ctx, const fgpu_reads* reads) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = need_scan(ctx, "scan_prepare")) return rc;
    int rc = fgpu_check_reads(ctx, reads);
    if (rc) return rc;
    return scan_prepare_from(ctx, reads, nullptr);
}

int fgpu_scan_prepare_kept(fgpu_ctx* ctx, uint64_t i, uint64_t* n_reads_out) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = need_scan(ctx, "scan_prepare_kept")) return rc;
    const ResidentBatch* kept = nullptr;
    if (int rc = kept_batch_at(ctx, "scan_prepare_kept", i, &kept)) return rc;
    if (n_reads_out) *n_reads_out = kept->n_reads;
    return scan_prepare_from(ctx, nullptr, kept);
}

// Read shards: a FRESHER preview has taken the place of the one the batches were prepared against (fgpu_scan_import_hint again: the table the
// shard below was handed, one hop before this shard's own arrives) -- the snapshot planes of every prepared batch are made again against it,
// off the chain of walks.  When the real table arrives it differs from this preview by the keys ONE shard created, and the walk only has to
// look for those (fgpu_scan_import_table).
int fgpu_scan_refresh_prepared(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = need_scan(ctx, "scan_refresh_prepared")) return rc;
    if (!ctx->hint_in_table) { ctx->err = "scan_refresh_prepared without a preview in the table (fgpu_scan_import_hint)"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const bool no_sparse = ctx->no_sparse_link;
    for (BatchBufs* b : ctx->prepared) {
        if (b->planes_gen != ctx->hint_gen) {
            if (int rc = fgpu_scan_refresh_planes(ctx, b)) return rc;
            b->planes_gen = ctx->hint_gen;
            b->cand_gen = 0;
        }
        // ... and, while this rank still waits, the plane that lets its walk link a window by visiting candidates only (round 6, k_walk_link_sparse)
        if (!no_sparse && b->cand_gen != ctx->hint_gen)
            if (int rc = fgpu_scan_build_cand(ctx, b)) return rc;
    }
    ctx->launch_stream = ctx->stream;
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}

int fgpu_scan_walk_prepared(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    int rc;
    if ((rc = need_scan(ctx, "scan_walk_prepared")) || (rc = need_real_table(ctx))) return rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->lazy_failed) return scan_replay(ctx);      // (walks the prepared batches as well)
    // The batches were prepared before their turn: their snapshot planes speak of a table that has since been replaced (the preview by the real
    // table) and walked on, so they are made again by the walk stream right before every batch's walk (refresh_snapshot; making batch i + 1's
    // beside batch i's walk instead was measured and is no faster: DESIGN.md section 10, profiles/r05_hop_refresh_ab.txt).
    for (size_t i = 0; i < ctx->prepared.size() && !rc; i++) {
        BatchBufs* b = ctx->prepared[i];
        if (i > 0) {   // feedback for the window controller and for the size of the junction table between batches
            if ((rc = fgpu_pull_counters(ctx))) break;                  // (the walk of batch i - 1 has finished; so have the planes of batch i)
            if (ctx->lazy_failed) { ctx->cur = &ctx->bb_default; return scan_replay(ctx); }
        }
        ctx->cur = b;
        rc = scan_walk_step(ctx, b, i > 0 ? WALK_REFRESH : WALK_REFRESH | WALK_NO_FEEDBACK);
    }
    ctx->cur = &ctx->bb_default;
    for (BatchBufs* b : ctx->prepared) ctx->pool.push_back(b);
    ctx->prepared.clear();
    return rc;
}

int fgpu_scan_set_eager(fgpu_ctx* ctx, int on) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_scan_set_eager while a pass is open"; return FGPU_ERR_STATE; }
    ctx->eager_runtime = on != 0;
    return FGPU_OK;
}

// ---- the short pair filter on the device ---------------------------------------------------------------------------------
int fgpu_scan_short_pairs(fgpu_ctx* ctx, uint64_t tai, int32_t n_hash, int32_t lists_to_host) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_scan_short_pairs while a pass is open"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->short_pf) {
        FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        FGPU_HIP(hipFree(ctx->short_pf));
        ctx->short_pf = nullptr;
        ctx->short_pf_tai = 0;
    }
    if (!tai) return FGPU_OK;
    if (!ctx->record_stops) { ctx->err = "fgpu_scan_short_pairs needs FGPU_FLAG_RECORD_STOPS"; return FGPU_ERR_STATE; }
    if (!fgpu_is_pow2(tai) || tai < 128 || n_hash < 1 || n_hash > 32) { ctx->err = "fgpu_scan_short_pairs: tai must be a power of two >= 128, n_hash 1..32"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipMalloc(&ctx->short_pf, tai / 8));
    FGPU_HIP(hipMemsetAsync(ctx->short_pf, 0, tai / 8, ctx->stream));
    ctx->short_pf_tai = tai;
    ctx->short_pf_hashes = n_hash;
    ctx->short_pf_lists_to_host = lists_to_host != 0;
    return FGPU_OK;
}

int fgpu_scan_short_pairs_download(fgpu_ctx* ctx, uint8_t* out, uint64_t n_bytes) {
    if (!ctx || !out) return FGPU_ERR_ARG;
    if (!ctx->short_pf) { ctx->err = "fgpu_scan_short_pairs_download without fgpu_scan_short_pairs"; return FGPU_ERR_STATE; }
    if (ctx->phase != 0) { ctx->err = "fgpu_scan_short_pairs_download while a pass is open"; return FGPU_ERR_STATE; }
    if (n_bytes != ctx->short_pf_tai / 8) { ctx->err = "fgpu_scan_short_pairs_download: the filter has tai / 8 bytes"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    FGPU_HIP(hipMemcpyAsync(out, ctx->short_pf, n_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}

int fgpu_scan_take_stops(fgpu_ctx* ctx, fgpu_stop* out, uint64_t cap, uint64_t* n_out, int64_t* batch_seq) {
    if (!ctx || !n_out || !batch_seq) return FGPU_ERR_ARG;
    if (!ctx->record_stops) { ctx->err = "fgpu_scan_take_stops needs FGPU_FLAG_RECORD_STOPS"; return FGPU_ERR_STATE; }
    *n_out = 0;
    *batch_seq = -1;
    if (ctx->phase == 2 && ctx->lazy_failed) {
        if (int rc = scan_replay(ctx)) return rc;
    }
    if (ctx->stop_queue.empty() && !ctx->to_harvest.empty()) {
        FGPU_HIP(hipSetDevice(ctx->prm.device));
        int rc = fgpu_scan_harvest(ctx, ctx->to_harvest.front());
        if (rc == FGPU_INTERNAL_REPLAY && ctx->phase == 2) {
            if ((rc = scan_replay(ctx))) return rc;
            if (!ctx->to_harvest.empty()) rc = fgpu_scan_harvest(ctx, ctx->to_harvest.front());
        }
        if (rc) return rc;
    }
    if (ctx->stop_queue.empty()) return FGPU_OK;
    StopBatch& sb = ctx->stop_queue.front();
    *n_out = sb.n;
    *batch_seq = (int64_t)sb.seq;
    if (sb.n > cap || (sb.n && !out)) return FGPU_ERR_CAPACITY;
    if (sb.n) memcpy(out, sb.data, sb.n * sizeof(fgpu_stop));
    ctx->stops_delivered = sb.seq + 1;
    if (sb.data) { StopBatch f; f.data = sb.data; f.cap = sb.cap; ctx->stop_pool.push_back(f); }
    ctx->stop_queue.pop_front();
    return FGPU_OK;
}

int fgpu_scan_end(fgpu_ctx* ctx, fgpu_scan_stats* stats) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 2) { ctx->err = "scan_end without scan_begin"; return FGPU_ERR_STATE; }
    static const bool dbg_host = getenv("FGPU_DEBUG_HOST") != nullptr;
    static const bool dbg_waits = getenv("FGPU_DEBUG_WAITS") != nullptr;
    struct TellWaits {      // (at the very end of the call: the last walks and harvests are waited for inside it)
        fgpu_ctx* c;
        bool on;
        ~TellWaits() {
            if (!on) return;
            for (const WaitSite& w : c->wait_sites) {
                const char* f = strrchr(w.file, '/');
                fprintf(stderr, "[waits] %-14s:%-5d %6llu times %9.2f ms\n", f ? f + 1 : w.file, w.line, (unsigned long long)w.n, w.ms);
            }
        }
    } tell_waits{ctx, dbg_waits};
    if (dbg_host) {
        fprintf(stderr, "[host] scan: wait for the buffers' last walk %.2f ms, pack issue %.2f, pure stage issue (first half) %.2f, wait for the piece count %.2f, "
                        "pure stage issue (second half) %.2f, walk issue %.2f\n", ctx->host_ms[0], ctx->host_ms[1], ctx->host_ms[2], ctx->host_ms[3], ctx->host_ms[4], ctx->host_ms[5]);
        for (double& v : ctx->host_ms) v = 0;
    }
    int rc = fgpu_pull_counters(ctx);
    if (!rc && ctx->lazy_failed) {                          // the last walks met a preview they could not repair: scan again before closing
        rc = scan_replay(ctx);
        if (!rc) rc = fgpu_pull_counters(ctx);
    }
    while (!rc && !ctx->to_harvest.empty()) rc = fgpu_scan_harvest(ctx, ctx->to_harvest.front());   // every walk has finished
    if (!rc) rc = fgpu_long_pairs_close(ctx);              // the last batch of lists: its rounds' outcome, a first end left without a mate
    ctx->phase = 0;
    ctx->journal_on = false;
    if (!rc) ctx->span.end_scan(ctx->prm.walk_window_span, ctx->scan_windows);
    if (rc) return rc;
    const DevCounters& c = *ctx->counters_host;
    fgpu_scan_stats& s = ctx->scan_stats;
    s.unambiguous_reads = c.segments + ctx->carried.unambiguous_reads;
    s.reads_no_errors = c.pieces + ctx->carried.reads_no_errors;
    s.nb_jcheck_kmer = c.nb_jcheck + ctx->carried.nb_jcheck_kmer;
    s.nb_no_juncs = c.nb_no_juncs + ctx->carried.nb_no_juncs;
    s.nb_processed = c.nb_processed + ctx->carried.nb_processed;
    s.nb_skipped = c.nb_skipped + ctx->carried.nb_skipped;
    s.n_junctions = c.n_junctions + ctx->scan_imported;
    s.kmers = c.kmers + ctx->carried.kmers;
    s.reads_processed += ctx->carried.reads_processed;
    s.walk_windows = ctx->scan_windows;
    s.walk_followers = c.followers;
    s.walk_max_cluster = c.max_cluster;
    s.flag_positions = c.flag_positions;
    s.piece_positions = c.piece_positions;
    s.valid_reused = c.valid_reused;
    s.flags_filled = c.flags_filled;
    s.walk_parallel = c.walk_parallel;
    memset(&ctx->carried, 0, sizeof(ctx->carried));
    if (stats) *stats = s;
    return FGPU_OK;
}

int fgpu_scan_junction_count(fgpu_ctx* ctx, uint64_t* n) {
    if (!ctx || !n) return FGPU_ERR_ARG;
    if (int rc = fgpu_sync_all(ctx)) return rc;
    return fgpu_scan_download_impl(ctx, nullptr, nullptr, 0, n);
}

int fgpu_scan_download_junctions(fgpu_ctx* ctx, uint64_t* keys, fgpu_junction* recs, uint64_t cap, uint64_t* n_out) {
    if (!ctx || !keys || !recs || !n_out) return FGPU_ERR_ARG;
    if (!ctx->jkeys) { *n_out = 0; return FGPU_OK; }
    if (int rc = fgpu_sync_all(ctx)) return rc;
    return fgpu_scan_download_impl(ctx, keys, recs, cap, n_out);
}

int fgpu_scan_table_entries(fgpu_ctx* ctx, uint64_t* n_entries) { return fgpu_scan_junction_count(ctx, n_entries); }

int fgpu_scan_dump_order(fgpu_ctx* ctx, const uint64_t* rehash_counts, const uint64_t* rehash_buckets, uint64_t n_rehashes, uint64_t n, uint32_t* order) {
    if (!ctx || !rehash_counts || !rehash_buckets || !n_rehashes || (n && !order)) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_scan_dump_order while a pass is open"; return FGPU_ERR_STATE; }
    if (!ctx->dl_keys_n || n > ctx->dl_keys_n) { ctx->err = "fgpu_scan_dump_order works on the keys of the last fgpu_scan_download_junctions (at most that many)"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    return fgpu_scan_dump_order_impl(ctx, (const uint64_t*)ctx->dl_keys.p, rehash_counts, rehash_buckets, n_rehashes, n, order);
}

int fgpu_scan_export_table(fgpu_ctx* ctx, void* dev_buf, uint64_t buf_bytes, uint64_t* n_entries) {
    if (!ctx || !dev_buf || !n_entries) return FGPU_ERR_ARG;
    uint64_t n = 0;
    int rc = fgpu_sync_all(ctx);   // walks still running on the walk stream are part of the table
    if (!rc) rc = fgpu_scan_junction_count(ctx, &n);
    if (rc) return rc;
    if (buf_bytes < n * FGPU_TABLE_ENTRY_BYTES) { ctx->err = "export buffer too small"; return FGPU_ERR_CAPACITY; }
    if ((rc = fgpu_ensure(ctx, &ctx->export_stamps, n * 8 + 8))) return rc;
    return fgpu_scan_export_impl(ctx, dev_buf, n, (uint64_t*)ctx->export_stamps.p, n_entries);
}

int fgpu_scan_import_table(fgpu_ctx* ctx, const void* dev_buf, uint64_t n_entries, const fgpu_scan_stats* carried) {
    if (!ctx || (n_entries && !dev_buf)) return FGPU_ERR_ARG;
    if (int rc = need_scan(ctx, "import_table")) return rc;
    int rc = fgpu_sync_all(ctx);
    if (rc) return rc;
    ctx->delta_ready = false;
    if (ctx->hint_in_table) {   // the preview has done its work (the prepared batches' planes): the real table takes its place
        if ((rc = fgpu_scan_clear_table(ctx))) return rc;
        ctx->hint_in_table = false;
        // If every prepared batch's planes speak of the newest preview and this table is a LATER STATE of it (the caller's promise, checked by
        // counting: the entries with a creation stamp beyond the preview's are exactly the surplus), the walk merges the new keys into the planes
        // through a filter of just those keys instead of probing the whole table's filter at every position again (22 -> ~7 ms per 25 M reads).
        static const bool no_delta = getenv("FGPU_NO_DELTA_REFRESH") != nullptr;
        bool all = ctx->hint_gen != 0 && !ctx->prepared.empty() && !no_delta && n_entries >= ctx->hint_n;
        for (BatchBufs* b : ctx->prepared) all = all && b->planes_gen == ctx->hint_gen;
        const uint64_t surplus = all ? n_entries - ctx->hint_n : 0;
        if (all && surplus <= (1ULL << 23)) {
            uint64_t bits = 1ULL << 20;      // (room for what this shard's own batches will add: they join the filter as they are walked)
            // (32 bits of filter per new key, swept in round 6 on config 4's hop, 8 / 16 / 32 / 64 bits per key: the merge 16.4 / 14.4 / 13.0 / 13.9 ms, the
            // link by the candidate plane -- which takes the filter's hits -- 11.6 / 9.7 / 8.7 / 8.2 ms, the hop 71.1 / 67.6 / 64.8 / 66.0 ms: false hits cost more than cache misses)
            while (bits < 32 * surplus) bits <<= 1;
            if ((rc = fgpu_ensure(ctx, &ctx->delta_filter, bits / 8))) return rc;
            FGPU_HIP(hipMemsetAsync(ctx->delta_filter.p, 0, bits / 8, ctx->stream));
            uint64_t max_seq = 0, newer = 0, digest[2] = {0, 0};
            if ((rc = fgpu_scan_import_probe(ctx, dev_buf, n_entries, ctx->hint_max_seq, (uint32_t*)ctx->delta_filter.p, bits, &max_seq, &newer, digest))) return rc;
            // a later state of the preview: as many newer entries as the surplus, AND the others are the preview's keys (their digest)
            if (newer == surplus && digest[0] == ctx->hint_digest[0] && digest[1] == ctx->hint_digest[1]) {
                ctx->delta_ready = true;
                ctx->delta_filter_bits = bits;
                ctx->delta_keys = newer;
            }
        }
    }
    if ((rc = fgpu_scan_reserve(ctx, ctx->counters_host->n_junctions + ctx->scan_imported + n_entries))) return rc;
    rc = fgpu_scan_import_impl(ctx, dev_buf, n_entries);
    if (rc) return rc;
    if (ctx->journal_on) {   // a replay starts from this table again
        if ((rc = fgpu_ensure(ctx, &ctx->import_copy, n_entries * FGPU_TABLE_ENTRY_BYTES + 16))) return rc;
        if (n_entries) FGPU_HIP(hipMemcpyAsync(ctx->import_copy.p, dev_buf, n_entries * FGPU_TABLE_ENTRY_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->import_n = n_entries;
        ctx->have_import = true;
        ctx->import_has_carried = carried != nullptr;
        if (carried) ctx->import_carried = *carried;
    }
    // the import runs on the main stream, the ordered walk on the walk stream behind events recorded BEFORE this call
    // (end of each prepared batch's pure stage): without this wait the walk would start on a half-imported table
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    ctx->scan_imported += n_entries;
    if (carried) ctx->carried = *carried;
    // creation stamps of this shard must sort after everything imported
    ctx->scan_piece_base = std::max<uint64_t>(ctx->scan_piece_base, carried ? carried->reads_no_errors : 0);
    return FGPU_OK;
}

int fgpu_scan_import_hint(fgpu_ctx* ctx, const void* dev_buf, uint64_t n_entries) {
    if (!ctx || (n_entries && !dev_buf)) return FGPU_ERR_ARG;
    if (int rc = need_scan(ctx, "import_hint")) return rc;
    if (ctx->scan_windows || ctx->scan_imported) {
        ctx->err = "import_hint comes before any walk and before the real table (batches prepared earlier have simply seen an empty table)";
        return FGPU_ERR_STATE;
    }
    int rc = fgpu_sync_all(ctx);
    if (rc) return rc;
    if (ctx->hint_in_table && (rc = fgpu_scan_clear_table(ctx))) return rc;      // a fresher preview takes the place of an older one
    if ((rc = fgpu_scan_reserve(ctx, n_entries))) return rc;
    if ((rc = fgpu_scan_import_impl(ctx, dev_buf, n_entries))) return rc;
    uint64_t newer = 0;
    ctx->hint_max_seq = 0;
    if ((rc = fgpu_scan_import_probe(ctx, dev_buf, n_entries, ~0ULL, nullptr, 0, &ctx->hint_max_seq, &newer, ctx->hint_digest))) return rc;
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    ctx->hint_in_table = true;
    ctx->hint_n = n_entries;
    ctx->hint_gen++;
    return FGPU_OK;
}

}  // extern "C"
