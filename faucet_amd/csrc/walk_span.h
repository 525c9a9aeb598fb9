// walk_span.h — the window-span controller of the ordered walk: its state and its four decisions.
// Host only, integer arithmetic on three counters of the device, no HIP: tests/test_span_control_cpu.py drives it from a program of its own.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

// Scheduling windows of the ordered walk, in stream positions.  A window grows (x4, up to FGPU_MAX_SPAN) while fewer than a third of its
// pieces queue behind another piece of their cluster and is halved above a half.  Since the walk takes its in-map bits from the batch's
// snapshot planes and registers the keys created since then per window (round 2), a window's fixed costs -- the delta registrations, five
// launches -- weigh more than the longer clusters of a larger window: config 2 measured 131.3 / 127.0 / 126.0 ms per step at 2^24 / 2^25 /
// 2^26 positions (16 % / 27 % / 36 % of the pieces queueing; round 1's look-up kernel per window had its optimum at 2^24; round 4, with
// dynamic cluster hand-out and no event brackets: 121.9 / 117.4 / 118.7 ms at 25 % / 43 % / 58 %).  How the size moves from batch to batch:
// WalkSpan::after_batch, from window to window while the host still looks at each: WalkSpan::after_window.  The window
// tables are sized for the context's bound, FGPU_MAX_SPAN (2 GiB) for filters up to 2^30 bits, more for larger ones (fgpu_create).
#define FGPU_USUAL_SPAN (1ULL << 26)
#define FGPU_MAX_SPAN (1ULL << 26)

struct WalkSpan {
    uint64_t window_span = 1ULL << 17;   // adaptive: stream positions per scheduling window
    uint64_t max_span = FGPU_MAX_SPAN;   // upper bound of window_span (sizes the window table)
    uint64_t settled_span = 0;           // window_span at the end of the context's previous scan (0: none yet): where the next one starts from
    uint64_t proven_span = 0;            // largest window size a batch of this context was walked at without most pieces queueing
    uint64_t span_ceiling = ~0ULL;       // a size at which the large-cluster walks' tables overflowed in this scan: the windows do not grow to it again
    int calib_left = 0;                  // windows the controller still waits for individually (start of a scan, after a bad batch)
    uint64_t calib_f = 0, calib_p = 0;   // followers and walked pieces as of the last look at a window ...
    uint64_t calib_ovf = 0;              // ... and ko_overflows (a window whose large clusters outgrew the large-cluster walks' tables)
    uint64_t adapt_followers = 0, adapt_pieces = 0, adapt_overflows = 0;   // the same three as of the last batch
    int adapt_vote = 0;                  // what the last batch's counters asked for without getting it yet (-1 smaller, +1 larger)
    bool repeats_seen_before = false;    // this scan's counters have shown repeats (kept while a lagging snapshot shows too few pieces to judge)

    // Start of a scan, and of a replay.  fixed: fgpu_params.walk_window_span (0 = adaptive).  What the context has learnt stays: max_span,
    // settled_span, proven_span.
    void begin_scan(uint64_t fixed) {
        // calibrated upwards window by window; a context that has scanned before starts a quarter below where that scan ended up
        const uint64_t start_span = std::max<uint64_t>(1ULL << 18, settled_span / 4);
        window_span = fixed ? std::min<uint64_t>(std::max<uint64_t>(fixed, 64), max_span) : std::min<uint64_t>(start_span, max_span);
        calib_left = 16;
        calib_f = calib_p = calib_ovf = 0;
        adapt_followers = adapt_pieces = adapt_overflows = 0;
        adapt_vote = 0;
        span_ceiling = ~0ULL;
        repeats_seen_before = false;
    }

    // After a batch: adapt the scheduling window to the data.  Larger windows mean fewer launches and fuller kernels but longer
    // dependency chains inside the clusters; measured on config 2 the step time keeps falling until about a third of the
    // pieces queue behind an earlier piece of their cluster (2^21: 254 ms, 2^22: 225, 2^23: 213, 2^24: 207, 2^25: 205).
    // The three counters (DevCounters::followers_seen, walked_pieces, ko_overflows) must be fresh with respect to the walks issued so far.
    void after_batch(uint64_t followers_seen, uint64_t walked_pieces, uint64_t ko_overflows, uint64_t fixed, bool dbg) {
        // Round 4.  On config 2 the share of queueing pieces is 0.25 / 0.43 / 0.58 at 2^24 / 2^25 / 2^26 positions and one batch's counters are a
        // noisy sample of it, so the controller of rounds 1-3 moved the size up and down between batches for good -- and every move asked the
        // host to wait for the next windows one by one, which keeps it from feeding the next batch's pure stage: 12 waits per step
        // (scripts/timeline.py), 121.4-122.1 ms a step against 116.8-118.9 with any fixed size in that range (scripts/span_fixed_ab.sh).
        // Now: both counts come from one snapshot of the device's counters (pieces counted behind their window's walks); growing on a share that
        // is not clear-cut (0.15-1/3) has to be asked for by two batches running; growing waits for windows only beyond the largest size a batch
        // of this context has been walked at, shrinking only towards a size it has not walked yet or when most pieces queue (the percolation
        // case the waits are for).  The thresholds themselves are unchanged, and shrinking still acts at once: a wider dead band, decisions held
        // back for a batch or two (shrinking included) and x4 steps were tried as well -- they walked config 4 at larger windows than suit it
        // and config 3's repeats at a percolating size now and then (pass 2 of 170 ms at 310-360).
        const uint64_t f = followers_seen - adapt_followers;
        const uint64_t p = walked_pieces - adapt_pieces;
        if (p == 0 || fixed) return;      // (no window has been completed since the last look at the counters)
        const uint64_t usual = std::min<uint64_t>(std::min<uint64_t>(max_span, FGPU_USUAL_SPAN), span_ceiling);
        int want = 0;             // -1 smaller, +1 larger
        bool clear = false;
        if (f * 2 > p) { want = -1; clear = f * 5 > p * 4; }
        else if (f * 3 < p) { want = 1; clear = f * 20 < p * 3; }
        // too large is dear (a batch at a percolating size), too small is not: shrinking acts at once, growing on a clear share or the second time
        const bool act = want < 0 || (want > 0 && (clear || adapt_vote > 0));
        adapt_vote = act ? 0 : want;
        if (want >= 0) proven_span = std::max(proven_span, window_span);
        if (ko_overflows > adapt_overflows && window_span > 4096) {
            // a window's large clusters outgrew the tables of the large-cluster walks and were walked piece after piece by their one thread:
            // far too large a window for this data
            window_span = std::max<uint64_t>(4096, window_span / 4);
            proven_span = std::min(proven_span, window_span);
            span_ceiling = std::min(span_ceiling, window_span * 2);     // (this scan does not grow to that size again)
            calib_ovf = ko_overflows;
            calib_left = 0;
        }
        else if (act && want < 0 && window_span > 4096) {
            window_span /= 2;
            // ... and look again window by window -- unless this context has walked a batch at the smaller size before and the share is not
            // the percolation case (most pieces queueing) the looks are for
            if (clear || window_span > proven_span) calib_left = 8;
            proven_span = std::min(proven_span, window_span);
        }
        else if (act && want > 0 && window_span < usual) {
            // clusters percolate at a sharp threshold (about one genome coverage per window): a whole batch at a size that turns out to be
            // beyond it costs seconds, so the first windows at a size this context has not walked yet are looked at one by one
            window_span = std::min<uint64_t>(window_span * 2, usual);
            if (window_span > proven_span) calib_left = std::max(calib_left, 2);
        }
        else if (f * 16 < p && window_span < std::min<uint64_t>(max_span, span_ceiling)) window_span *= 2;   // thin coverage per window: see FGPU_MAX_SPAN
        if (dbg) fprintf(stderr, "[span] batch: followers %llu of %llu pieces -> span %llu, looks %d, vote %d\n", (unsigned long long)f, (unsigned long long)p,
                         (unsigned long long)window_span, calib_left, adapt_vote);
        adapt_followers = followers_seen;
        adapt_pieces = walked_pieces;
        adapt_overflows = ko_overflows;
    }

    // After a window, while looks are left (calib_left > 0, no fixed span: the caller's test).  Calibration: at the start of a scan (and again
    // whenever a batch came out with most of its pieces queueing) the host waits for the window it has just issued and looks at the share of
    // pieces that had to queue behind an earlier piece of their cluster.  High coverage makes clusters percolate -- 250x reads of a small
    // genome were 20x slower with the 4 M position windows that suit 50x data -- and a whole batch is too long to walk with the wrong size.
    // The three values are DevCounters::followers, walked_pieces and ko_overflows as read back behind that window.
    // *span_now: the span of the batch's windows so far, and of those that follow (window_span itself moves when the batch's walk has been issued).
    void after_window(uint64_t followers, uint64_t walked_pieces, uint64_t ko_overflows, uint64_t* span_now, bool dbg) {
        uint64_t span = *span_now;
        const uint64_t f = followers - calib_f, p = walked_pieces - calib_p;
        if (ko_overflows > calib_ovf && span > 4096) {
            // the window's large clusters outgrew the tables of the large-cluster walks (their pieces do not queue, so the share of
            // followers says nothing about them) and were walked by one thread each: far too large a window for this data -- a quarter,
            // and the next windows are looked at as well (round 4: read pairs inside repeats at 600x, a 36 MB file whose windows grew to
            // 2^23 positions within its three batches: pass 2 2.0 s, 0.8 s with windows of 2^20)
            calib_ovf = ko_overflows;
            calib_f = followers;
            calib_p = walked_pieces;
            span = std::max<uint64_t>(4096, span / 4);
            proven_span = std::min(proven_span, span);
            calib_left = std::max(calib_left, 4);
            span_ceiling = std::min(span_ceiling, span * 2);     // (this scan does not grow to that size again)
            if (dbg) fprintf(stderr, "[span] look: the large-cluster walks' tables overflowed -> span %llu, looks left %d\n", (unsigned long long)span, calib_left);
        } else if (p >= 64) {
            calib_f = followers;
            calib_p = walked_pieces;
            bool shrunk = false;
            const uint64_t ceiling = std::min<uint64_t>(max_span, span_ceiling), usual = std::min<uint64_t>(ceiling, FGPU_USUAL_SPAN);
            if (f * 2 > p && span > 4096) { span /= 2; shrunk = true; }
            else if (f * 3 < p && span < usual) span = std::min<uint64_t>(span * 4, usual);
            else if (f * 16 < p && span < ceiling) span = std::min<uint64_t>(span * 4, ceiling);
            else calib_left = 1;          // settled
            calib_left--;
            // waiting for a window keeps the host from feeding the pure stage of the next batch: worth it while windows are small
            // (a fraction of a millisecond each, and the wrong size hurts most there); from 2^22 positions on the per-batch
            // controller (after_batch, no waiting) takes over unless the last look said "too large"
            if (!shrunk && span >= (1ULL << 22)) calib_left = 0;
            if (dbg) fprintf(stderr, "[span] look: followers %llu of %llu pieces -> span %llu, looks left %d\n", (unsigned long long)f, (unsigned long long)p,
                             (unsigned long long)span, calib_left);
        }
        *span_now = span;
    }

    // End of a scan that went well: where the context's next scan starts from, if this one has walked enough windows to have an opinion
    void end_scan(uint64_t fixed, uint64_t windows) {
        if (!fixed && windows > 8) settled_span = window_span;
    }
};
