// span_control_check.cpp — drives the window-span controller (faucet_amd/csrc/walk_span.h) from a script on stdin, for tests/test_span_control_cpu.py.
// One command per line, one line of state per command:
//   new MAX_SPAN                        a context's controller as fgpu_create leaves it
//   begin FIXED                         start of a scan (FIXED: fgpu_params.walk_window_span, 0 = adaptive)
//   batch FOLLOWERS PIECES OVERFLOWS FIXED   the host's counters after a batch (totals of the scan, as the device counts them)
//   look FOLLOWERS PIECES OVERFLOWS     the three values read back behind a window; the span it leaves is the next window's (a batch of one window)
//   end FIXED WINDOWS                   end of a scan that walked WINDOWS windows
#include <stdio.h>
#include <string.h>

#include "walk_span.h"

int main() {
    WalkSpan c;
    char cmd[16];
    unsigned long long a, b, d, e;
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        a = b = d = e = 0;
        if (sscanf(line, "%15s %llu %llu %llu %llu", cmd, &a, &b, &d, &e) < 1) continue;
        if (!strcmp(cmd, "new")) { c = WalkSpan(); c.max_span = a; }
        else if (!strcmp(cmd, "begin")) c.begin_scan(a);
        else if (!strcmp(cmd, "batch")) c.after_batch(a, b, d, e, false);
        else if (!strcmp(cmd, "look")) {
            if (c.calib_left > 0) {      // (the caller's test, with the fixed span's: fgpu_stage_scan_walk looks only while looks are left)
                uint64_t span = c.window_span;
                c.after_window(a, b, d, &span, false);
                c.window_span = span;
            }
        }
        else if (!strcmp(cmd, "end")) c.end_scan(a, b);
        else { fprintf(stderr, "unknown command: %s\n", cmd); return 2; }
        printf("span=%llu looks=%d vote=%d ceiling=%llu proven=%llu settled=%llu adapt_pieces=%llu calib_pieces=%llu\n", (unsigned long long)c.window_span, c.calib_left,
               c.adapt_vote, (unsigned long long)c.span_ceiling, (unsigned long long)c.proven_span, (unsigned long long)c.settled_span,
               (unsigned long long)c.adapt_pieces, (unsigned long long)c.calib_p);
    }
    return 0;
}
