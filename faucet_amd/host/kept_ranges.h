// kept_ranges.h — pass 2's shards over the batches pass 1 kept, where the stream came from a pipe (shard_host.h, --scan_kept under filter slices).
//
// After a sliced pass 1 every rank holds every batch of the stream; a piped stream has no byte ranges to shard, so pass 2 is cut into N
// contiguous ranges of the global batch number g, balanced by stream positions: range r ends behind the first g at which the running sum of
// T reaches (r + 1) * total / N (integer arithmetic).  Ranges may be empty (more ranks than batches, one huge batch).  With `group` = 2
// (--paired_ends: reads 2p and 2p + 1 of the scan are a pair, and every rank counts its own reads from 0) a range also ends only where the
// reads so far are a multiple of the group.  The last range always ends behind the last batch.
// One pure function of the board's (T, n_reads) values: every rank computes the same bounds.  The standard library only, so that it can be
// tested alone.
#pragma once
#include <stdint.h>

#include <vector>

namespace faucet_host {

// n + 1 bounds: rank r scans the global batches [bounds[r], bounds[r + 1]).  n_reads may be empty when group <= 1.
inline std::vector<uint64_t> kept_scan_ranges(const std::vector<uint64_t>& T, const std::vector<uint64_t>& n_reads, int n, uint64_t group) {
    const uint64_t G = (uint64_t)T.size();
    if (n < 1) n = 1;
    std::vector<uint64_t> bounds((size_t)n + 1, G);
    bounds[0] = 0;
    uint64_t total = 0;
    for (uint64_t t : T) total += t;
    uint64_t g = 0, run = 0, reads = 0;
    for (int r = 0; r < n - 1; r++) {
        // (r + 1) * total / n without the product leaving 64 bits
        const uint64_t q = (uint64_t)(r + 1), target = total / (uint64_t)n * q + total % (uint64_t)n * q / (uint64_t)n;
        while (g < G && (run < target || (group > 1 && reads % group != 0))) {
            run += T[(size_t)g];
            if (group > 1) reads += n_reads[(size_t)g];
            g++;
        }
        bounds[(size_t)r + 1] = g;
    }
    return bounds;
}

}  // namespace faucet_host
