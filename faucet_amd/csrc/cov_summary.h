// cov_summary.h — what a cleaning step reads of a contig's coverage list, and how it joins: the one definition the kernel (k_cov_calls,
// stage3_join.hip), the host's plans and the tests' C++ check (tests/host/chimera_plan_check.cpp, its fold mode) share.  No HIP is needed to include it.
//   ContigJuncList::getAvgCoverage   utils/ContigJuncList.cpp:162-172   (double) sum / (double) size
//   ContigJuncList::concatenate      utils/ContigJuncList.cpp:107-123   the left side's last entry and the right side's first become ONE entry,
//                                                                       the smaller of the two; everything else is appended
//   ContigJuncList::reverse          utils/ContigJuncList.cpp:98-103    the list reversed
// A list enters those through four numbers: its sum, its size, its first and its last entry.  The join of two summaries is the summary of the
// joined lists, and it is associative: an entry of a joined list is the minimum over a contiguous run of the concatenated inputs (the header
// comment above fgpu_stage3_join, include/faucet_gpu.h), whichever way the calls are bracketed, so a fold may run in any grouping that keeps
// the order.  A summary of no entries (n == 0) has no join: the reference reads back() of an empty list there.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FGPU_COV_HD __host__ __device__
#else
#define FGPU_COV_HD
#endif

struct fgpu_cov_summary {
    uint64_t sum;          // of the entries
    uint32_t n;            // entries
    uint8_t first, last;   // entry 0 and entry n - 1 (both 0 for n == 0)
    uint8_t reserved[2];
};
static_assert(sizeof(fgpu_cov_summary) == 16, "the record as api.py lays it out");

// the summary of A.concatenate(B), both with at least one entry
FGPU_COV_HD inline fgpu_cov_summary fgpu_cov_concatenate(const fgpu_cov_summary& a, const fgpu_cov_summary& b) {
    const uint8_t m = a.last < b.first ? a.last : b.first;
    fgpu_cov_summary r;
    r.sum = a.sum + b.sum - a.last - b.first + m;
    r.n = a.n + b.n - 1;
    r.first = a.n == 1 ? m : a.first;
    r.last = b.n == 1 ? m : b.last;
    r.reserved[0] = r.reserved[1] = 0;
    return r;
}

// ... of the list reversed
FGPU_COV_HD inline fgpu_cov_summary fgpu_cov_reverse(const fgpu_cov_summary& a) {
    fgpu_cov_summary r = a;
    r.first = a.last;
    r.last = a.first;
    return r;
}

// getAvgCoverage of a list of at least one entry: a sum of bytes is exact in double, so it is the one division the reference makes
inline double fgpu_cov_average(const fgpu_cov_summary& a) {
    const double sum = (double)a.sum, size = (double)a.n;
    return sum / size;
}
