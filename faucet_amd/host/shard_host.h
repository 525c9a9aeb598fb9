// shard_host.h — the two passes over N GPUs from ONE process: one host thread per device, reads sharded in file order.
//
// The reference is one process on one core: load_two_filters (utils/Bloom.cpp:267-350, called at src/Faucet.cpp:220) and then
// ReadScanner::scanReads (src/ReadScanner.cpp:284-359, called at src/Faucet.cpp:241-245).  BASELINE.json's north_star keeps that command
// line and shards the reads over the GPUs of a node; this header is the host side of it for C++ callers -- the `faucet` command line
// (`-gpus N`, faucet_main.cpp) and the patch a maintainer links into the reference (integration/faucet_binding.cpp) -- over the C ABI only
// (include/faucet_gpu.h: the per-context calls and the fgpu_group_* exchanges; no HIP here).  faucet_amd/sharded.py is the same protocol for
// one PROCESS per GPU over torch.distributed; DESIGN.md section 5 says why each step is exact.
//
//   shard r = the r-th file-order share of the records (text_source.h, record_cuts), read and driven by thread r on device r
//   pass 0   (ShardedRun::estimate, for a caller that does not know -estimated_kmers / -singletons yet) every rank sketches its shard
//            (fgpu_estimate_begin / _batch), the sketches are merged by slices of the planes and counted (fgpu_group_estimate_end)
//   pass 1   fix-up protocol (a shard that stays in HBM, at most 4 hash functions): every rank loads its shard alone
//            (FGPU_LOAD_SHARD_TIMES) -> exclusive prefix-OR of the shards' bloo1 over ranks -> fgpu_load_fixup against that prefix on
//            ranks > 0 -> OR-allreduce of bloo2;  presence protocol (otherwise, and with --mercy): presence bitmap of the shard ->
//            exclusive prefix-OR = the carried-in bloo1 -> ordered load on it -> OR-allreduce of bloo2;  filter slices
//            (FAUCET_SHARD_PROTOCOL=slices, opt-in): every rank packs its own shard's batches and sends the packed blocks to the others, all
//            load the whole stream into their slice of the bit positions -> OR-allreduce of the batches' fail (miss) planes -> commit ->
//            all-gather of both filters by the slices' byte ranges (load_slices below)
//            With ShardOptions::scan_kept the sliced pass also keeps the reads (fgpu_load_slice_keep_reads) and pass 2 scans the kept batches: the
//            input is read ONCE, and may then be a pipe -- the ranks take turns at one reader (text_source.h, TurnSource), pass 2's shards
//            are ranges of the stream's batches (kept_ranges.h), and the read offsets of a batch packed by another rank than its scanner
//            travel between the passes
//   pass 2   rank 0 streams its shard and shows the others its junction table after a quarter of it (the preview their pure stage uses);
//            ranks > 0 run the pure stage of their shard meanwhile (fgpu_scan_prepare), then take the table, the counters and the two
//            pair filters from the rank below, walk, and hand all four on.  The last rank holds the run's junction map and pair filters.
#pragma once
#include <string.h>

#include <sys/stat.h>

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <string>
#include <thread>
#include <vector>

#include "batch_board.h"
#include "faucet_gpu.h"
#include "kept_ranges.h"
#include "text_source.h"

// The sliced pass' entry points are referred to WEAKLY: a library that defines them (libfaucet_gpu.so) resolves them as usual; linked against
// an implementation of the ABI that answers only the read-shard protocols they are null, and FAUCET_SHARD_PROTOCOL=slices is refused.
#pragma weak fgpu_load_slice_begin
#pragma weak fgpu_load_slice_mercy_begin
#pragma weak fgpu_load_slice_pack
#pragma weak fgpu_load_slice_expect
#pragma weak fgpu_load_slice_batch_packed
#pragma weak fgpu_load_slice_plane
#pragma weak fgpu_load_slice_mercy_probe
#pragma weak fgpu_load_slice_mercy_planes
#pragma weak fgpu_load_slice_commit
#pragma weak fgpu_load_slice_end
#pragma weak fgpu_group_allgather
#pragma weak fgpu_scan_resident_base
#pragma weak fgpu_diag_long_pairs_state
// ... those of the sliced pass that keeps its reads and of the scan of kept batches (ShardOptions::scan_kept)
#pragma weak fgpu_load_slice_keep_reads
#pragma weak fgpu_load_slice_packed_reads
#pragma weak fgpu_load_slice_expect_reads
#pragma weak fgpu_load_slice_adopt_reads
#pragma weak fgpu_scan_kept_range
#pragma weak fgpu_scan_batch_kept
#pragma weak fgpu_scan_prepare_kept
// ... and so are those of pass 0 over read shards (ShardedRun::estimate)
#pragma weak fgpu_estimate_begin
#pragma weak fgpu_estimate_batch
#pragma weak fgpu_estimate_kmers
#pragma weak fgpu_group_estimate_end

namespace faucet_host {

struct ShardOptions {
    int n_ranks = 1;
    int transport = FGPU_TRANSPORT_COPY;
    std::vector<int> devices;             // device of every rank (size n_ranks)
    fgpu_params prm;                      // .device is filled in per rank
    bool fastq = false, mercy = false, paired_ends = false, no_cleaning = false;
    uint64_t chunk_bytes = 64u << 20;
    uint64_t short_tai = 0, long_tai = 0; // pair filters (0: none), create_bloom_filter_optimal's sizes (src/Faucet.cpp:266-283)
    int short_hashes = 0, long_hashes = 0;
    bool verbose = false;                 // FGPU_CLI_TIMES: per-rank stage times on stderr
    bool scan_kept = false;               // filter slices only: pass 1 keeps the reads, pass 2 scans them -- the input is read once (a pipe included)
};

// The options of a run of n_ranks read shards: rank r on device r % fgpu_device_count() (fewer devices than shards: they share).  The caller
// has made sure there is a device (the hosts word that failure differently); the pair filters follow with ShardedRun::set_pair_filters.
inline ShardOptions shard_options(int n_ranks, int transport, const fgpu_params& prm, bool fastq, bool mercy, bool paired_ends, bool no_cleaning,
                                  uint64_t chunk_bytes) {
    ShardOptions so;
    so.n_ranks = n_ranks;
    so.transport = transport;
    const int ndev = std::max(fgpu_device_count(), 1);
    for (int r = 0; r < n_ranks; r++) so.devices.push_back(r % ndev);
    so.prm = prm;
    so.fastq = fastq;
    so.mercy = mercy;
    so.paired_ends = paired_ends;
    so.no_cleaning = no_cleaning;
    so.chunk_bytes = chunk_bytes;
    return so;
}

struct ShardLoadResult {
    fgpu_load_stats stats;                // summed over the shards = the sequential run's
    float w1 = 0, w2 = 0;                 // Bloom::weight of the run's bloo1 / bloo2
    bool fixup = false;
    bool slices = false;                  // the pass ran by filter slices (FAUCET_SHARD_PROTOCOL=slices)
    bool reads_kept = false;              // ... and kept the reads: every rank holds the offsets of the batches it scans (ShardedRun::scan, from_kept)
    uint64_t kept_bytes = 0, kept_budget = 0;   // what a rank keeps resident for that (planes of every batch, offsets of its own range), and may
};

struct ShardScanResult {
    fgpu_scan_stats stats;                // the last rank's = the sequential run's
    uint64_t empty_count = 0, not_empty_count = 0;
};

#define RANK_CHECK(call)                                                                                              \
do {                                                                                                              \
    const int rc__ = (call);                                                                                      \
    if (rc__ != FGPU_OK) { err_[(size_t)r] = std::string(#call) + " failed: " + fgpu_last_error(c); return rc__; } \
} while (0)
#define GROUP_CHECK(call)                                                                                             \
do {                                                                                                              \
    const int rc__ = (call);                                                                                      \
    if (rc__ != FGPU_OK) { err_[(size_t)r] = std::string(#call) + " failed: " + fgpu_group_last_error(group_, r); return rc__; } \
} while (0)
#define RANK_TRY(call)                                  \
do {                                                \
    const int rc__ = (call);                        \
    if (rc__ != FGPU_OK) return rc__;               \
} while (0)

class ShardedRun {
public:
    explicit ShardedRun(const ShardOptions& o) : o_(o), ctx_((size_t)o.n_ranks, nullptr), err_((size_t)o.n_ranks), bufs_((size_t)o.n_ranks) { graveyard_.resize((size_t)std::max(o.n_ranks, 1)); }
    ~ShardedRun() { close(); }
    ShardedRun(const ShardedRun&) = delete;
    ShardedRun& operator=(const ShardedRun&) = delete;

    const std::string& error() const { return error_; }
    fgpu_ctx* ctx(int rank) const { return ctx_[(size_t)rank]; }
    fgpu_ctx* first_ctx() const { return ctx_.front(); }
    fgpu_ctx* last_ctx() const { return ctx_.back(); }
    int n_ranks() const { return o_.n_ranks; }
    // the pair filters of the scan (0 bits: none): create_bloom_filter_optimal's sizes, known once the host has made its own (src/Faucet.cpp:266-283)
    void set_pair_filters(uint64_t short_tai, int short_hashes, uint64_t long_tai, int long_hashes) {
        o_.short_tai = short_tai; o_.short_hashes = short_hashes; o_.long_tai = long_tai; o_.long_hashes = long_hashes;
    }

    // contexts (one per rank, made by the rank's thread) and the group that ties them together
    int create() {
        int rc = fgpu_group_create(o_.n_ranks, o_.transport, &group_);
        if (rc != FGPU_OK) {
            error_ = std::string("fgpu_group_create: ") + (group_ ? fgpu_group_last_error(group_, -1) : "bad arguments");
            return rc;
        }
        return run_ranks([this](int r) -> int {
            fgpu_params p = o_.prm;
            p.device = o_.devices[(size_t)r];
            int rc = fgpu_create(&p, &ctx_[(size_t)r]);
            if (rc != FGPU_OK) { err_[(size_t)r] = std::string("fgpu_create: ") + fgpu_last_error(nullptr); return rc; }
            for (int i = 0; i < 2; i++) {
                bufs_[(size_t)r].p[i] = (char*)fgpu_host_alloc(kTextPad + o_.chunk_bytes);
                if (!bufs_[(size_t)r].p[i]) { err_[(size_t)r] = "page-locked text buffers could not be allocated"; return FGPU_ERR_NOMEM; }
            }
            rc = fgpu_group_attach(group_, r, ctx_[(size_t)r]);
            if (rc != FGPU_OK) err_[(size_t)r] = std::string("fgpu_group_attach: ") + fgpu_group_last_error(group_, r);
            return rc;
        });
    }

    void close() {
        if (group_) { fgpu_group_destroy(group_); group_ = nullptr; }
        // exchange buffers of a pass that FAILED: freed only here, behind fgpu_group_destroy, which has synchronised every rank's stream -- a peer's
        // copy may still have been reading them when their rank gave up
        for (size_t r = 0; r < graveyard_.size() && r < ctx_.size(); r++) {
            for (void* p : graveyard_[r]) if (ctx_[r]) fgpu_device_free(ctx_[r], p);
            graveyard_[r].clear();
        }
        for (size_t r = 0; r < ctx_.size(); r++) {
            if (ctx_[r]) { fgpu_destroy(ctx_[r]); ctx_[r] = nullptr; }
            for (int i = 0; i < 2; i++) if (bufs_[r].p[i]) { fgpu_host_free(bufs_[r].p[i]); bufs_[r].p[i] = nullptr; }
        }
    }

    // ---- pass 0 (not in the reference: include/faucet_gpu.h, fgpu_estimate_*): every rank sketches its shard of `path` with 2^r_bits cells per
    // level (0: the library's default) and the ranks merge their sketches; *out is what ONE sketch of the whole file gives, to the last counter.
    // FGPU_ERR_CAPACITY (the sketch is too full: raise r_bits) leaves the counts in *out.  kmers_by_rank (or null): the occurrences per shard.
    static bool estimate_linked() { return fgpu_estimate_begin && fgpu_estimate_batch && fgpu_estimate_kmers && fgpu_group_estimate_end; }
    int estimate(const std::string& path, int r_bits, fgpu_estimate* out, std::vector<uint64_t>* kmers_by_rank = nullptr) {
        if (!estimate_linked()) {
            error_ = "the library this program is linked against lacks the entry points of the estimate pass over read shards "
                     "(fgpu_estimate_begin, fgpu_estimate_batch, fgpu_estimate_kmers, fgpu_group_estimate_end)";
            return FGPU_ERR_STATE;
        }
        std::vector<uint64_t> cuts;
        const double t_cuts = now_ms();
        if (!record_cuts(path, o_.fastq ? 4 : 2, o_.paired_ends ? 2 : 1, o_.n_ranks, &cuts)) {
            error_ = "cannot cut " + path + " into read shards: with several GPUs the input must be a regular file";
            return FGPU_ERR_ARG;
        }
        if (o_.verbose) fprintf(stderr, "[cli]   pass 0: record cuts of %s found in %.1f ms (kept for the passes that follow)\n", path.c_str(), now_ms() - t_cuts);
        std::vector<fgpu_estimate> est((size_t)o_.n_ranks);
        std::vector<uint64_t> kmers((size_t)o_.n_ranks, 0);
        std::vector<int> status((size_t)o_.n_ranks, FGPU_OK);
        int rc = run_ranks([&](int r) -> int {
            fgpu_ctx* c = ctx_[(size_t)r];
            const double t0 = now_ms();
            RANK_CHECK(fgpu_estimate_begin(c, r_bits));
            // (a rank that fails before the collective end aborts the group through run_ranks: the others' end returns, and fgpu_destroy
            // gives this rank's planes back behind fgpu_group_destroy)
            RANK_TRY(for_each_batch(r, path, cuts, [&](const fgpu_reads* b) { return fgpu_estimate_batch(c, b); }, nullptr));
            RANK_CHECK(fgpu_estimate_kmers(c, &kmers[(size_t)r]));
            const double t1 = now_ms();
            memset(&est[(size_t)r], 0, sizeof(fgpu_estimate));
            const int rc_end = fgpu_group_estimate_end(group_, r, &est[(size_t)r]);
            status[(size_t)r] = rc_end;
            if (rc_end != FGPU_OK && rc_end != FGPU_ERR_CAPACITY) { err_[(size_t)r] = std::string("fgpu_group_estimate_end failed: ") + fgpu_group_last_error(group_, r); return rc_end; }
            tell(r, "pass 0: sketch of the shard %.1f ms, merge by slices + count %.1f ms", t1 - t0, now_ms() - t1);
            return FGPU_OK;             // (too full a sketch is every rank's answer, not a rank's failure: the group stays usable)
        });
        if (rc != FGPU_OK) return rc;
        *out = est[0];
        if (kmers_by_rank) *kmers_by_rank = kmers;
        if (status[0] == FGPU_ERR_CAPACITY) error_ = "the sketch is too full even at its thinnest level: raise r_bits";
        return status[0];
    }

    // ---- pass 1 (load_two_filters, utils/Bloom.cpp:267-350): afterwards every rank holds the run's bloo2, the last rank its bloo1
    // the entry points ShardOptions::scan_kept needs beside those of the sliced pass
    static bool scan_kept_linked() {
        return fgpu_load_slice_keep_reads && fgpu_load_slice_packed_reads && fgpu_load_slice_expect_reads && fgpu_load_slice_adopt_reads &&
               fgpu_scan_kept_range && fgpu_scan_batch_kept && fgpu_scan_prepare_kept;
    }
    static bool slices_asked() {
        const char* e = getenv("FAUCET_SHARD_PROTOCOL");
        return e && !strcmp(e, "slices");
    }

    int load(const std::string& path, ShardLoadResult* out) {
        std::vector<uint64_t> cuts;
        struct stat st_in;
        if (o_.scan_kept && slices_asked() && stat(path.c_str(), &st_in) == 0 && !S_ISREG(st_in.st_mode)) {
            // one stream that can be read once: no byte ranges, the ranks take turns at it (load_slices)
            uint64_t b = ~0ULL;
            for (int r = 0; r < o_.n_ranks; r++) {
                uint64_t rb = 0;
                if (fgpu_load_fixup_state(ctx_[(size_t)r], nullptr, &rb) != FGPU_OK) rb = 0;
                b = std::min(b, rb);
            }
            return load_slices(path, cuts, b, out);
        }
        if (!record_cuts(path, o_.fastq ? 4 : 2, o_.paired_ends ? 2 : 1, o_.n_ranks, &cuts)) {
            error_ = "cannot cut " + path + " into read shards: with several GPUs the input must be a regular file";
            return FGPU_ERR_ARG;
        }
        uint64_t largest = 0;
        for (int r = 0; r < o_.n_ranks; r++) largest = std::max(largest, cuts[(size_t)r + 1] - cuts[(size_t)r]);
        // the fix-up protocol keeps the shard's batches in HBM (about a byte per base with the fail planes) within what the library sets aside for
        // resident batches -- asked of every context, not assumed -- and covers four hash functions; --mercy leaves no fix-up state
        uint64_t budget = ~0ULL;
        for (int r = 0; r < o_.n_ranks; r++) {
            uint64_t b = 0;
            if (fgpu_load_fixup_state(ctx_[(size_t)r], nullptr, &b) != FGPU_OK) b = 0;
            budget = std::min(budget, b);
        }
        if (const char* e = getenv("FAUCET_SHARD_PROTOCOL"))
            if (!strcmp(e, "slices")) return load_slices(path, cuts, budget, out);
        sliced_counts_.clear();
        const char* force_planes = getenv("FAUCET_SHARD_PLANES");
        const bool short_shards = largest < 0xFFF00000ULL - (1ULL << 24) && !(force_planes && force_planes[0] == '1' && o_.prm.n_hash <= 4);   // a shard's positions (<= its bytes) fit one 32-bit clock
        bool fixup = !o_.mercy && (short_shards || o_.prm.n_hash <= 4) && largest + (64ULL << 20) < budget;
        if (const char* e = getenv("FAUCET_SHARD_PROTOCOL")) {
            if (!strcmp(e, "presence")) fixup = false;
            else if (!strcmp(e, "fixup") && !fixup) { error_ = "FAUCET_SHARD_PROTOCOL=fixup: a shard is too large to stay in HBM, more than 4 hash functions, or --mercy is on"; return FGPU_ERR_ARG; }
        }
        const char* dbg_not_ready = getenv("FAUCET_DEBUG_FIXUP_NOT_READY");      // tests: this rank's own load "did not stay resident"
        std::vector<fgpu_load_stats> st((size_t)o_.n_ranks);
        float w1 = 0, w2 = 0;
        const uint64_t nbytes = o_.prm.tai / 8;
        std::atomic<bool> fixup_done{fixup};
        int rc = run_ranks([&](int r) -> int {
            fgpu_ctx* c = ctx_[(size_t)r];
            const double t0 = now_ms();
            void *b1 = nullptr, *b2 = nullptr, *prefix = nullptr;
            RANK_CHECK(fgpu_device_alloc(c, nbytes, &prefix));
            Deferred free_prefix(this, r, &prefix, nullptr, nullptr, nullptr);
            bool use_fixup = fixup;
            double t1 = t0;
            if (use_fixup) {
                RANK_CHECK(fgpu_load_begin(c, short_shards ? FGPU_LOAD_SHARD_TIMES : FGPU_LOAD_SHARD_PLANES));
                RANK_TRY(for_each_batch(r, path, cuts, [&](const fgpu_reads* b) { return fgpu_load_batch(c, b); }, nullptr));
                RANK_CHECK(fgpu_load_end(c, &st[(size_t)r]));
                t1 = now_ms();
                // Can every rank complete its pass by the fix-up?  (A batch that did not stay resident -- over the budget, or no memory at that
                // moment -- leaves fgpu_load_fixup nothing to work on.)  The ranks agree: if one cannot, ALL run the presence protocol instead --
                // a pass more, the same filters -- rather than the run dying after a full pass 1.
                int ready = 0;
                RANK_CHECK(fgpu_load_fixup_state(c, &ready, nullptr));
                if (dbg_not_ready && atoi(dbg_not_ready) == r) ready = 0;
                if (!vote(ready != 0)) {
                    if (aborted_) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
                    use_fixup = false;
                    fixup_done = false;
                    tell(r, "pass 1: own load %.1f ms; a rank cannot complete it by the fix-up: the presence protocol instead", t1 - t0);
                }
            }
            if (use_fixup) {
                RANK_CHECK(fgpu_bloom_devptr(c, FGPU_BLOO1, &b1, nullptr));
                GROUP_CHECK(fgpu_group_exclusive_prefix_or(group_, r, b1, prefix, nbytes));
                if (r > 0) RANK_CHECK(fgpu_load_fixup(c, prefix, &st[(size_t)r]));
                tell(r, "pass 1: own load %.1f ms, prefix-OR exchange + fix-up %.1f ms", t1 - t0, now_ms() - t1);
            } else {
                const double t1p = now_ms();
                RANK_CHECK(fgpu_load_begin(c, 0));             // (empties both filters)
                RANK_CHECK(fgpu_load_end(c, nullptr));
                RANK_TRY(for_each_batch(r, path, cuts, [&](const fgpu_reads* b) { return fgpu_presence_batch(c, b); }, nullptr));
                const double t2p = now_ms();
                RANK_CHECK(fgpu_bloom_devptr(c, FGPU_BLOO1, &b1, nullptr));
                GROUP_CHECK(fgpu_group_exclusive_prefix_or(group_, r, b1, prefix, nbytes));
                RANK_CHECK(fgpu_device_copy(c, b1, prefix, nbytes));      // the carried-in bloo1 of this shard
                RANK_CHECK(fgpu_load_begin(c, FGPU_LOAD_KEEP_CARRY));
                RANK_TRY(for_each_batch(r, path, cuts, [&](const fgpu_reads* b) { return fgpu_load_batch(c, b); }, nullptr));
                RANK_CHECK(fgpu_load_end(c, &st[(size_t)r]));
                tell(r, "pass 1: presence pass %.1f ms, prefix-OR exchange + ordered load %.1f ms", t2p - t1p, now_ms() - t2p);
            }
            const double t2 = now_ms();
            RANK_CHECK(fgpu_bloom_devptr(c, FGPU_BLOO2, &b2, nullptr));
            GROUP_CHECK(fgpu_group_or_allreduce(group_, r, b2, nbytes));
            if (r == o_.n_ranks - 1) {
                RANK_CHECK(fgpu_bloom_weight(c, FGPU_BLOO1, &w1));
                RANK_CHECK(fgpu_bloom_weight(c, FGPU_BLOO2, &w2));
            } else {
                RANK_CHECK(fgpu_synchronize(c));
            }
            tell(r, "pass 1: OR-allreduce of bloo2 %.1f ms (to the device's completion)", now_ms() - t2);
            free_prefix.ok = true;
            return FGPU_OK;
        });
        if (rc != FGPU_OK) return rc;
        memset(&out->stats, 0, sizeof(out->stats));
        for (const fgpu_load_stats& s : st) {
            out->stats.reads_processed += s.reads_processed;
            out->stats.unambiguous_reads += s.unambiguous_reads;
            out->stats.kmers += s.kmers;
            out->stats.to_bloo2 += s.to_bloo2;
        }
        out->w1 = w1;
        out->w2 = w2;
        out->fixup = fixup_done;
        return FGPU_OK;
    }

    // ---- pass 1 by FILTER SLICES ("the sliced pass in the C++ host"): rank r owns the filter bits of slice r and loads the
    // WHOLE stream into them.  Each batch is read, split and packed by the owner of its read shard only (fgpu_load_slice_pack) and travels to the
    // other ranks in its packed form, 3 bits per stream position; the board (batch_board.h) tells every rank what to expect from whom, in file
    // order, so that all ranks load the same batches and make the same sequence of collectives.
    int load_slices(const std::string& path, const std::vector<uint64_t>& cuts, uint64_t budget, ShardLoadResult* out) {
        const int n = o_.n_ranks;
        const bool by_turns = cuts.empty();                  // a pipe: no byte ranges, one reader the ranks take turns at
        if (!slices_linked()) {
            error_ = "FAUCET_SHARD_PROTOCOL=slices: the library this program is linked against lacks the entry points of the sliced pass "
                     "(fgpu_load_slice_*, fgpu_group_allgather, fgpu_scan_resident_base)";
            return FGPU_ERR_STATE;
        }
        if (o_.scan_kept && !scan_kept_linked()) {
            error_ = "FAUCET_SHARD_PROTOCOL=slices with kept reads: the library this program is linked against lacks the entry points "
                     "(fgpu_load_slice_keep_reads, fgpu_load_slice_packed_reads, fgpu_load_slice_expect_reads, fgpu_load_slice_adopt_reads, "
                     "fgpu_scan_kept_range, fgpu_scan_batch_kept, fgpu_scan_prepare_kept)";
            return FGPU_ERR_STATE;
        }
        if (const char* e = getenv("FAUCET_DEBUG_SLICES_BUDGET")) budget = strtoull(e, nullptr, 10);      // tests: "the ranks keep this many bytes resident"
        // every rank keeps every batch: 5 bits per stream position (codes, bad, fail, sure), 9 with the four miss planes of --mercy; a stream
        // position per input byte is the upper bound (headers and quality lines only lower it).  (A pipe's size is not known: there the
        // batches are counted as they come, SliceKept::add.)
        if (!by_turns) {
            const uint64_t input = cuts.back(), bits = o_.mercy ? 9 : 5, need = input / 8 * bits + (input % 8 * bits + 7) / 8;
            if (need > budget) {
                error_ = "FAUCET_SHARD_PROTOCOL=slices: every rank keeps the whole input resident in its packed form: " + std::to_string(input) +
                         " bytes of input x " + (o_.mercy ? "9/8 (--mercy)" : "5/8") + " = " + std::to_string(need) + " bytes, the ranks' smallest budget for resident batches is " +
                         std::to_string(budget) + " bytes";
                return FGPU_ERR_NOMEM;
            }
        }
        // slice bounds: tai bits over n ranks in units of 512 bits (64 bytes), the last ones short or empty
        const uint64_t nbytes = o_.prm.tai / 8;
        std::vector<uint64_t> bounds((size_t)n + 1);
        {
            uint64_t step = (nbytes + (uint64_t)n - 1) / (uint64_t)n;
            step = (step + 63) & ~63ULL;
            for (int q = 0; q <= n; q++) bounds[(size_t)q] = std::min<uint64_t>((uint64_t)q * step, nbytes);
        }
        BatchBoard board(n);
        std::unique_ptr<TextSource> stream;
        std::unique_ptr<TurnSource> turns;
        if (by_turns) {
            stream.reset(new TextSource(path, o_.fastq, o_.chunk_bytes, 0, ~0ULL, bufs_[0].p));
            if (!stream->is_open()) { error_ = "cannot open " + path; return FGPU_ERR_ARG; }
            turns.reset(new TurnSource(stream.get(), n));
        }
        SliceShared sh;
        sh.board = &board;
        sh.turns = turns.get();
        sh.budget = budget;
        sh.longest.assign((size_t)n, 0);
        std::vector<fgpu_load_stats> st((size_t)n);
        std::vector<uint64_t> counts((size_t)n, 0);
        float w1 = 0, w2 = 0;
        kept_ready_ = false;
        kept_bounds_.clear();
        int rc = run_ranks([&](int r) -> int {
            const int rc_rank = slice_rank(r, path, cuts, bounds, &sh, &st[(size_t)r], r == 0 ? &counts : nullptr, &w1, &w2);
            if (rc_rank != FGPU_OK) {                        // (ranks that wait for a batch or a turn of this one wake up and fail)
                board.abort();
                if (turns) turns->abort();
            }
            return rc_rank;
        });
        turns.reset();
        stream.reset();
        if (rc != FGPU_OK) return rc;
        sliced_counts_ = counts;
        out->stats = st[0];                                  // the stats of a sliced pass are the whole run's on every rank: one rank's, not a sum
        out->w1 = w1;
        out->w2 = w2;
        out->fixup = false;
        out->slices = true;
        out->reads_kept = kept_ready_;
        out->kept_bytes = kept_bytes_ = sh.kept_bytes;
        out->kept_budget = kept_budget_ = budget;
        if (o_.verbose && o_.scan_kept && by_turns)
            fprintf(stderr, "[cli]   pass 1: the read offsets of %llu of %llu batches changed ranks between the passes\n", (unsigned long long)sh.moved.load(),
                    (unsigned long long)kept_T_.size());
        return FGPU_OK;
    }

private:
    static bool slices_linked() {
        return fgpu_load_slice_begin && fgpu_load_slice_mercy_begin && fgpu_load_slice_pack && fgpu_load_slice_expect && fgpu_load_slice_batch_packed &&
               fgpu_load_slice_plane && fgpu_load_slice_mercy_probe && fgpu_load_slice_mercy_planes && fgpu_load_slice_commit && fgpu_load_slice_end &&
               fgpu_group_allgather && fgpu_scan_resident_base;
    }

    // what the ranks of one sliced pass share beside the board
    struct SliceShared {
        BatchBoard* board = nullptr;
        TurnSource* turns = nullptr;           // a pipe: the one reader (null: every rank reads its own byte range)
        uint64_t budget = 0;                   // bytes a rank may keep resident
        uint64_t kept_bytes = 0;               // (rank 0's count: what a rank keeps, see slice_rank step 5)
        std::vector<uint64_t> longest;         // per rank: the longest read it packed
        std::atomic<uint64_t> moved{0};        // batches whose offsets changed ranks
    };

    // one rank of load_slices
    int slice_rank(int r, const std::string& path, const std::vector<uint64_t>& cuts, const std::vector<uint64_t>& bounds, SliceShared* sh,
                   fgpu_load_stats* stats, std::vector<uint64_t>* counts, float* w1, float* w2) {
        fgpu_ctx* c = ctx_[(size_t)r];
        BatchBoard* board = sh->board;
        const int n = o_.n_ranks;
        const bool by_turns = sh->turns != nullptr;
        const double t0 = now_ms();
        // 1  open the pass on the own slice
        RANK_CHECK(o_.mercy ? fgpu_load_slice_mercy_begin(c, bounds[(size_t)r] * 8, bounds[(size_t)r + 1] * 8)
                            : fgpu_load_slice_begin(c, bounds[(size_t)r] * 8, bounds[(size_t)r + 1] * 8));
        if (o_.scan_kept) RANK_CHECK(fgpu_load_slice_keep_reads(c));
        // 2  publish: pack the own batches, post them, send them.  Nothing here waits for another rank's CONSUMPTION (with one reader a rank
        //    waits for its turn to read, which the ranks before it give up as soon as their chunk is split).  Under --mercy the sends wait
        //    for the batch's turn in step 3: there every batch is followed by collectives, and point-to-point calls pair up per (source,
        //    destination) in the order they are made -- a block sent now would meet the receive of an earlier batch's plane.
        std::vector<fgpu_packed> own;
        auto publish = [&](const fgpu_reads* b) -> int {
            fgpu_packed pk;
            const int rc = fgpu_load_slice_pack(c, b, &pk);
            if (rc != FGPU_OK) return rc;
            own.push_back(pk);
            BoardBatch bb;
            bb.T = pk.T;
            bb.n_reads = pk.n_reads;
            if (!board->post(r, bb)) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
            if (!o_.mercy && pk.block_dev)
                for (int q = 0; q < n; q++)
                    if (q != r) GROUP_CHECK(fgpu_group_send_async(group_, r, q, pk.block_dev, pk.nbytes));
            return FGPU_OK;
        };
        if (by_turns) {
            fgpu_reads b;
            uint64_t g = 0;
            for (int more; (more = sh->turns->next(r, c, &b, &g)) != 0;) {
                if (more == TurnSource::ABORTED) { err_[(size_t)r] = "the run was aborted while this rank waited for its turn at the input"; return FGPU_ERR_STATE; }
                if (more < 0) { err_[(size_t)r] = std::string("fgpu_text_split failed: ") + fgpu_last_error(c); return -more; }
                const int rc = publish(&b);
                if (rc != FGPU_OK) { if (err_[(size_t)r].empty()) err_[(size_t)r] = std::string("a batch call failed: ") + fgpu_last_error(c); return rc; }
                if (aborted_) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
            }
        } else {
            RANK_TRY(for_each_batch(r, path, cuts, publish, nullptr));
        }
        board->close(r);
        const double t1 = now_ms();
        // 3  consume in the stream's order (batch_board.h, StreamCursor); a peer's batch is received into a block of its size
        double t_exchange = 0;
        uint64_t loaded = 0;                                  // non-empty batches so far = the index of the next one's planes
        std::vector<uint64_t> in_shard((size_t)n, 0);
        std::vector<fgpu_packed> blocks;                      // the non-empty batches in the stream's order ...
        std::vector<int> owner_of;                            // ... who packed each ...
        std::vector<uint64_t> Ts, reads_of;                   // ... its stream positions and reads
        uint64_t planes_bytes = 0;
        StreamCursor cursor(board, by_turns);
        for (;;) {
            BoardBatch bb;
            int s = 0;
            uint64_t j = 0;
            const BatchBoard::Wait w = cursor.next(&s, &j, &bb);
            if (w == BatchBoard::ABORTED) { err_[(size_t)r] = "the run was aborted while this rank waited for a batch of shard " + std::to_string(s); return FGPU_ERR_STATE; }
            if (w == BatchBoard::CLOSED) break;
            fgpu_packed pk;
            if (s == r) {
                pk = own[(size_t)j];
                if (o_.mercy && pk.block_dev)
                    for (int q = 0; q < n; q++)
                        if (q != r) GROUP_CHECK(fgpu_group_send_async(group_, r, q, pk.block_dev, pk.nbytes));
            } else {
                RANK_CHECK(fgpu_load_slice_expect(c, bb.T, bb.n_reads, &pk));
                if (pk.block_dev) GROUP_CHECK(fgpu_group_recv(group_, r, s, pk.block_dev, pk.nbytes));
            }
            RANK_CHECK(fgpu_load_slice_batch_packed(c, &pk));
            if (!pk.block_dev) continue;
            if (o_.mercy) {                               // the lockstep of a mercy pass: the batch's fail plane over all ranks, then its probe
                const double tx = now_ms();
                void* plane = nullptr;
                uint64_t pb = 0;
                RANK_CHECK(fgpu_load_slice_plane(c, loaded, &plane, &pb));
                GROUP_CHECK(fgpu_group_or_allreduce(group_, r, plane, pb));
                RANK_CHECK(fgpu_load_slice_mercy_probe(c));
                t_exchange += now_ms() - tx;
            }
            loaded++;
            in_shard[(size_t)s]++;
            if (o_.scan_kept) {
                blocks.push_back(pk);
                owner_of.push_back(s);
                Ts.push_back(bb.T);
                reads_of.push_back(bb.n_reads);
                // a stream of unknown size is counted as it comes: the same sum on every rank, so all of them stop at the same batch
                planes_bytes += (o_.mercy ? 9 : 5) * ((bb.T + 63) / 64 + 8) * 8;
                if (by_turns && planes_bytes > sh->budget) {
                    err_[(size_t)r] = "FAUCET_SHARD_PROTOCOL=slices: the stream does not fit the ranks' budget for resident batches: " + std::to_string(planes_bytes) +
                                      " bytes kept after " + std::to_string(loaded) + " batches, budget " + std::to_string(sh->budget) +
                                      " bytes; a pipe cannot be read again (fewer reads per run, or a file and the read-shard protocols)";
                    return FGPU_ERR_NOMEM;
                }
            }
        }
        if (counts) *counts = in_shard;
        const double t2 = now_ms();
        // 4  the planes over all ranks (the same batches on every rank: the same sequence of collectives), commit, the filters by slices
        for (uint64_t i = 0; i < loaded; i++) {
            void* plane = nullptr;
            uint64_t pb = 0;
            RANK_CHECK(o_.mercy ? fgpu_load_slice_mercy_planes(c, i, &plane, &pb) : fgpu_load_slice_plane(c, i, &plane, &pb));
            GROUP_CHECK(fgpu_group_or_allreduce(group_, r, plane, pb));
        }
        const double t3 = now_ms();
        RANK_CHECK(fgpu_load_slice_commit(c));
        RANK_CHECK(fgpu_load_slice_end(c, stats));
        const double t4 = now_ms();
        for (int which = FGPU_BLOO1; which <= FGPU_BLOO2; which++) {
            void* bits = nullptr;
            uint64_t nb = 0;
            RANK_CHECK(fgpu_bloom_devptr(c, which, &bits, &nb));
            GROUP_CHECK(fgpu_group_allgather(group_, r, bits, nb, bounds.data()));
        }
        GROUP_CHECK(fgpu_group_flush(group_, r));
        if (r == n - 1) {
            RANK_CHECK(fgpu_bloom_weight(c, FGPU_BLOO1, w1));
            RANK_CHECK(fgpu_bloom_weight(c, FGPU_BLOO2, w2));
        } else {
            RANK_CHECK(fgpu_synchronize(c));
        }
        const double t5 = now_ms();
        tell(r, "pass 1 (filter slices): pack + publish %.1f ms, load %.1f ms, exchange of the planes %.1f ms, commit %.1f ms, gather of the filters %.1f ms",
             t1 - t0, t2 - t1 - t_exchange, t_exchange + (t3 - t2), t4 - t3, t5 - t4);
        if (!o_.scan_kept) return FGPU_OK;
        // 5  pass 2's shards over the kept batches.  A file: rank r scans the batches it packed -- no offsets move.  A pipe: contiguous ranges of
        //    the stream's batches balanced by stream positions (kept_ranges.h), and every batch whose owner is not its scanner has its offsets
        //    sent from owner to scanner, point to point, in ascending g per (source, destination) pair.  The same arithmetic on every rank.
        std::vector<uint64_t> range((size_t)n + 1, 0);
        if (by_turns) {
            range = kept_scan_ranges(Ts, reads_of, n, o_.paired_ends ? 2 : 1);
        } else {
            for (int q = 0; q < n; q++) range[(size_t)q + 1] = range[(size_t)q] + in_shard[(size_t)q];
        }
        std::vector<int> scanner_of(blocks.size(), 0);
        for (int q = 0; q < n; q++)
            for (uint64_t g = range[(size_t)q]; g < range[(size_t)q + 1]; g++) scanner_of[(size_t)g] = q;
        // the longest read this rank packed (the library knows it since the pass has ended): every rank needs the pass-wide one
        for (size_t g = 0; g < blocks.size(); g++)
            if (owner_of[g] == r) {
                fgpu_kept_reads mine;
                RANK_CHECK(fgpu_load_slice_packed_reads(c, &blocks[g], &mine));
                sh->longest[(size_t)r] = mine.max_read_len;
                break;
            }
        if (!vote(true)) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }      // the barrier between the passes
        uint64_t longest = 0;
        for (uint64_t l : sh->longest) longest = std::max(longest, l);
        uint64_t offs_bytes = 0, moved_in = 0;
        for (size_t g = 0; g < blocks.size(); g++)
            if (owner_of[g] == r && scanner_of[g] != r) {
                fgpu_kept_reads mine;
                RANK_CHECK(fgpu_load_slice_packed_reads(c, &blocks[g], &mine));
                GROUP_CHECK(fgpu_group_send_async(group_, r, scanner_of[g], mine.offsets_dev, (mine.n_reads + 1) * 8));
            }
        for (size_t g = 0; g < blocks.size(); g++) {
            if (scanner_of[g] != r) continue;
            offs_bytes += (reads_of[g] + 1) * 8;
            if (owner_of[g] == r) continue;
            fgpu_kept_reads theirs;
            RANK_CHECK(fgpu_load_slice_expect_reads(c, &blocks[g], &theirs));
            GROUP_CHECK(fgpu_group_recv(group_, r, owner_of[g], theirs.offsets_dev, (theirs.n_reads + 1) * 8));
            theirs.max_read_len = longest;
            RANK_CHECK(fgpu_load_slice_adopt_reads(c, &blocks[g], &theirs));      // (checked on the device against the block: reported below)
            moved_in++;
        }
        GROUP_CHECK(fgpu_group_flush(group_, r));
        int complete = 0;
        RANK_CHECK(fgpu_scan_kept_range(c, range[(size_t)r], range[(size_t)r + 1], longest, &complete));
        // what this rank keeps resident against what it may (tests lower the budget: FAUCET_DEBUG_SLICES_BUDGET)
        uint64_t may = sh->budget;
        if (const char* e = getenv("FAUCET_DEBUG_SCAN_KEPT_BUDGET")) may = std::min<uint64_t>(may, strtoull(e, nullptr, 10));      // (the one-device run's knob)
        const bool fits = planes_bytes + offs_bytes <= may;
        sh->moved += moved_in;
        if (r == 0) sh->kept_bytes = planes_bytes + offs_bytes;
        const bool all = vote(complete != 0 && fits);
        if (aborted_) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
        if (r == 0) {
            kept_ready_ = all;
            kept_bounds_ = range;
            kept_T_ = Ts;
        }
        tell(r, "pass 1 (filter slices): reads kept for batches %llu to %llu of %llu, the offsets of %llu of them from other ranks, %.1f ms%s",
             (unsigned long long)range[(size_t)r], (unsigned long long)range[(size_t)r + 1], (unsigned long long)blocks.size(), (unsigned long long)moved_in, now_ms() - t5,
             all ? "" : ": NOT every rank holds its range");
        return FGPU_OK;
    }

public:

    // ---- pass 2 (ReadScanner::scanReads, src/ReadScanner.cpp:284-359): afterwards the last rank holds the junction map and the pair filters
    // from_kept (after a sliced pass 1 that kept the reads, ShardLoadResult::reads_kept): no input is opened; rank r scans the kept batches of its
    // range -- fgpu_scan_batch_kept on the first rank, fgpu_scan_prepare_kept on the ranks above -- and the progress that times the two
    // previews is counted in stream positions instead of bytes.  The hand-over of tables, counters, hints and pair filters is the same.
    bool reads_kept() const { return kept_ready_; }
    uint64_t kept_bytes() const { return kept_bytes_; }      // what a rank keeps resident for it, and what it may
    uint64_t kept_budget() const { return kept_budget_; }
    int scan(const std::string& path, ShardScanResult* out, bool from_kept = false) {
        std::vector<uint64_t> cuts;
        if (from_kept && !(kept_ready_ && kept_bounds_.size() == (size_t)o_.n_ranks + 1 && scan_kept_linked())) {
            error_ = "the scan of kept reads needs a sliced pass 1 that kept them on every rank";
            return FGPU_ERR_STATE;
        }
        if (!from_kept && !record_cuts(path, o_.fastq ? 4 : 2, o_.paired_ends ? 2 : 1, o_.n_ranks, &cuts)) {
            error_ = "cannot cut " + path + " into read shards: with several GPUs the input must be a regular file";
            return FGPU_ERR_ARG;
        }
        const int n = o_.n_ranks;
        // the batches of rank r, in the stream's order, each handed to `each`; after(units of the shard handed out so far) runs behind each:
        // bytes of text, or -- kept batches -- stream positions
        auto shard_total = [&](int r) -> uint64_t {
            if (!from_kept) return cuts[(size_t)r + 1] - cuts[(size_t)r];
            uint64_t t = 0;
            for (uint64_t g = kept_bounds_[(size_t)r]; g < kept_bounds_[(size_t)r + 1]; g++) t += kept_T_[(size_t)g];
            return t;
        };
        auto each_batch = [&](int r, const std::function<int(const fgpu_reads*, uint64_t)>& each, const std::function<int(uint64_t)>& after) -> int {
            if (!from_kept) return for_each_batch(r, path, cuts, [&](const fgpu_reads* b) { return each(b, 0); }, after);
            uint64_t done = 0;
            for (uint64_t g = kept_bounds_[(size_t)r]; g < kept_bounds_[(size_t)r + 1]; g++) {
                const int rc = each(nullptr, g);
                if (rc != FGPU_OK) { if (err_[(size_t)r].empty()) err_[(size_t)r] = std::string("a kept batch call failed: ") + fgpu_last_error(ctx_[(size_t)r]); return rc; }
                done += kept_T_[(size_t)g];
                if (after) { const int rc2 = after(done); if (rc2 != FGPU_OK) return rc2; }
                if (aborted_) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
            }
            return FGPU_OK;
        };
        const bool short_pairs = !o_.no_cleaning && o_.short_tai, long_filter = o_.paired_ends && !o_.no_cleaning && o_.long_tai;
        hint_ = Announce();
        chain_.assign((size_t)n, Announce());
        late_.assign((size_t)n, Announce());
        const char* late_env = getenv("FAUCET_LATE_HINT");
        const bool late_hints = !(late_env && late_env[0] == '0');
        std::vector<uint64_t> empty((size_t)n, 0), not_empty((size_t)n, 0);
        fgpu_scan_stats last_stats;
        memset(&last_stats, 0, sizeof(last_stats));
        int rc = run_ranks([&](int r) -> int {
            fgpu_ctx* c = ctx_[(size_t)r];
            const double t0 = now_ms();
            if (short_pairs) RANK_CHECK(fgpu_scan_short_pairs(c, o_.short_tai, o_.short_hashes, 0));
            if (o_.paired_ends)
                RANK_CHECK(long_filter ? fgpu_scan_long_pairs(c, o_.long_tai, o_.long_hashes, FGPU_LONG_PAIRS_FILTER) : fgpu_scan_long_pairs(c, 0, 0, FGPU_LONG_PAIRS_COUNT));
            if (long_filter) {      // (a note on stderr, once per run, when the first-set times are kept per batch: include/faucet_gpu.h)
                uint64_t form[4] = {0, 0, 0, 0};
                if (fgpu_diag_long_pairs_state && fgpu_diag_long_pairs_state(c, form) == FGPU_OK && form[0] == 2 && !sparse_said_.exchange(true))
                    fprintf(stderr, "note: the long pair filter (%llu bits) keeps its first-set times per batch (sparse state)\n", (unsigned long long)o_.long_tai);
            }
            if (!sliced_counts_.empty() && !from_kept) {
                // after a sliced pass 1 this rank holds the batches of the whole stream: its own shard's begin behind those of the shards below
                uint64_t below = 0;
                for (int q = 0; q < r; q++) below += sliced_counts_[(size_t)q];
                RANK_CHECK(fgpu_scan_resident_base(c, below));
            }
            RANK_CHECK(fgpu_scan_begin(c));
            fgpu_scan_stats st;
            memset(&st, 0, sizeof(st));
            void *hint_buf = nullptr, *table_in = nullptr, *table_out = nullptr, *late_buf = nullptr;
            Deferred free_all(this, r, &hint_buf, &table_in, &table_out, &late_buf);
            if (r == 0) {
                // the first shard has nothing to wait for: it streams (pure stage of batch b + 1 beside the walk of batch b, lazy junction tests).
                // Once a quarter of it is walked the others are shown its table -- an earlier state of the very table they will be handed, which is
                // all the preview of their pure stage needs (fgpu_scan_import_hint); the hint never enters a result.
                bool shown = n == 1;
                const uint64_t quarter = shard_total(0) / 4;
                // Round 6: the rank above this one has nobody to pass it a table, so it is shown a second, later state of this one (after 7/10 of the
                // shard): its planes and candidate planes are made against a table a few million keys short of the one it is handed, and its
                // hop is the short one of every later rank (fgpu_scan_refresh_prepared).  Sent without waiting: the scan goes on beside the copy.
                bool shown_late = n == 1 || !late_hints;
                const uint64_t late_at = shard_total(0) / 10 * 7;
                // (both previews: show_table -- asynchronous sends, announced once they are queued)
                auto show = [&]() -> int { shown = true; return show_table(&hint_buf, 1, n, &hint_); };
                auto show_late = [&]() -> int { shown_late = true; return show_table(&late_buf, 1, 2, &late_[1]); };
                RANK_TRY(each_batch(r, [&](const fgpu_reads* b, uint64_t g) { return b ? fgpu_scan_batch(c, b) : fgpu_scan_batch_kept(c, g, nullptr); },
                                        [&](uint64_t bytes_done) -> int {
                                            if (!shown && bytes_done >= quarter) { const int src = show(); if (src != FGPU_OK) return src; }
                                            if (shown && !shown_late && bytes_done >= late_at) return show_late();
                                            return FGPU_OK;
                                        }));
                if (!shown) RANK_TRY(show());                 // (a shard without batches still owes the others their preview)
                if (!shown_late) RANK_TRY(show_late());
                RANK_CHECK(fgpu_scan_end(c, &st));
                tell(r, "%s: first shard streamed in %.1f ms; valid_reused %llu", from_kept ? "pass 2 (scan of kept reads)" : "pass 2", now_ms() - t0,
                     (unsigned long long)st.valid_reused);
            } else {
                // pure stage while the lower shards walk.  It does not wait for the preview: batches prepared before it arrives see an empty table
                // (every junction test evaluated), the others the preview.
                bool have_hint = false;
                auto take_hint = [&](bool wait, bool use) -> int {
                    uint64_t n_entries = 0;
                    if (!announced(&hint_, wait, &n_entries, nullptr)) return aborted_ ? FGPU_ERR_STATE : FGPU_OK;
                    RANK_TRY(receive_table(r, 0, n_entries, &hint_buf));
                    if (use) RANK_CHECK(fgpu_scan_import_hint(c, hint_buf, n_entries));
                    have_hint = true;
                    return FGPU_OK;
                };
                RANK_TRY(each_batch(r, [&](const fgpu_reads* b, uint64_t g) -> int {
                    if (!have_hint) { const int rc = take_hint(false, true); if (rc != FGPU_OK) return rc; }
                    return b ? fgpu_scan_prepare(c, b) : fgpu_scan_prepare_kept(c, g, nullptr);
                }, nullptr));
                if (!have_hint) RANK_TRY(take_hint(true, false));   // the send is received even when it came too late to be of use
                if (late_hints && r >= 1) {
                    // the table the rank below has just been HANDED, passed on at once: a preview one shard older than the table this rank will get
                    // (the rank above the first one: the first rank's own table after 7/10 of its shard).
                    // The planes of the prepared batches are made again against it while the rank below walks; the walk then only looks for the
                    // keys that rank created (fgpu_scan_refresh_prepared, faucet_gpu.h)
                    uint64_t n_late = 0;
                    if (!announced(&late_[(size_t)r], true, &n_late, nullptr)) { err_[(size_t)r] = "the run was aborted while this rank waited for the fresher preview"; return FGPU_ERR_STATE; }
                    RANK_TRY(receive_table(r, r - 1, n_late, &late_buf));
                    RANK_CHECK(fgpu_scan_import_hint(c, late_buf, n_late));
                    RANK_CHECK(fgpu_scan_refresh_prepared(c));
                }
                const double t1 = now_ms();
                uint64_t n_in = 0;
                fgpu_scan_stats carried;
                if (!announced(&chain_[(size_t)r], true, &n_in, &carried)) { err_[(size_t)r] = "the run was aborted while this rank waited for the junction table"; return FGPU_ERR_STATE; }
                RANK_TRY(receive_table(r, r - 1, n_in, &table_in));
                if (late_hints && r + 1 < n) {                       // pass it on before walking on it: the copy runs beside the walk
                    GROUP_CHECK(fgpu_group_send_async(group_, r, r + 1, table_in, n_in * FGPU_TABLE_ENTRY_BYTES));
                    announce(&late_[(size_t)r + 1], n_in, nullptr);
                }
                RANK_TRY(move_pair_filters(r, short_pairs, long_filter, false));
                const double t2 = now_ms();
                RANK_CHECK(fgpu_scan_import_table(c, table_in, n_in, &carried));   // (takes the place of the preview)
                RANK_CHECK(fgpu_scan_walk_prepared(c));
                RANK_CHECK(fgpu_scan_end(c, &st));
                tell(r, "%s: pure stage %.1f ms, waited %.1f ms for the table, import + walk %.1f ms; valid_reused %llu",
                     from_kept ? "pass 2 (scan of kept reads)" : "pass 2", t1 - t0, t2 - t1, now_ms() - t2, (unsigned long long)st.valid_reused);
            }
            if (o_.paired_ends) RANK_CHECK(fgpu_scan_long_pairs_download(c, nullptr, 0, &empty[(size_t)r], &not_empty[(size_t)r]));
            if (r < n - 1) {
                uint64_t got = 0;
                RANK_TRY(export_table(r, &table_out, &got));
                announce(&chain_[(size_t)r + 1], got, &st);
                GROUP_CHECK(fgpu_group_send(group_, r, r + 1, table_out, got * FGPU_TABLE_ENTRY_BYTES));
                RANK_TRY(move_pair_filters(r, short_pairs, long_filter, true));
            } else {
                last_stats = st;
            }
            if (n > 1 && (r == 0 || (late_hints && r + 1 < n))) GROUP_CHECK(fgpu_group_flush(group_, r));      // (asynchronous sends: the previews)
            RANK_CHECK(fgpu_synchronize(c));
            free_all.ok = true;
            return FGPU_OK;
        });
        if (rc != FGPU_OK) return rc;
        out->stats = last_stats;
        out->empty_count = out->not_empty_count = 0;
        for (int r = 0; r < n; r++) { out->empty_count += empty[(size_t)r]; out->not_empty_count += not_empty[(size_t)r]; }
        return FGPU_OK;
    }

private:
    struct Bufs { char* p[2] = {nullptr, nullptr}; };
    // device buffers of one rank's pass: freed at once when the pass ended well (everything that touched them has been waited for), else left to close()
    struct Deferred {
        ShardedRun* run;
        int r;
        void** p[4];
        bool ok;
        Deferred(ShardedRun* run_, int r_, void** a, void** b, void** c, void** d) : run(run_), r(r_), ok(false) { p[0] = a; p[1] = b; p[2] = c; p[3] = d; }
        Deferred(const Deferred&) = delete;
        ~Deferred() {
            for (void** q : p) {
                if (!q || !*q) continue;
                if (ok) fgpu_device_free(run->ctx_[(size_t)r], *q);
                else { std::lock_guard<std::mutex> g(run->m_); run->graveyard_[(size_t)r].push_back(*q); }
            }
        }
    };
    // every rank arrives with its answer; true iff all said yes (false as well when the run has been aborted meanwhile)
    bool vote(bool mine) {
        std::unique_lock<std::mutex> g(m_);
        const uint64_t gen = vote_gen_;
        vote_all_ = vote_all_ && mine;
        if (++vote_count_ == o_.n_ranks) {
            vote_result_ = vote_all_;
            vote_count_ = 0;
            vote_all_ = true;
            vote_gen_++;
            cv_.notify_all();
            return vote_result_;
        }
        cv_.wait(g, [&] { return vote_gen_ != gen || aborted_; });
        return vote_gen_ != gen ? vote_result_ : false;
    }
    // what one rank tells another through host memory (the ranks share a process): a count, the scan's counters.  The bytes themselves
    // travel device to device (fgpu_group_send / _recv).
    struct Announce {
        bool ready = false;
        uint64_t n = 0;
        fgpu_scan_stats stats;
        Announce() { memset(&stats, 0, sizeof(stats)); }
    };

    static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

    template <class... A>
    void tell(int r, const char* fmt, A... a) const {
        if (!o_.verbose) return;
        char b[320];
        snprintf(b, sizeof(b), fmt, a...);
        fprintf(stderr, "[cli] rank %d %s\n", r, b);
    }

    void announce(Announce* a, uint64_t n, const fgpu_scan_stats* st) {
        {
            std::lock_guard<std::mutex> g(m_);
            a->n = n;
            if (st) a->stats = *st;
            a->ready = true;
        }
        cv_.notify_all();
    }
    bool announced(Announce* a, bool wait, uint64_t* n, fgpu_scan_stats* st) {
        std::unique_lock<std::mutex> g(m_);
        if (wait) cv_.wait(g, [&] { return a->ready || aborted_; });
        if (!a->ready) return false;
        *n = a->n;
        if (st) *st = a->stats;
        return true;
    }

    // the rank's junction table as it stands, exported into a buffer of its size: *buf (freed by the caller's Deferred), *got entries
    int export_table(int r, void** buf, uint64_t* got) {
        fgpu_ctx* c = ctx_[(size_t)r];
        uint64_t n_entries = 0;
        RANK_CHECK(fgpu_scan_table_entries(c, &n_entries));
        const uint64_t bytes = std::max<uint64_t>(n_entries, 1) * FGPU_TABLE_ENTRY_BYTES;
        RANK_CHECK(fgpu_device_alloc(c, bytes, buf));
        RANK_CHECK(fgpu_scan_export_table(c, *buf, bytes, got));
        return FGPU_OK;
    }
    // ... and a table of n_entries that rank `from` has announced, received into a buffer of its size
    int receive_table(int r, int from, uint64_t n_entries, void** buf) {
        fgpu_ctx* c = ctx_[(size_t)r];
        RANK_CHECK(fgpu_device_alloc(c, std::max<uint64_t>(n_entries, 1) * FGPU_TABLE_ENTRY_BYTES, buf));
        GROUP_CHECK(fgpu_group_recv(group_, r, from, *buf, n_entries * FGPU_TABLE_ENTRY_BYTES));
        return FGPU_OK;
    }
    // the first rank shows ranks [to, to_end) its table as it stands -- sent without waiting: its scan goes on beside the copies -- and raises `a`
    int show_table(void** buf, int to, int to_end, Announce* a) {
        const int r = 0;
        uint64_t got = 0;
        RANK_TRY(export_table(r, buf, &got));
        for (int q = to; q < to_end; q++) GROUP_CHECK(fgpu_group_send_async(group_, r, q, *buf, got * FGPU_TABLE_ENTRY_BYTES));
        announce(a, got, nullptr);
        return FGPU_OK;
    }

    // the two pair filters travel with the junction table: what rank r ends with is what rank r + 1 starts from (adds only; check-then-insert
    // in file order; the shards begin at even records, so no first end is left waiting across a cut)
    int move_pair_filters(int r, bool short_pairs, bool long_filter, bool send) {
        fgpu_ctx* c = ctx_[(size_t)r];
        for (int which = 0; which < 2; which++) {
            if (which == 0 ? !short_pairs : !long_filter) continue;
            void* p = nullptr;
            uint64_t nb = 0;
            RANK_CHECK(fgpu_scan_pairs_devptr(c, which, &p, &nb));
            if (send) GROUP_CHECK(fgpu_group_send(group_, r, r + 1, p, nb));
            else GROUP_CHECK(fgpu_group_recv(group_, r, r - 1, p, nb));
        }
        return FGPU_OK;
    }

    // the batches of rank r's shard, in file order; after(bytes of the shard handed out so far) runs behind each
    int for_each_batch(int r, const std::string& path, const std::vector<uint64_t>& cuts, const std::function<int(const fgpu_reads*)>& each,
                       const std::function<int(uint64_t)>& after) {
        fgpu_ctx* c = ctx_[(size_t)r];
        TextSource src(path, o_.fastq, o_.chunk_bytes, cuts[(size_t)r], cuts[(size_t)r + 1], bufs_[(size_t)r].p);
        if (!src.is_open()) { err_[(size_t)r] = "cannot open " + path; return FGPU_ERR_ARG; }
        fgpu_reads b;
        for (int more; (more = src.next(c, &b)) != 0;) {
            if (more < 0) { err_[(size_t)r] = std::string("fgpu_text_split failed: ") + fgpu_last_error(c); return -more; }
            const int rc = each(&b);
            if (rc != FGPU_OK) { if (err_[(size_t)r].empty()) err_[(size_t)r] = std::string("a batch call failed: ") + fgpu_last_error(c); return rc; }
            if (after) { const int rc2 = after(src.bytes_handed_out()); if (rc2 != FGPU_OK) return rc2; }
            if (aborted_) { err_[(size_t)r] = "the run was aborted (another rank failed)"; return FGPU_ERR_STATE; }
        }
        return FGPU_OK;
    }

    // one thread per rank; the first failure aborts the group (every thread that waits for another wakes up and fails) and is reported
    int run_ranks(const std::function<int(int)>& body) {
        std::vector<int> rcs((size_t)o_.n_ranks, FGPU_OK);
        std::vector<std::thread> th;
        for (int r = 0; r < o_.n_ranks; r++)
            th.emplace_back([&, r] {
                rcs[(size_t)r] = body(r);
                if (rcs[(size_t)r] != FGPU_OK) {
                    {
                        std::lock_guard<std::mutex> g(m_);
                        aborted_ = true;
                    }
                    cv_.notify_all();
                    if (group_) fgpu_group_abort(group_);
                }
            });
        for (std::thread& t : th) t.join();
        // the rank that failed first by its own doing (not by the abort) is the one to report
        int rc = FGPU_OK;
        for (int pass = 0; pass < 2 && rc == FGPU_OK; pass++)
            for (int r = 0; r < o_.n_ranks; r++) {
                if (rcs[(size_t)r] == FGPU_OK) continue;
                const bool by_abort = err_[(size_t)r].find("abort") != std::string::npos;
                if (pass == 0 && by_abort) continue;
                rc = rcs[(size_t)r];
                error_ = "rank " + std::to_string(r) + ": " + err_[(size_t)r];
                break;
            }
        return rc;
    }

#undef RANK_CHECK
#undef GROUP_CHECK
#undef RANK_TRY

    ShardOptions o_;
    fgpu_group* group_ = nullptr;
    std::vector<fgpu_ctx*> ctx_;
    std::vector<std::string> err_;
    std::vector<Bufs> bufs_;
    std::string error_;
    std::mutex m_;
    std::condition_variable cv_;
    std::atomic<bool> aborted_{false};
    std::atomic<bool> sparse_said_{false};     // the note about the long pair filter's sparse state is out
    Announce hint_;
    std::vector<Announce> chain_;
    std::vector<Announce> late_;      // the table a rank was handed, passed on to the rank above as a fresher preview
    std::vector<std::vector<void*>> graveyard_{64};
    // after a sliced pass 1 that kept the reads: every rank holds the offsets of its range; the ranges of pass 2 over the stream's non-empty
    // batches (n + 1 bounds), and the batches' stream positions
    bool kept_ready_ = false;
    uint64_t kept_bytes_ = 0, kept_budget_ = 0;
    std::vector<uint64_t> kept_bounds_, kept_T_;
    std::vector<uint64_t> sliced_counts_;   // after a sliced pass 1: non-empty batches per read shard (pass 2 finds its own among the resident ones)
    int vote_count_ = 0;
    bool vote_all_ = true, vote_result_ = false;
    uint64_t vote_gen_ = 0;
};

}  // namespace faucet_host
