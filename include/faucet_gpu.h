/*
 * faucet_gpu.h — C ABI of libfaucet_gpu.so: Faucet's two-pass k-mer pipeline on MI355X (gfx950).
 *
 * The reference (Shamir-Lab/Faucet) has no plugin / FFI layer; this ABI cuts the two seams that
 * SURVEY.md §8(b) names and is what a maintainer's `faucet` binary (or any other host language)
 * binds.  Every entry point cites the reference interface it replaces.
 *
 *   pass 1   void load_two_filters(Bloom*, Bloom*, std::string, bool fastq, bool mercy)
 *            utils/Bloom.h:294, utils/Bloom.cpp:267, caller src/Faucet.cpp:220
 *   pass 2   void ReadScanner::scanReads(bool fastq, bool paired_ends, bool no_cleaning)
 *            src/ReadScanner.cpp:284, constructed and called at src/Faucet.cpp:241-245
 *   sizing   getBloomFilterFromReads / create_bloom_filter_optimal / _2_hash / Bloom::Bloom
 *            src/Faucet.cpp:197-219, utils/Bloom.cpp:165-247
 *
 * Conventions: extern "C", opaque context, POD structs, caller-owned buffers with explicit sizes,
 * int status (0 = ok), no exceptions / STL / torch types across the boundary.  One host thread
 * drives one context; one context drives one HIP device.  Results are bit-identical to the
 * reference CPU path (same Bloom bit array, same junction records).  There is no CPU fallback:
 * every compute entry point returns FGPU_ERR_HIP when no gfx950 device is usable.
 */
#ifndef FAUCET_GPU_H
#define FAUCET_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGPU_ABI_VERSION 3

enum {
    FGPU_OK = 0,
    FGPU_ERR_ARG = 1,       /* bad parameter (k out of 1..31, tai not a power of two, ...) */
    FGPU_ERR_HIP = 2,       /* HIP runtime error or no device; see fgpu_last_error() */
    FGPU_ERR_STATE = 3,     /* call out of sequence (e.g. load_batch before load_begin) */
    FGPU_ERR_CAPACITY = 4,  /* batch larger than max_batch_bases, junction table full, ... */
    FGPU_ERR_NOMEM = 5,
    FGPU_ERR_INTERNAL = 6   /* a bound that holds by construction did not (fgpu_stage3_build's round guard) */
};

enum { FGPU_BLOO1 = 0, FGPU_BLOO2 = 1 };

typedef struct fgpu_ctx fgpu_ctx;

typedef struct {
    int32_t  k;                 /* -size_kmer (src/Faucet.cpp:66), 1..31 */
    int32_t  j;                 /* -j, default 1 (src/Faucet.h:15) */
    int32_t  max_spacer_dist;   /* -max_spacer_dist, default 100 (src/Faucet.h:48) */
    int32_t  n_hash;            /* hash functions of both load filters (utils/Bloom.cpp:243-244) */
    uint64_t tai;               /* bits per load filter, power of two (utils/Bloom.cpp:173-175) */
    int32_t  device;            /* HIP device ordinal */
    int32_t  flags;             /* FGPU_FLAG_* */
    uint64_t junction_capacity; /* INITIAL slots of the device junction table, power of two; 0 = default (tai / 32).  The table is
                                 * rehashed into a larger one between batches whenever it is more than a quarter full (the
                                 * reference's unordered_map grows the same way, utils/JunctionMap.h:61).  A single batch that outgrows
                                 * it is absorbed by the library while the scan's batches are in its journal (see fgpu_scan_set_eager:
                                 * the journal is scanned again on a table four times the size; fgpu_diag_scan_replays counts it); only a
                                 * scan without a journal -- FGPU_FLAG_EAGER_FLAGS, fgpu_scan_set_eager(1), or beyond the journal's
                                 * budget of an eighth of the device memory -- ends with FGPU_ERR_CAPACITY there.  Either way no list
                                 * of a walk that overflowed reaches fgpu_scan_take_stops or a pair filter: the replay comes first, or
                                 * the call that would have handed them out returns FGPU_ERR_CAPACITY. */
    uint64_t max_batch_bases;   /* largest batch (bases + one separator per read); 0 = default 2^30 */
    void*    stream;            /* hipStream_t to run on, or NULL for a private stream */
    uint64_t walk_window_span;  /* stream positions per scheduling window of the ordered walk; 0 = adaptive.
                                 * Any value gives the same results (tests use small ones to force clusters). */
} fgpu_params;

#define FGPU_FLAG_PROFILE 1     /* bracket every kernel with HIP events (fgpu_kernel_times) */
#define FGPU_FLAG_MERCY 16       /* load_two_filters(..., mercy = true): also add low-coverage k-mers between solid ones to bloo2
                                 * (utils/Bloom.cpp:300-333; the reference's --mercy) */
#define FGPU_FLAG_RECORD_STOPS 8 /* keep scanInputRead's return value for every read (fgpu_scan_take_stops) */
#define FGPU_FLAG_NO_RESIDENT 4 /* do not keep the load batches in HBM for the scan pass (see fgpu_load_batch) */
#define FGPU_FLAG_KEY_ORDER_FROM_START 32 /* large clusters are walked in the order of their junction k-mers' turns from a scan's first window on,
                                 * not only once the scan has shown such a cluster, and "large" means 32 pieces instead of 64 (DESIGN.md
                                 * section 4): four small launches more per window; same results.  For callers that expect repeats at
                                 * high coverage. */
#define FGPU_FLAG_EAGER_FLAGS 2 /* evaluate testForJunction at every position instead of only where the walk can stop
                                 * skipping (same results; the lazy default checks itself and repairs what it finds, see fgpu_scan_set_eager) */

/* A batch of sequence lines in file order: read i = bases[offsets[i] .. offsets[i+1]).  Any byte
 * may occur; everything except upper-case A C G T splits a read exactly as isValidNuc /
 * getUnambiguousReads do (utils/Kmer.cpp:50-80).  offsets[0] need not be 0.
 * on_device != 0: all pointers are device (HBM) pointers on params.device.
 * starts != NULL (device batches only): the reads are not contiguous in `bases` -- read i is
 * bases[starts[i] .. starts[i] + offsets[i+1] - offsets[i]) (sequence lines inside raw FASTA/FASTQ text,
 * see fgpu_text_split); offsets still carries the lengths as differences.
 * total_bases (device batches only; host batches: ignored): offsets[n_reads] - offsets[0] if the caller knows it, else 0.  With 0 the library
 * reads the two offsets back from the device, which makes every call wait for everything it has queued before -- the kernels of the batch
 * before -- before it can queue this batch's: a caller that streams device batches should fill it in (round 4, config 2: the host spent 9 ms of a
 * 64 ms scan in that wait).  A value that does not match the offsets is an error the pass reports at its next synchronising call (FGPU_ERR_ARG). */
typedef struct {
    const char*     bases;
    const uint64_t* offsets;    /* n_reads + 1 entries */
    uint64_t        n_reads;
    int32_t         on_device;
    uint32_t        total_bases;
    const uint64_t* starts;     /* n_reads entries, or NULL */
} fgpu_reads;

typedef struct {
    uint64_t reads_processed;    /* "Reads processed"   utils/Bloom.cpp:335,346 */
    uint64_t unambiguous_reads;  /* "Unambiguous reads" utils/Bloom.cpp:287,347 */
    uint64_t kmers;              /* iterations of the loop at utils/Bloom.cpp:289 — the unit N */
    uint64_t to_bloo2;           /* occurrences routed to bloo2 (utils/Bloom.cpp:293) */
} fgpu_load_stats;

typedef struct {
    uint64_t reads_processed;    /* src/ReadScanner.cpp:348 */
    uint64_t unambiguous_reads;  /* :269 */
    uint64_t reads_no_errors;    /* :276 */
    uint64_t nb_jcheck_kmer;     /* :49  */
    uint64_t nb_no_juncs;        /* :196 */
    uint64_t nb_processed;       /* :83,:192 */
    uint64_t nb_skipped;         /* :192 */
    uint64_t n_junctions;        /* JunctionMap::getNumJunctions, utils/JunctionMap.cpp:598-600 */
    uint64_t kmers;              /* windows inside unambiguous segments (same unit N as pass 1) */
    /* diagnostics of the ordered walk (not in the reference) */
    uint64_t walk_windows;       /* scheduling windows executed */
    uint64_t walk_followers;     /* pieces that had to wait for an earlier piece of their cluster */
    uint64_t walk_max_cluster;   /* largest dependency cluster seen */
    uint64_t flag_positions;     /* window positions at which testForJunction was evaluated (lazy flags: a subset of all) */
    uint64_t piece_positions;    /* window positions inside valid pieces */
    uint64_t valid_reused;       /* getValidReads answers taken from the load pass' resident planes (no filter probe) */
    uint64_t flags_filled;       /* windows whose testForJunction the walk evaluated itself because the preview had left them out */
    uint64_t walk_parallel;      /* pieces of large clusters walked apart from their cluster's thread: in the order of their junction k-mers'
                                  * turns (k_walk_ko, the default for clusters of 64 pieces and more) or all at once, round after round until
                                  * their logs settle (k_ovw_round / k_ovw_commit, the optimistic walk) */
} fgpu_scan_stats;

/* One element of the list ReadScanner::scanInputRead returns for a read (src/ReadScanner.cpp:260-282): the real-extension
 * k-mer pushed at a junction visit of scan_forward (:140) or add_fake_junction's extension (:197,:103), with what the
 * callers of that list need to know about the visit (:147-169, :208-225).  Needs FGPU_FLAG_RECORD_STOPS. */
typedef struct {
    uint64_t ext;    /* ReadKmer::getRealExtension() at the visit */
    uint32_t read;   /* index of the read within its batch */
    uint32_t info;   /* bits 0-27 ReadKmer::pos inside the valid piece; FGPU_STOP_* bits */
} fgpu_stop;
#define FGPU_STOP_POS_MASK 0x0FFFFFFFu
#define FGPU_STOP_FORWARD  (1u << 28)   /* facing FORWARD (else BACKWARD) */
#define FGPU_STOP_FIRST    (1u << 29)   /* first element of its valid piece (= of one scan_forward call) */
#define FGPU_STOP_FAKE     (1u << 30)   /* the piece had no junction: this is add_fake_junction's element */

/* Junction record, field for field utils/Junction.h:10-18 (cov is private there). */
typedef struct {
    uint8_t cov[4];
    uint8_t dist[5];
    uint8_t linked[5];
} fgpu_junction;

/* ---- library / context ------------------------------------------------------------------- */
int         fgpu_abi_version(void);
/* Number of usable gfx950 devices (0 when there is none; never fails). */
int         fgpu_device_count(void);
int         fgpu_create(const fgpu_params* params, fgpu_ctx** out);
void        fgpu_destroy(fgpu_ctx* ctx);
const char* fgpu_last_error(const fgpu_ctx* ctx);   /* ctx may be NULL: last fgpu_create failure */
int         fgpu_synchronize(fgpu_ctx* ctx);

/* ---- filter sizing (host arithmetic only; replaces src/Faucet.cpp:197-219, Bloom.cpp:165-247) --- */
/* p1 such that two filters at rate p1 give overall rate fp; <0 when the root is not bracketed
 * (e.g. singletons == 0) — callers must treat that as an argument error. */
double   fgpu_solve_p1(uint64_t estimated_kmers, uint64_t singletons, float fp, int32_t* iterations);
uint64_t fgpu_bloom_tai(uint64_t requested_bits);                                  /* Bloom.cpp:173-178 */
void     fgpu_size_optimal(uint64_t estimated, float fp, int32_t* bits_per_item, uint64_t* tai, int32_t* n_hash);
void     fgpu_size_two_hash(uint64_t estimated, float fp, int32_t* bits_per_item, uint64_t* tai, int32_t* n_hash);

/* ---- pass 0: the two numbers the sizing above starts from, counted on the device ------------------------
 * Every run needs -estimated_kmers (F0: distinct canonical k-mers of the read set) and -singletons (f1: those seen exactly once); the reference
 * sizes its filters from nothing else (src/Faucet.cpp:197-219) and leaves it to a separate k-mer counter to find them.  This pass sketches the
 * reads instead.  Every valid window -- the occurrences of the loop at utils/Bloom.cpp:289, fgpu_load_stats.kmers of them -- is hashed once with
 * a 64-bit bijection, h; it falls into level min(clz64(h) / FGPU_EST_SHIFT, FGPU_EST_LEVELS - 1) (clz64(0) = 64) and there into cell
 * h & (m - 1) of m = 2^r_bits: levels >= l together hold a 16^-l sample of the k-mer space.  A cell knows whether it was hit at least once and
 * whether at least twice (by the same or by different k-mers): 2 bits x 4 levels x m cells = 2^r_bits bytes of device memory between _begin
 * and _end (r_bits 8..34; the default, 30, is 1 GiB).  What comes back per level: empty[l], the cells never hit, and once[l], the cells hit
 * exactly once -- functions of the multiset of occurrences alone, whatever the batching.
 * The solve (host arithmetic in doubles): level l is usable iff 8 * empty[l] >= m (a load of at most ln 8); level = the smallest l such that
 * levels l..3 are all usable; with n distinct keys thrown into m cells a cell stays empty with probability e^-(n/m) and holds exactly one
 * occurrence with probability (n/m) e^-(n/m) x (the singletons' share), hence
 *     f0 = 16^level * sum over l >= level of m * ln(m / empty[l])          f1 = 16^level * sum over l >= level of m * once[l] / empty[l]
 * At level 0 nothing is sampled: only the collision correction is left.  Level 3 not usable: FGPU_ERR_CAPACITY ("raise r_bits"), level = -1.
 * The pass reads k, the device and max_batch_bases of the context, never tai or n_hash: a caller that does not know its sizes yet creates a
 * context with tai = 128, n_hash = 1 for it, and destroys that context before it makes the real one (two contexts would hold their working
 * buffers side by side). */
#define FGPU_EST_LEVELS 4
#define FGPU_EST_SHIFT 4
#define FGPU_EST_MIN_BITS 8
#define FGPU_EST_MAX_BITS 34
#define FGPU_EST_DEFAULT_BITS 30
typedef struct {
    uint64_t empty[FGPU_EST_LEVELS];   /* cells of the level that no occurrence hit */
    uint64_t once[FGPU_EST_LEVELS];    /* cells of the level that exactly one occurrence hit */
    uint64_t kmers;                    /* occurrences sketched: fgpu_load_stats.kmers of a load of the same reads */
    int32_t  r_bits;                   /* m = 2^r_bits cells per level */
    int32_t  level;                    /* the level the estimates start from; -1: none */
    double   f0, f1;
} fgpu_estimate;
/* r_bits = 0: the default.  A pass of its own: FGPU_ERR_STATE inside a load or scan pass (and their _begin inside this one); FGPU_ERR_ARG for
 * other r_bits; FGPU_ERR_NOMEM when the planes cannot be had. */
int fgpu_estimate_begin(fgpu_ctx* ctx, int32_t r_bits);
/* One batch, in any order: host, device and fgpu_text_split batches alike (packed as fgpu_load_batch packs them). */
int fgpu_estimate_batch(fgpu_ctx* ctx, const fgpu_reads* reads);
/* Counts, solves, frees the planes and ends the pass whatever it returns; out may be NULL.  FGPU_ERR_CAPACITY leaves the counts filled in. */
int fgpu_estimate_end(fgpu_ctx* ctx, fgpu_estimate* out);
/* Host only, no device: level, f0, f1 from empty / once / r_bits.  FGPU_ERR_ARG: r_bits outside 8..34, or counts no sketch of m cells gives
 * (empty[l] + once[l] > m). */
int fgpu_estimate_solve(fgpu_estimate* e);
/* The sketches of the shards of a read set merge into the sketch of all of it.  A cell is a counter that saturates at 2 -- `seen` alone: 1,
 * `seen` and `twice`: 2 or more -- and merging is saturating addition, cell by cell; on the 32-bit words of the planes (16 cells: `seen` in
 * the low half, `twice` in the high half at the same place)
 *     out = a | b | ((a & b & 0xFFFF) << 16)
 * which is associative and commutative: whatever the order, the merged planes are those one pass over all reads ends with, to the last bit.
 * The planes are 2^r_bits bytes, level l in bytes [l * 2^(r_bits - 2), (l + 1) * 2^(r_bits - 2)), cell c of a level in bit c & 15 (`seen`) and
 * 16 + (c & 15) (`twice`) of its word c >> 4.
 * _planes: the device pointer and size of the open pass' planes, as fgpu_bloom_devptr gives the filters'; nbytes may be NULL.
 * _merge: peer_dev holds bytes [first_byte, first_byte + nbytes) of another sketch with the same r_bits (on this context's device); they are
 * merged into the same bytes of this context's planes, on the context's stream, behind whatever it has queued.  first_byte, nbytes and
 * peer_dev are multiples of 16; nbytes = 0 does nothing.  FGPU_ERR_ARG: a null or misaligned pointer, a misaligned range, a range past the planes.
 * _download: the planes to the host (nbytes = 2^r_bits), behind everything queued; waits.  For tests and diagnosis.
 * _kmers: the occurrences the open pass has sketched so far (fgpu_estimate.kmers of this context alone: a rank's share under
 * fgpu_group_estimate_end, which returns the sum); waits for what is queued.
 * All four: FGPU_ERR_STATE outside estimate_begin / estimate_end. */
int fgpu_estimate_planes(fgpu_ctx* ctx, void** dev, uint64_t* nbytes);
int fgpu_estimate_merge(fgpu_ctx* ctx, const void* peer_dev, uint64_t first_byte, uint64_t nbytes);
int fgpu_estimate_download(fgpu_ctx* ctx, void* host, uint64_t nbytes);
int fgpu_estimate_kmers(fgpu_ctx* ctx, uint64_t* kmers);

/* ---- pass 1: Bloom load (replaces load_two_filters, utils/Bloom.cpp:267-350) ------------------- */
/* Zero both filters (or keep bloo1's current content as the carried-in state when keep_carry != 0:
 * multi-GPU shards start from the prefix-OR of the lower ranks' k-mer presence bitmaps). */
int fgpu_load_begin(fgpu_ctx* ctx, int keep_carry);
#define FGPU_LOAD_KEEP_CARRY   1   /* bloo1's current content is the carried-in state */
#define FGPU_LOAD_SHARD_TIMES  2   /* the pass of a read shard that fgpu_load_fixup will complete, for shards of fewer than 2^32 - 16 stream positions
                                    * (FGPU_ERR_CAPACITY beyond): first-set times count from the start of the pass, not of an epoch, and the fix-up
                                    * compares them.  Costs the pass nothing. */
#define FGPU_LOAD_SHARD_PLANES 4   /* the same for shards of ANY size (round 5): while it resolves its occurrences the pass writes down which of an
                                    * occurrence's bits were NOT set before it within the shard (n_hash <= 4 planes of one bit per position, kept in HBM
                                    * with the batch), and the fix-up asks the lower shards' bits for exactly those.  The resolve kernel then looks at every
                                    * missing bit instead of stopping at the first that fails (+10 % on the pass). */
#define FGPU_LOAD_KEEP_READS   8   /* the plain pass (with or without FGPU_LOAD_KEEP_CARRY; FGPU_ERR_STATE together with the two shard flags) keeps, beside
                                    * every resident batch's codes, bad and sure planes, what a scan of the batch needs without its text: the
                                    * (n_reads + 1) read offsets, charged to the resident budget, the read count, and the longest read of the pass.
                                    * fgpu_scan_batch_kept then scans the batches with no second reading of the input.  Filters, stats and sure
                                    * planes are bit for bit those of a pass without the flag; a batch that does not fit ends the keeping as always. */
/* Consume one batch, in file order.  Exact: occurrence t goes to bloo2 iff all its bits were set
 * by occurrences < t, t following the reference's processing order. */
int fgpu_load_batch(fgpu_ctx* ctx, const fgpu_reads* reads);
int fgpu_load_end(fgpu_ctx* ctx, fgpu_load_stats* stats);
/* OR the bits of every k-mer of the batch into bloo1 with no ordering (presence bitmap; used by
 * multi-GPU shards before the prefix-OR exchange).  Same unit counters as load_batch. */
int fgpu_presence_batch(fgpu_ctx* ctx, const fgpu_reads* reads);
/* Read shards without the presence pass.  After a load pass of THIS shard alone (begun with FGPU_LOAD_SHARD_TIMES, or with
 * FGPU_LOAD_SHARD_PLANES and at most 4 hash functions; an empty carry, all batches kept resident, no --mercy) and the exchange of the shards' bloo1, `prefix_dev` = OR of the bloo1
 * of all lower shards (device pointer, tai/8 bytes) is what the sequential run has in bloo1 when it reaches this shard.  Every occurrence the local
 * pass kept out of bloo2 is looked at again: it goes to bloo2 iff each of its bits is in the prefix or was set locally before it (by the pass's
 * times, or by the planes it wrote down).  Adds
 * those occurrences to bloo2, to the planes the scan reuses and to stats->to_bloo2; bloo1 |= prefix.  FGPU_ERR_STATE when the pass was not
 * begun that way or a batch was not kept. */
int fgpu_load_fixup(fgpu_ctx* ctx, const void* prefix_dev, fgpu_load_stats* stats);
/* What a host needs to CHOOSE between the two protocols of pass 1 and to fall back from one to the other (shard_host.h had a
 * constant of its own and no way back).  *ready (may be NULL): 1 iff fgpu_load_fixup can complete the load pass that has just ended -- 0 when
 * a batch was not kept resident (budget, or no memory at that moment), the pass was not begun as a shard's, or --mercy: the ranks then
 * agree to run the presence protocol instead (every rank the same).  *resident_budget_bytes (may be NULL): device bytes this context keeps
 * load batches resident in; a shard's batches need about one byte per base (codes, bad, sure, and up to four fail planes). */
int fgpu_load_fixup_state(fgpu_ctx* ctx, int* ready, uint64_t* resident_budget_bytes);

/* ---- pass 1 by FILTER SLICES: every rank loads the WHOLE stream into its slice of the bit positions ----------------
 * The transposed partition of the multi-GPU pass: instead of a shard of the reads and all of the filter, a rank sees every batch (the same
 * batches, in file order, on every rank) and owns the filter bits [bit_lo, bit_hi) -- both multiples of 512, bit_hi <= tai, any number of
 * slices, an empty one included.  Exact because "bit b was first set at time t" is a property of bit b alone: the owner finds it from the
 * stream, and occurrence t goes to bloo2 iff NO rank reports "one of my bits of occurrence t was not set before t".  That report is one bit
 * per stream position per rank, the FAIL PLANE of a batch; the caller ORs the planes of all ranks in place (fgpu_bitmap_or, or any transport),
 * then fgpu_load_slice_commit sets the own bloo2 bits of the occurrences nobody failed.  No presence pass, no prefix-OR, no fix-up.
 *
 *     fgpu_load_slice_begin(lo, hi);  fgpu_load_slice_batch(b) ...;               every rank, the same batches
 *     for every batch i: fgpu_load_slice_plane(i, &p, &n);  p := OR over ranks     the exchange (caller)
 *     fgpu_load_slice_commit();  fgpu_load_slice_end(&stats);
 *
 * Working state: 4.25 bytes per OWN bit (first-set times + the interleaved {carry, bloo2} pair), always the pair layout
 * (FGPU_LOAD_LAYOUT=records is not used here).  Every batch stays resident in HBM (packed codes, bad mask, fail plane, later the `sure`
 * plane): 5 bits per stream position; a batch that cannot be kept -- FGPU_FLAG_NO_RESIDENT, or beyond the budget
 * (fgpu_load_fixup_state) -- makes fgpu_load_slice_batch return FGPU_ERR_NOMEM.  Stream-ordered on the context's stream like the rest.
 * FGPU_ERR_STATE: _begin while a pass is open or with FGPU_FLAG_MERCY (the mercy rule needs time-aware tests of other slices' bits: the
 * five-step protocol below, opened by fgpu_load_slice_mercy_begin);
 * _batch / _plane / _commit / _end outside a sliced pass; _batch after _commit; _commit twice; _end before _commit; fgpu_load_batch inside
 * a sliced pass; fgpu_load_fixup after one.  FGPU_ERR_ARG: bounds that are not multiples of 512, bit_lo > bit_hi, bit_hi > tai, a batch index
 * out of range. */
int fgpu_load_slice_begin(fgpu_ctx* ctx, uint64_t bit_lo, uint64_t bit_hi);
/* mark + resolve of one batch against the slice; the batch and its fail plane stay in HBM */
int fgpu_load_slice_batch(fgpu_ctx* ctx, const fgpu_reads* reads);
/* The fail plane of the i-th NON-EMPTY batch of the pass: one bit per stream position of the batch's packed stream (64 positions per word, LSB =
 * lowest position), *nbytes padded with zero words to a multiple of 16 (fgpu_bitmap_or's granule).  The layout follows from the batch alone:
 * identical batches give identical layouts on every rank, which is what makes the OR across ranks meaningful.  To be ORed IN PLACE.  Does not
 * synchronise: the plane is complete in stream order behind the fgpu_load_slice_batch that made it. */
int fgpu_load_slice_plane(fgpu_ctx* ctx, uint64_t batch, void** fail_dev, uint64_t* nbytes);
/* After the planes hold the OR over all ranks: the own bloo2 bits of every occurrence whose fail bit is 0, the batches' `sure` planes
 * (= valid & ~fail, the global routing decision: a scan of the same reads in this context reuses them as after a plain load). */
int fgpu_load_slice_commit(fgpu_ctx* ctx);
/* bloo1 / bloo2 of the context (fgpu_bloom_devptr, tai/8 bytes) then hold the own slice and are ZERO outside it: the all-gather is a copy of the
 * byte ranges [bit_lo/8, bit_hi/8) or a plain fgpu_bitmap_or.  stats: reads_processed, unambiguous_reads, kmers as a plain load of the whole
 * stream; to_bloo2 = the GLOBAL count, the same on every rank. */
int fgpu_load_slice_end(fgpu_ctx* ctx, fgpu_load_stats* stats);
/* *ready (may be NULL): 1 inside a sliced pass that has not been committed yet.  *working_bytes (may be NULL): device bytes allocated for the
 * slice state (first-set times + pair).  *n_batches (may be NULL): planes fgpu_load_slice_plane can hand out (0 outside a sliced pass). */
int fgpu_load_slice_state(fgpu_ctx* ctx, int* ready, uint64_t* working_bytes, uint64_t* n_batches);

/* ---- the sliced pass under --mercy: FIVE steps, a lockstep per batch -----------------------------------------------------------------------
 * load_two_filters(..., mercy = true) asks bloo1, as it stood at occurrence t, about the four extensions of a k-mer (isJunction), and their
 * bits lie in any slice.  "Bit b was set by time t" concerns b alone, so its owner answers it from the carry and its first-set times; a
 * candidate is contained iff NO rank finds an own bit of it unset.  Each rank therefore writes four MISS PLANES per batch -- bit (position, nt):
 * an own bit of candidate nt at this position was not set by then -- for a superset of the positions the reference tests (every window but
 * the first of its segment that is not contained, or is contained behind one that is not; known from the ORed fail plane alone), the caller
 * ORs them across the ranks like the fail planes, and the commit runs the reference's per-segment state machine on the ORed answers, setting
 * the own bloo2 bits of every accepted run.  The first-set times answer "<= t" only until the batch joins the carry, so the probe of a batch
 * comes after the exchange of ITS fail plane and before the next batch:
 *
 *     fgpu_load_slice_mercy_begin(lo, hi);
 *     for every batch b, every rank:   fgpu_load_slice_batch(b);                                               1  mark + resolve, no fold
 *                                      fgpu_load_slice_plane(i, &p, &n);  p := OR over ranks                    2  the exchange (caller)
 *                                      fgpu_load_slice_mercy_probe();                                          3  miss planes, then the fold
 *     for every batch i:               fgpu_load_slice_mercy_planes(i, &m, &n);  m := OR over ranks              4  the exchange (caller)
 *     fgpu_load_slice_commit();  fgpu_load_slice_end(&stats);                                                  5
 *
 * bloo1, bloo2, `sure` and the stats come out as the plain --mercy pass leaves them (to_bloo2 = contained occurrences).  Resident state: 9 bits
 * per stream position instead of 5.  FGPU_ERR_STATE: _mercy_begin on a context without FGPU_FLAG_MERCY or while a pass is open; _batch or
 * _commit while the latest batch has not been probed; _mercy_probe / _mercy_planes outside a mercy pass; _mercy_planes of the batch whose
 * probe is owed.  FGPU_ERR_ARG as fgpu_load_slice_begin / fgpu_load_slice_plane. */
int fgpu_load_slice_mercy_begin(fgpu_ctx* ctx, uint64_t bit_lo, uint64_t bit_hi);
/* The latest batch: reads its fail plane (ORed in place, ordered before this call), writes its four miss planes, then folds the batch into the
 * carry.  Nothing owed (an empty batch, or called twice): FGPU_OK, nothing done. */
int fgpu_load_slice_mercy_probe(fgpu_ctx* ctx);
/* The four miss planes of the i-th non-empty batch as ONE block, to be ORed in place: plane nt starts at nt * *nbytes / 4, each has the fail
 * plane's layout and is zero past its last word; *nbytes is a multiple of 16. */
int fgpu_load_slice_mercy_planes(fgpu_ctx* ctx, uint64_t batch, void** miss_dev, uint64_t* nbytes);
/* Counts of the last finished mercy pass (zero after a plain sliced pass): [0] positions THIS rank probed; then, from the commit and the same on
 * every rank: [1] high->low tests answered "junction", [2] runs opened, [3] low->high tests answered "junction", [4] runs added to bloo2,
 * [5] k-mers of those runs. */
int fgpu_diag_slice_mercy(fgpu_ctx* ctx, uint64_t out[6]);

/* ---- the sliced pass from PACKED batches: made once, moved device to device, loaded from the packed form ------------------------------------
 * Under filter slices every rank needs every batch, but only one rank should read, split and pack it.  A packed block is ONE contiguous
 * device buffer: the codes plane (2 bits per stream position, 2 x (n_words + 8) 64-bit words), the bad plane (1 bit per position, n_words + 8
 * words), n_words = ceil(T / 64), and a 16-byte trailer {digest, T} -- nbytes is a function of T alone, so a peer that knows T can receive it.
 *
 *     owner of the batch:   fgpu_load_slice_pack(reads, &p);           send p.block_dev, p.nbytes to the peers (fgpu_group_send_async, ...)
 *     every other rank:     fgpu_load_slice_expect(T, n_reads, &p);    fill p.block_dev (fgpu_group_recv, fgpu_device_copy, ...)
 *     every rank, in the stream's file order:   fgpu_load_slice_batch_packed(&p);   = fgpu_load_slice_batch of the same reads
 *
 * All three only inside a sliced pass (plain or mercy) before its commit, stream-ordered on the context's stream, none waits for the device;
 * they may be mixed with fgpu_load_slice_batch.  The block becomes the resident batch's codes / bad -- no second copy: 5 (9 under --mercy)
 * bits per position as before --, is counted against the resident budget when it is MADE, and stays the pass' until the next sliced pass begins.
 * The digest is an order-independent 64-bit sum over the block's words; _batch_packed recomputes it for a block from _expect and compares it
 * and T with the trailer that travelled with the block: in a protocol that pairs sends and receives by order, a block in the wrong slot would
 * otherwise be a silently wrong filter.  A mismatch is reported as FGPU_ERR_ARG by the pass' next synchronising call (fgpu_load_slice_end at
 * the latest), as a wrong fgpu_reads.total_bases is.
 * FGPU_ERR_STATE: outside a sliced pass or after its commit; _batch_packed of a block that is not of this pass' _pack / _expect, or has been
 * loaded already, or while a mercy pass owes its latest batch the probe.  FGPU_ERR_ARG: null arguments; _expect with n_reads > T, T > 0 without
 * reads or T beyond max_batch_bases; a description whose T / nbytes / n_reads are not the block's.  FGPU_ERR_NOMEM: the batch does not fit the
 * resident budget (fgpu_load_fixup_state; the message names the numbers) or the device has no memory for it.
 *
 * THE FORMAT (restated in plain Python by tests/pack_ref.py, which the tests hold the packing kernels to byte for byte).  Words are 64 bits,
 * little-endian; W = n_words + 8.
 *   stream     Read i starts at position S_i = (bytes of the reads before it) + i and is followed by ONE separator position; T = bytes + reads.
 *   tokens     A read is cut into its maximal runs of good bytes -- upper-case A C G T, nothing else -- and of other bytes.  The runs are laid
 *              out in REVERSE run order, the bytes inside a run in their own order: ascending stream position is the order in which the
 *              reference works through a read's pieces (getUnambiguousReads hands them out last first).
 *   codes      words 0 .. 2W-1.  Position p: word p / 32, bits 62 - 2 * (p % 32) and the one above (the first position of a word in its two most
 *              significant bits).  A good byte c has code (c >> 1) & 3 (A0 C1 T2 G3); every other position, the tail and the padding have 0.
 *   bad plane  words 2W .. 3W-1.  Position p: bit p % 64 of word p / 64.  1 for separators, for bytes that are not good, for every position
 *              from T to the end of word n_words - 1, and for all 64 bits of the 8 padding words.
 *   trailer    word 3W: the digest = sum mod 2^64 over i = 0 .. 3W-1 of mix(word[i] ^ ((i + 1) * 0x9E3779B97F4A7C15)), with mix the finaliser of
 *              splitmix64: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.  Word 3W+1: T. */
typedef struct {
    void*    block_dev;   /* the block on the context's device; NULL for a batch without reads (nbytes = T = 0) */
    uint64_t nbytes;      /* 24 * (ceil(T / 64) + 8) + 16 */
    uint64_t T;           /* stream positions: bases + one separator per read */
    uint64_t n_reads;
} fgpu_packed;
/* Packs now, loads later: k_pack / k_pack_fix straight into a block of the pass, its digest and T into the trailer.  T has to be known without
 * asking the device for the call not to wait: batches from fgpu_text_split, or with total_bases (host batches: always). */
int fgpu_load_slice_pack(fgpu_ctx* ctx, const fgpu_reads* reads, fgpu_packed* out);
/* An empty block of the same layout for a batch that is packed elsewhere; the caller fills all of its nbytes before it is loaded. */
int fgpu_load_slice_expect(fgpu_ctx* ctx, uint64_t T, uint64_t n_reads, fgpu_packed* out);
/* mark + resolve of that batch against the slice, exactly as fgpu_load_slice_batch behind its packing: segment count, epochs, fail plane, a
 * mercy pass' "probe owed"; the batch is the pass' next one (fgpu_load_slice_plane counts it), reads_processed grows by n_reads. */
int fgpu_load_slice_batch_packed(fgpu_ctx* ctx, const fgpu_packed* b);

/* ---- pass 0 keeps what it packs, the plain pass loads from it: one reading of the stream serves both -----------------------------------------
 * Pass 0 reads, splits and packs the whole stream only to sketch it, and pass 1 then does all of that again -- which a stream that can be
 * read once (a pipe) does not allow at all.  A pass that KEEPS packs every non-empty batch straight into a packed block of its own -- the
 * layout, padding, trailer and digest of fgpu_load_slice_pack, 3 bits per stream position -- and sketches it there: no second copy.  The
 * blocks are plain device allocations that belong to whoever holds them: the pass, then the caller that takes them, then the context that
 * loads them.  They outlive the context that made them, so the placeholder context of pass 0 (tai = 128) can be destroyed before the run's
 * context is made:
 *
 *     fgpu_estimate_begin(c0, r_bits);  fgpu_estimate_keep(c0, budget);  fgpu_estimate_batch(c0, b) ...;  fgpu_estimate_end(c0, &e);
 *     fgpu_estimate_take_kept(c0, blocks, cap, &n);  fgpu_destroy(c0);
 *     fgpu_create(sized from e, &c1);  fgpu_load_begin(c1, 0);  fgpu_load_batch_packed(c1, &blocks[i]) ...;  fgpu_load_end(c1, &stats);
 *
 * _keep: between fgpu_estimate_begin and the pass' first batch (FGPU_ERR_STATE otherwise).  A block is charged to budget_bytes as 4 bits per
 * position, 4 * (ceil(T / 64) + 8) * 8 bytes: what a plain load keeps of a batch (codes, bad, sure), so that whatever pass 0 keeps a context
 * with the same budget (fgpu_load_fixup_state) can keep resident.  A batch that does not fit the budget, or for which the device has no
 * memory, does not fail the pass: every block kept so far is released, the pass stops keeping and goes on sketching as one without _keep.
 * The sketch is the same to the last counter either way.
 * _keep_state: *keeping = 1 while every non-empty batch so far is held; *n_blocks, *bytes: the blocks held and what they are charged.  All
 * three may be NULL.  Host state: does not wait for the device.  Valid inside the pass and after its end, until the blocks are taken.
 * _take_kept: after fgpu_estimate_end (whether FGPU_OK or FGPU_ERR_CAPACITY; FGPU_ERR_STATE inside a pass): the blocks in batch order, one per
 * non-empty batch, with T, n_reads and nbytes.  Ownership passes to the caller: fgpu_load_batch_packed hands a block on, fgpu_device_free of
 * any context on the same device releases it.  *n_out (may be NULL) = the number of blocks, also when cap is too small (FGPU_ERR_ARG, nothing
 * taken).  FGPU_ERR_NOMEM, with a message naming the numbers, if the pass stopped keeping.  Blocks that are never taken are released by the
 * next fgpu_estimate_begin or by fgpu_destroy, with the stream waited for first. */
int fgpu_estimate_keep(fgpu_ctx* ctx, uint64_t budget_bytes);
int fgpu_estimate_keep_state(fgpu_ctx* ctx, int* keeping, uint64_t* n_blocks, uint64_t* bytes);
int fgpu_estimate_take_kept(fgpu_ctx* ctx, fgpu_packed* out, uint64_t cap, uint64_t* n_out);
/* One batch of the PLAIN pass from a packed block: fgpu_load_batch of the same reads behind its packing -- segment count, epochs, both
 * layouts, --mercy, the carry -- with reads_processed growing by n_reads and unambiguous_reads, kmers, to_bloo2 as for those reads.  In a
 * pass opened by fgpu_load_begin(ctx, 0) or with FGPU_LOAD_KEEP_CARRY; may be mixed with fgpu_load_batch.  On FGPU_OK the context ADOPTS the
 * block (on an error the caller still owns it): it becomes the resident batch's codes / bad, with only the `sure` plane allocated beside it,
 * until the next load pass begins or the context is destroyed.  Beyond the resident budget, or with FGPU_FLAG_NO_RESIDENT, the batch is
 * loaded all the same, the pass stops keeping batches as after an fgpu_load_batch that did not fit, and the block is released no later than
 * fgpu_load_end.  The block's digest and T are recomputed and compared with its trailer as for a block from fgpu_load_slice_expect: a mismatch
 * is FGPU_ERR_ARG at the pass' next synchronising call, fgpu_load_end at the latest.  A description with a NULL block must be all zeros and
 * does nothing.  FGPU_ERR_STATE: outside a plain pass (a sliced pass included), or in the pass of a read shard (FGPU_LOAD_SHARD_TIMES /
 * FGPU_LOAD_SHARD_PLANES).  FGPU_ERR_ARG: null arguments; nbytes != 24 * (ceil(T / 64) + 8) + 16, T beyond max_batch_bases, n_reads > T or
 * no reads. */
int fgpu_load_batch_packed(fgpu_ctx* ctx, const fgpu_packed* b);

/* ---- pass 0's blocks carry their reads: the offsets a scan of a block needs (fgpu_scan_batch_kept) ------------------------------------------
 * A packed block holds the stream, not where its reads begin (a separator and an N are both a bad position), and its format is fixed.  A
 * keeping pass 0 can keep every batch's (n_reads + 1) read offsets beside its block, as a plain device allocation of its own:
 *
 *     fgpu_estimate_keep(c0, budget);  fgpu_estimate_keep_reads(c0);  fgpu_estimate_batch(c0, b) ...;  fgpu_estimate_end(c0, &e);
 *     fgpu_estimate_take_kept(c0, blocks, cap, &n);  fgpu_estimate_take_kept_reads(c0, reads, cap, &n);  fgpu_destroy(c0);
 *     fgpu_load_begin(c1, FGPU_LOAD_KEEP_READS);  fgpu_load_batch_packed_reads(c1, &blocks[i], &reads[i]) ...;  fgpu_load_end(c1, &stats);
 *
 * _keep_reads: after fgpu_estimate_keep, before the pass' first batch (FGPU_ERR_STATE otherwise).  A batch is then charged (n_reads + 1) * 8
 * bytes more; a batch whose offsets cannot be had ends the keeping like one whose block cannot.
 * _take_kept_reads: after fgpu_estimate_take_kept of the same pass (FGPU_ERR_STATE before it, or in a pass that did not keep reads), in block
 * order; max_read_len is the longest read of the PASS in every entry.  Ownership passes to the caller as with the blocks: fgpu_device_free
 * releases an entry's offsets, fgpu_load_batch_packed_reads hands them on; what is never taken goes with the next fgpu_estimate_begin or
 * fgpu_destroy.  *n_out (may be NULL) = the number of entries, also when cap is too small (FGPU_ERR_ARG, nothing taken).
 * fgpu_load_batch_packed_reads: fgpu_load_batch_packed, in a pass opened with FGPU_LOAD_KEEP_READS (FGPU_ERR_STATE otherwise), plus the
 * adoption of the offsets: on FGPU_OK both allocations are the context's, released with the block; on an error both are still the caller's.
 * FGPU_ERR_ARG: null arguments, reads->n_reads != b->n_reads, no offsets beside a block. */
typedef struct fgpu_kept_reads {
    void*    offsets_dev;      /* (n_reads + 1) x uint64: fgpu_reads.offsets of the batch, on the device */
    uint64_t n_reads;
    uint64_t max_read_len;
} fgpu_kept_reads;
int fgpu_estimate_keep_reads(fgpu_ctx* ctx);
int fgpu_estimate_take_kept_reads(fgpu_ctx* ctx, fgpu_kept_reads* out, uint64_t cap, uint64_t* n_out);
int fgpu_load_batch_packed_reads(fgpu_ctx* ctx, const fgpu_packed* b, const fgpu_kept_reads* reads);

/* ---- a SLICED pass that keeps reads: every rank ends pass 1 holding the whole stream, and a rank can scan any batch it has the offsets of ------
 * After a sliced pass every rank holds every batch in packed form with its `sure` plane; what a scan without the text lacks is the
 * (n_reads + 1) read offsets, which only the rank that packed a batch has seen.  The block format is fixed (tests/pack_ref.py), so the offsets
 * travel SEPARATELY from the block, as a plain array of n_reads + 1 uint64:
 *
 *     fgpu_load_slice_begin / _mercy_begin(lo, hi);  fgpu_load_slice_keep_reads();                 every rank
 *     owner:   fgpu_load_slice_pack(reads, &p)                                                     keeps the offsets beside the block
 *     others:  fgpu_load_slice_expect(T, n, &q) ... fgpu_load_slice_batch_packed(&q)               as without keeping
 *     ... commit, fgpu_load_slice_end on every rank ...
 *     owner:   fgpu_load_slice_packed_reads(&p, &src)                                              device pointer, n_reads, longest read it packed
 *     scanner: fgpu_load_slice_expect_reads(&q, &dst);  fill dst.offsets_dev from src.offsets_dev  (fgpu_group_recv, fgpu_device_copy)
 *              dst.max_read_len = the maximum over the ranks;  fgpu_load_slice_adopt_reads(&q, &dst)
 *     fgpu_scan_kept_range(lo, hi, max over the ranks, &complete);  fgpu_scan_begin;  fgpu_scan_batch_kept(i) / fgpu_scan_prepare_kept(i) ...
 *
 * _keep_reads: inside a sliced pass, plain or mercy, before its first batch or block (FGPU_ERR_STATE otherwise).  fgpu_load_slice_pack then
 * also copies the batch's offsets, device to device inside that call and counted from 0, into an allocation beside the block; (n_reads + 1) * 8 bytes more are
 * charged to the resident budget with the block, and a block or offsets that do not fit are FGPU_ERR_NOMEM with the numbers in the message
 * (fgpu_load_slice_batch keeps its batch's offsets the same way).  Filters, planes, `sure` and stats are bit for bit those of a sliced pass
 * without it.  A batch a rank packed itself is resident WITH its offsets once fgpu_load_slice_batch_packed has loaded it.
 * _packed_reads: the offsets of a block this rank packed (or has adopted offsets for): the context's own memory, valid until the next load
 * pass; max_read_len = the longest read THIS rank packed, known once the pass has ended (0 inside it).
 * _expect_reads: an empty (n_reads + 1) * 8-byte allocation beside a block from fgpu_load_slice_expect, charged to the budget (FGPU_ERR_NOMEM
 * names the numbers); the caller fills all of it.  Called again before the adoption it hands out the same allocation.
 * _adopt_reads: the filled allocation becomes the offsets of the resident batch the block was loaded as (FGPU_ERR_STATE before
 * fgpu_load_slice_batch_packed); reads->max_read_len joins the pass' longest read.  The offsets are CHECKED ON THE DEVICE against the block
 * before any scan uses them -- offsets[0] = 0; ascending; offsets[n] + n = T; for every read the stream position of the separator behind it,
 * offsets[i + 1] + i, is a bad position of the block -- with every position compared with T before the plane is read.  (The offsets a rank
 * hands out start at 0 whatever fgpu_reads.offsets[0] was.)  A violation is reported as FGPU_ERR_ARG, naming the batch, by the next
 * synchronising call (fgpu_synchronize, fgpu_scan_kept_range, fgpu_scan_begin, the end of a pass), as a digest mismatch is; the offsets
 * adopted since the last such call are then dropped again (their allocations stay and may be filled and adopted once more).
 * The last three work inside the sliced pass and after its end, until the next load pass begins.  A description without a block (a batch
 * without reads) has no offsets: FGPU_OK, nothing done.  FGPU_ERR_STATE: the latest load pass was not a sliced pass that keeps reads, or
 * the description is not of a block of it; FGPU_ERR_ARG: null arguments, T / nbytes / n_reads that are not the block's, another allocation. */
int fgpu_load_slice_keep_reads(fgpu_ctx* ctx);
int fgpu_load_slice_packed_reads(fgpu_ctx* ctx, const fgpu_packed* b, fgpu_kept_reads* out);
int fgpu_load_slice_expect_reads(fgpu_ctx* ctx, const fgpu_packed* b, fgpu_kept_reads* out);
int fgpu_load_slice_adopt_reads(fgpu_ctx* ctx, const fgpu_packed* b, const fgpu_kept_reads* reads);

/* filters: raw bit arrays, tai/8 bytes, exactly the .bloom file body (utils/Bloom.cpp:571-587) */
int fgpu_bloom_download(fgpu_ctx* ctx, int which, uint8_t* host_out, uint64_t nbytes);
/* The same copy, started now and finished by fgpu_bloom_download_wait: it runs on its own copy stream behind the work
 * submitted so far, next to whatever the caller submits afterwards (the reference's bloo2 stays in host memory for the dump
 * and for Stage 3, src/Faucet.cpp:220-245 -- the scan in between does not read the host copy).  host_out should be page-locked
 * (fgpu_host_alloc); with pageable memory the call simply blocks until the copy is done.  The filter must not be rewritten
 * (load_begin, bloom_upload) before the wait: those calls wait themselves.  One download in flight per context. */
int fgpu_bloom_download_begin(fgpu_ctx* ctx, int which, uint8_t* host_out, uint64_t nbytes);
int fgpu_bloom_download_wait(fgpu_ctx* ctx);
int fgpu_bloom_upload(fgpu_ctx* ctx, int which, const uint8_t* host_in, uint64_t nbytes);   /* -bloom_file restart */
int fgpu_bloom_weight(fgpu_ctx* ctx, int which, float* weight);                             /* Bloom::weight, Bloom.cpp:191-203 */
int fgpu_bloom_devptr(fgpu_ctx* ctx, int which, void** dptr, uint64_t* nbytes);
/* dst |= src over nbytes (device pointers, nbytes multiple of 16): the local step of the
 * prefix-OR / OR-allreduce that RCCL cannot express as a reduction op. */
int fgpu_bitmap_or(fgpu_ctx* ctx, void* dst_dev, const void* src_dev, uint64_t nbytes);

/* ---- input side: record splitting on the device ------------------------------------------------
 * The reference's reading loop (utils/Bloom.cpp:280-282,340; src/ReadScanner.cpp:306-308,349):
 *     while (getline(header)) { getline(sequence); ...; if (fastq) { getline; getline; } }
 * applied to `nbytes` of file text (host or device memory).  Fills *out with a DEVICE batch (bases = the text on the
 * device, starts/offsets = the sequence line of every record) that stays valid until the next fgpu_text_split on this
 * context, ready for fgpu_load_batch / fgpu_scan_batch / fgpu_presence_batch.
 * final_chunk == 0: only records whose 2 (FASTA) or 4 (FASTQ) lines all end inside the text are taken; *consumed = bytes
 * they occupy -- the caller prepends the rest to the next chunk.  final_chunk != 0: the text ends the file; a last line
 * without a newline, a missing sequence line and missing FASTQ tail lines are handled as getline handles them, called
 * with ONE string as the reference calls it: behind a header that ends with its newline a missing sequence line is an
 * empty read; behind a header that ends with the text (no newline) the failed call leaves the string alone, and the read
 * is that header line.  *consumed = nbytes.  A carriage return before the newline stays part of the line, as it does in
 * the reference. */
/* Page-locked host memory for the text handed to fgpu_text_split (or for read batches): copies to the device then run at
 * link speed and asynchronously.  NULL when it cannot be had; plain malloc'ed memory works too, only slower. */
void* fgpu_host_alloc(uint64_t bytes);
void  fgpu_host_free(void* p);
/* Announces the largest chunk of text (bytes) the caller will hand to fgpu_text_split, so that the first, smaller chunks of a pass do not each
 * make the library free and re-allocate its working buffers (every re-allocation synchronises the device).  A hint: larger chunks still work. */
int fgpu_text_reserve(fgpu_ctx* ctx, uint64_t max_chunk_bytes);
int fgpu_text_split(fgpu_ctx* ctx, const char* text, uint64_t nbytes, int text_on_device, int fastq, int final_chunk,
                    fgpu_reads* out, uint64_t* consumed);

/* ---- pass 2: junction scan (replaces ReadScanner::scanReads, src/ReadScanner.cpp:284-359) ------- */
/* Uses bloo2 as resident on the device (after fgpu_load_end or fgpu_bloom_upload).
 * Device memory: the first scan of a context allocates the junction table (56 bytes per slot of junction_capacity) and the walk's window
 * tables -- 40 bytes per position of the largest scheduling window: 2.5 GiB for filters up to 2^30 bits, up to 10 GiB (windows of 2^28
 * positions) for filters of 2^32 bits and more.  The larger windows only buy speed on thin coverage: where a quarter of the free device
 * memory does not hold them (several contexts on one device, a smaller device) the bound is halved, down to 2^26 positions, before
 * FGPU_ERR_NOMEM is returned. */
/* Between the passes: batch i of the next scan pairs with the load pass' resident batch first_batch + i instead of i, for the reuse of the
 * `sure` planes (fgpu_scan_stats.valid_reused).  After a sliced pass a rank holds the batches of the WHOLE stream while its scan shard begins in
 * the middle of them; without this call the scan compares against the wrong batches -- safely (the streams are compared word for word before
 * anything is reused), but the reuse is lost.  Empty batches are not counted (they keep nothing).  0 again at the next load pass.
 * It shifts the batches of fgpu_scan_batch / fgpu_scan_prepare only: the index of fgpu_scan_batch_kept / fgpu_scan_prepare_kept is always the
 * global one among the pass' non-empty batches.  FGPU_ERR_STATE while a pass is open. */
int fgpu_scan_resident_base(fgpu_ctx* ctx, uint64_t first_batch);
int fgpu_scan_begin(fgpu_ctx* ctx);
/* Pure stage + ordered walk for one batch, in file order. */
int fgpu_scan_batch(fgpu_ctx* ctx, const fgpu_reads* reads);
/* ---- the scan of the batches pass 1 kept: one reading of the input serves both passes --------------------------------------------------------
 * After a load pass opened with FGPU_LOAD_KEEP_READS every resident batch holds what a scan needs (packed stream, sure plane, read offsets).
 * _scan_kept_state: host state only, never waits; valid from fgpu_load_end until the next load pass begins (plain or sliced; fgpu_bloom_upload
 * of bloo2 forgets the batches as well).  *complete = 1 iff the last load pass had the flag and EVERY non-empty batch stayed resident with
 * its offsets; *n_batches, *n_reads, *bytes: the resident batches, their reads, the budget they are charged.  All four may be NULL.
 * _scan_batch_kept: between fgpu_scan_begin and fgpu_scan_end, kept batch i (empty batches keep nothing: i counts the non-empty batches, as
 * for fgpu_scan_resident_base).  In every observable result -- junction records and their creation order, fgpu_scan_stats, stop lists, both
 * pair filters, pair counts, reads_processed -- it equals fgpu_scan_batch on the reads batch i was loaded from; nothing is packed or
 * compared, the sure plane is reused unconditionally (valid_reused grows as for a batch that compared equal).  The batch's planes are COPIED
 * into the scan's buffers (3 bits per position, device to device); the journal, the replay after a voided lazy scan or an outgrown junction
 * table, and the harvest of stop lists work as for fgpu_scan_batch, and text batches may be mixed in.  *n_reads_out (may be NULL) = the
 * batch's reads.  The batches live until the next load pass: a later scan of the same context may scan them again.
 * fgpu_scan_batch's preconditions apply (no prepared batches waiting, no preview in the table).  FGPU_ERR_STATE: outside a scan, or the
 * state is not complete; FGPU_ERR_ARG: i >= n_batches.
 * After a SLICED pass that keeps reads (fgpu_load_slice_keep_reads) a rank holds every batch but only some batches' offsets: _scan_batch_kept(i)
 * works for every resident batch that has them -- i is the global index among the pass' non-empty batches, whatever fgpu_scan_resident_base
 * says -- and answers FGPU_ERR_STATE for a batch without.  _scan_kept_state stays as above (complete = EVERY batch).
 * _scan_kept_range: between the load pass and fgpu_scan_begin; *complete = 1 iff batches [lo, hi) are all resident with their offsets (after a
 * plain pass: iff the state is complete and hi <= n_batches).  It WAITS for the context's stream and reports offsets that failed their check
 * (FGPU_ERR_ARG, fgpu_load_slice_adopt_reads).  max_read_len: the longest read of the pass over ALL ranks -- a scan of kept batches bounds how
 * far a piece reaches by it, and under slices a rank has packed only its own batches -- or 0 after a plain pass.
 * _scan_prepare_kept: the two-step form, fgpu_scan_prepare (below) of the reads batch i was loaded from: ranks above the first run their pure
 * stage from kept batches, take the hint / the table as always, and walk with fgpu_scan_walk_prepared; fgpu_scan_refresh_prepared works on
 * batches prepared this way.  Errors as _scan_batch_kept, without its preconditions on prepared batches and previews. */
int fgpu_scan_kept_state(fgpu_ctx* ctx, int* complete, uint64_t* n_batches, uint64_t* n_reads, uint64_t* bytes);
int fgpu_scan_batch_kept(fgpu_ctx* ctx, uint64_t i, uint64_t* n_reads_out);
int fgpu_scan_kept_range(fgpu_ctx* ctx, uint64_t lo, uint64_t hi, uint64_t max_read_len, int* complete);
int fgpu_scan_prepare_kept(fgpu_ctx* ctx, uint64_t i, uint64_t* n_reads_out);
/* The same in two steps, so that read shards can do the pure part concurrently and only the
 * ordered walk is serial: scan_prepare runs the pure stage and keeps its bit planes resident
 * (about 1.6 bytes of HBM per base); scan_walk_prepared walks every prepared batch in the order
 * they were prepared.  scan_batch(b) == scan_prepare(b); scan_walk_prepared(). */
int fgpu_scan_prepare(fgpu_ctx* ctx, const fgpu_reads* reads);
int fgpu_scan_walk_prepared(fgpu_ctx* ctx);
int fgpu_scan_end(fgpu_ctx* ctx, fgpu_scan_stats* stats);
/* The scan evaluates testForJunction only where its preview of the walk says the walk can stop (lazy
 * flags); where the walk scans a window outside that preview it evaluates the tests itself, so the results are exact either
 * way.  The one case the walk cannot absorb on the spot is such a late test coming out TRUE (a junction at a k-mer the window's dependency
 * clusters did not know, AND whose k-mer occurs on another piece of the same window).  The library absorbs that too: while a scan is lazy it keeps the packed form of every batch in HBM (3 bits per
 * base, up to an eighth of the device memory) and, should the case arise, resets the junction map and scans those batches again by itself
 * with every test evaluated -- the caller sees an ordinary scan and never has to hand its reads over twice (they may come from a pipe).
 * A scan that outgrows that journal is verified up to there and goes on with eager tests.  fgpu_diag_scan_replays counts the replays;
 * fgpu_scan_stats.flags_filled counts the windows evaluated inside the walk.  fgpu_scan_set_eager(ctx, 1) switches the preview off for the
 * following scans altogether (same results as FGPU_FLAG_EAGER_FLAGS, about 1.5x the junction-test probes, no journal). */
int fgpu_scan_set_eager(fgpu_ctx* ctx, int on);
/* The short pair filter on the device.  With cleaning on, scan_forward feeds every piece's result list to
 * short_pair_filter->addPair (src/ReadScanner.cpp:208-225; Bloom::addPair utils/Bloom.cpp:127-139): adds only, so their order is free.
 * After fgpu_scan_short_pairs(tai, n_hash) -- the filter create_bloom_filter_optimal would make, src/Faucet.cpp:266-283 -- every scan keeps
 * that filter in HBM and applies the rules to each batch's lists as they are harvested; fgpu_scan_short_pairs_download (after
 * fgpu_scan_end) returns its tai / 8 bytes, the content of the reference's .short_pair_filter.  lists_to_host = 0: the lists are not
 * brought to the host at all (nothing else reads them, or their other reader -- the long pair filter, fgpu_scan_long_pairs -- is on the
 * device as well; fgpu_scan_take_stops then reports no batches); != 0: they are still handed out (a caller that applies the paired-end
 * loop itself).
 * Needs FGPU_FLAG_RECORD_STOPS; tai = 0 switches it off again.  Only between passes. */
int fgpu_scan_short_pairs(fgpu_ctx* ctx, uint64_t tai, int32_t n_hash, int32_t lists_to_host);
int fgpu_scan_short_pairs_download(fgpu_ctx* ctx, uint8_t* out, uint64_t n_bytes);

/* The long pair filter on the device (src/ReadScanner.cpp:317-343 with Bloom::containsPair / addPair, utils/Bloom.cpp:127-154).
 * With --paired_ends the reference treats consecutive records of the scan file as the two ends of a pair and, when both of their
 * scanInputRead lists are non-empty, CHECKS every k-mer of the first end's list for a partner among the second end's
 * (long_pair_filter->containsPair) and INSERTS (k-mer, second end's first k-mer) when there is none -- check-then-insert in file order.
 * After fgpu_scan_long_pairs(tai, n_hash, FGPU_LONG_PAIRS_FILTER) -- the filter create_bloom_filter_optimal would make, src/Faucet.cpp:268-281 --
 * every scan keeps that filter in HBM and applies the loop to each batch's lists as they are harvested, exactly: every list element gets
 * its file-order time, inserts post first-set times per filter bit, and the check / insert decisions are iterated to their fixed point,
 * which is the sequential run's (faucet_amd/csrc/pairs.hip).  Reads 2p and 2p+1 of the
 * SCAN (counted over all its batches, empty records included) are a pair; a first end at the end of a batch waits for the next batch.
 * FGPU_LONG_PAIRS_COUNT: only the reference's "Empty count / not empty count" (what --no_cleaning leaves of the loop); tai, n_hash unused.
 * fgpu_scan_long_pairs_download (after fgpu_scan_end): the tai / 8 bytes of the reference's .long_pair_filter (out may be NULL) and the two
 * counts.  Lists then leave the device only if fgpu_scan_short_pairs(..., lists_to_host != 0) asks for them.
 * The first-set times have two forms.  DENSE: one per filter bit, 4 bytes of HBM per bit beside the filter's tai / 8.  SPARSE: a table per
 * batch, keyed by bit position -- only the bits that round 0 of a batch posts can carry a time in that batch, at most n_hash per list
 * element -- so the working state is tai / 8 + O(batch) bytes; a table that cannot be allocated is FGPU_ERR_NOMEM from the batch call.
 * FGPU_LONG_PAIRS_FILTER chooses: dense where both allocations succeed, sparse where only the bits fit; FGPU_ERR_NOMEM is left for a filter
 * whose bits themselves do not fit the device (hosts then run the loop themselves, host/pair_loop.h).  FGPU_LONG_PAIRS_FILTER_SPARSE: always
 * sparse.  The environment variable FGPU_LONG_PAIRS_STATE = dense | sparse | auto (read at every call) overrides the choice of
 * FGPU_LONG_PAIRS_FILTER: sparse makes it FGPU_LONG_PAIRS_FILTER_SPARSE, dense answers FGPU_ERR_NOMEM where the 4 bytes per bit do not fit.
 * Both forms compute the same filter, counts and fgpu_diag_long_pairs figures.
 * Needs FGPU_FLAG_RECORD_STOPS; FGPU_LONG_PAIRS_OFF switches it off again.  Only between passes. */
#define FGPU_LONG_PAIRS_OFF 0
#define FGPU_LONG_PAIRS_COUNT 1
#define FGPU_LONG_PAIRS_FILTER 2
#define FGPU_LONG_PAIRS_FILTER_SPARSE 3
int fgpu_scan_long_pairs(fgpu_ctx* ctx, uint64_t tai, int32_t n_hash, int32_t mode);
int fgpu_scan_long_pairs_download(fgpu_ctx* ctx, uint8_t* out, uint64_t n_bytes, uint64_t* empty_count, uint64_t* not_empty_count);

/* scanInputRead's lists of one scanned batch, flattened in processing order (reads in file order; inside a read the
 * valid pieces in the order scanInputRead walks them; inside a piece by half-step).  Batches come out in scan order,
 * one per call: *batch_seq = number of the batch within the scan, or -1 (and *n_out = 0) when none is left.  The
 * call waits for the ordered walk of that batch only, so calling it once after every fgpu_scan_batch (it then returns
 * the previous batch) keeps the walk of the newest batch overlapped; after fgpu_scan_end call it until -1.
 * FGPU_ERR_CAPACITY with *batch_seq >= 0: *n_out = elements needed, nothing consumed; with *batch_seq = -1: the junction table is full
 * (a walk outgrew it where the library cannot absorb that, see fgpu_params.junction_capacity) and no list of the scan is handed out. */
int fgpu_scan_take_stops(fgpu_ctx* ctx, fgpu_stop* out, uint64_t cap, uint64_t* n_out, int64_t* batch_seq);
/* Junction map after the scan, in CREATION order (inserting the records in this order into a
 * std::unordered_map<kmer_type,Junction> reproduces the reference's dump order,
 * utils/JunctionMap.cpp:588-593).  keys are the oriented k-mers (ReadKmer::getKmer). */
int fgpu_scan_junction_count(fgpu_ctx* ctx, uint64_t* n);
int fgpu_scan_download_junctions(fgpu_ctx* ctx, uint64_t* keys, fgpu_junction* recs, uint64_t cap, uint64_t* n_out);
/* Multi-GPU hand-over of the ordered state between consecutive read shards: export on rank r
 * (device buffer of n_entries * FGPU_TABLE_ENTRY_BYTES), import on rank r+1 before its first scan_batch. */
int fgpu_scan_table_entries(fgpu_ctx* ctx, uint64_t* n_entries);
/* The ORDER in which the reference dumps its junctions (JunctionMap::writeToFile, utils/JunctionMap.cpp:579-596: the iteration order of its
 * std::unordered_map, utils/JunctionMap.h:61), computed on the device for the keys of the last fgpu_scan_download_junctions -- which are in
 * creation order = the reference's insertion order.  The container's node list has a closed form (host/junction_order.h): between two rehashes
 * the nodes stand sorted by (first insertion into their bucket, own insertion), both latest first, and a rehash re-inserts the list as it
 * stands -- one radix sort per stretch, about 2 n elements in all.  The caller supplies WHEN its standard library rehashes and to how many
 * buckets (DumpOrder::schedule: asked of the library's own policy object): rehash_counts[j] nodes are present when the table goes to
 * rehash_buckets[j] buckets, first entry {0, buckets of the empty container}; the hash of a 64-bit key is the key (libstdc++).  order[i] =
 * index in creation order of the i-th junction dumped, for the first n keys (n <= the downloaded count; a prefix lets a host check the device
 * against its own container before trusting it).  Replaces a host-side replay that took 5.7 s for 2.95e7 junctions.
 * Preconditions on the schedule, all checked on the host before anything runs on the device (FGPU_ERR_ARG otherwise): n_rehashes >= 1;
 * rehash_counts[0] == 0; the counts do not descend (equal counts = several rehashes in a row) and none exceeds n; every bucket count is in
 * 1 .. 2^32 - 1 (the device keeps a bucket number in 32 bits, and one 4-byte word per bucket of the largest count).  FGPU_ERR_STATE: inside
 * an open pass, before any download, or n above the downloaded count.  n == 0 (after a download of at least one key) writes nothing. */
int fgpu_scan_dump_order(fgpu_ctx* ctx, const uint64_t* rehash_counts, const uint64_t* rehash_buckets, uint64_t n_rehashes, uint64_t n, uint32_t* order);
int fgpu_scan_export_table(fgpu_ctx* ctx, void* dev_buf, uint64_t buf_bytes, uint64_t* n_entries);
int fgpu_scan_import_table(fgpu_ctx* ctx, const void* dev_buf, uint64_t n_entries, const fgpu_scan_stats* carried);
/* A PREVIEW of the table a later shard will be handed: an earlier state of the same ordered table (what the first shard has built
 * after part of its reads).  Imported before (or between) the calls of fgpu_scan_prepare -- before any walk --, it lets the pure stage evaluate the junction tests only where the walk
 * may stop, as it does in a streaming scan -- with an empty table every test of every position is evaluated (2.5x the probes).  Valid
 * because the table only grows along the file (keys are never removed, distances only rise), the same reason a batch may be previewed
 * against the table as of two batches earlier; the walk verifies the preview as always.  The hint is not part of the result: the
 * fgpu_scan_import_table that must follow replaces it, and the walk refuses to start while it is in place (FGPU_ERR_STATE). */
int fgpu_scan_import_hint(fgpu_ctx* ctx, const void* dev_buf, uint64_t n_entries);
/* A FRESHER preview (round 5): fgpu_scan_import_hint may be called again -- still before the real table --, e.g. with the table the shard below
 * has just been HANDED (one hop before this shard's own arrives), and fgpu_scan_refresh_prepared makes the in-map planes of every prepared batch
 * again against it, off the chain of walks.  When fgpu_scan_import_table then brings a later state of that very table, the walk only has to look
 * for the keys created since (found by their creation stamps, counted against the surplus of entries: a table that is NOT a later state of the
 * preview is noticed and handled the long way, exactly): 22 -> ~7 ms per 25 M reads on the chain.  FGPU_NO_DELTA_REFRESH=1: always the long way.
 * fgpu_diag_prepared_refresh (after fgpu_scan_end): [0] batches whose planes the walk made again in full, [1] batches it merged the new keys
 * into, [2] new keys of the last import, [3] with FGPU_DEBUG_DELTA_CHECK=1 (tests): plane words in which the merged planes differed from planes
 * made again in full (must be 0).  The filter of new keys also takes the keys this shard's own batches create as they are walked: the batches
 * behind them were prepared before any of the shard was walked. */
int fgpu_scan_refresh_prepared(fgpu_ctx* ctx);
int fgpu_diag_prepared_refresh(fgpu_ctx* ctx, uint64_t out[4]);
/* Round 6: fgpu_scan_refresh_prepared also makes, for every prepared batch, the plane of positions a link pass of the walk can find at all
 * (their hash is a candidate's by the planes as the preview left them); the merge of the new keys adds the positions that hit the filter of new
 * keys, and the walk links a window by visiting those positions only instead of probing the window table at every position (18 -> 3 ms per
 * 25 M reads on the chain; windows that follow another window of their batch are linked in full).  FGPU_NO_SPARSE_LINK=1: every window in full.
 * fgpu_diag_sparse_link (after fgpu_scan_end): [0] windows of prepared batches linked by the plane, [1] in full; FGPU_DEBUG_DELTA_CHECK=1 runs
 * the full pass behind every sparse one and counts differing lk words into fgpu_diag_prepared_refresh's [3]. */
int fgpu_diag_sparse_link(fgpu_ctx* ctx, uint64_t out[2]);
#define FGPU_TABLE_ENTRY_BYTES 32

/* The two pair filters as they stand on the device while a scan is open (after fgpu_scan_begin, which empties them): which = 0 the short
 * one (fgpu_scan_short_pairs), 1 the long one (fgpu_scan_long_pairs, FGPU_LONG_PAIRS_FILTER); tai / 8 bytes each.  For read shards walked one
 * after the other (several GPUs): the filters a shard ends with are what the next shard starts from -- the short filter only collects adds, the
 * long one is check-then-insert in file order, and a shard that begins at an even record finds no first end waiting.  The next shard copies
 * them in (fgpu_group_recv / fgpu_device_copy on the context's stream) before its first walk. */
int fgpu_scan_pairs_devptr(fgpu_ctx* ctx, int which, void** dptr, uint64_t* nbytes);

/* ---- device memory for the host's exchange buffers (HIP stays behind the ABI) -------------------- */
int fgpu_device_alloc(fgpu_ctx* ctx, uint64_t nbytes, void** dptr);      /* on the context's device */
int fgpu_device_free(fgpu_ctx* ctx, void* dptr);                          /* waits for the context's stream first */
int fgpu_device_copy(fgpu_ctx* ctx, void* dst_dev, const void* src_dev, uint64_t nbytes);   /* on the context's stream */
int fgpu_device_zero(fgpu_ctx* ctx, void* dst_dev, uint64_t nbytes);                        /* on the context's stream */

/* ---- several GPUs driven by ONE process: a group of contexts and their exchanges -----------------
 * The reference is a single process (src/Faucet.cpp:204-245); BASELINE.json's north_star shards its reads over the GPUs of one node.
 * A group ties N contexts together -- one per rank, each driven by its own host thread (the rule above), each on its own device, or
 * several on one device where there are fewer devices than ranks (tests) -- and moves DEVICE buffers between them on the contexts' own
 * streams: whatever a context has queued before an exchange is finished before its buffers are read, whatever it queues afterwards
 * sees what has arrived, and no call waits for a device.  Host threads do wait for each other (a receive for its send to be posted, a
 * send for its receive), which is the only synchronisation there is.
 *   FGPU_TRANSPORT_COPY  device-to-device copies inside the process (hipMemcpyPeerAsync over xGMI between devices), ordered by events
 *   FGPU_TRANSPORT_RCCL  ncclSend / ncclRecv on one communicator per rank (librccl.so is loaded when the first such group is made);
 *                        needs one device per rank (RCCL refuses two ranks on one device)
 * Every rank's thread makes the same sequence of collective calls; point-to-point calls pair up per (source, destination) in the order
 * they are made.  An error on one rank: fgpu_group_abort wakes every thread that waits and makes all further calls fail. */
typedef struct fgpu_group fgpu_group;
#define FGPU_TRANSPORT_COPY 0
#define FGPU_TRANSPORT_RCCL 1
int         fgpu_group_create(int n_ranks, int transport, fgpu_group** out);
void        fgpu_group_destroy(fgpu_group* g);                /* after every rank's thread has stopped using it */
/* rank's thread: ties ctx to the rank; returns when every rank has attached (RCCL: the communicators exist) */
int         fgpu_group_attach(fgpu_group* g, int rank, fgpu_ctx* ctx);
void        fgpu_group_abort(fgpu_group* g);
const char* fgpu_group_last_error(const fgpu_group* g, int rank);
int         fgpu_group_barrier(fgpu_group* g, int rank);       /* host threads only; no device is waited for */
/* bitmap := OR over ranks, in place on every rank (nbytes a multiple of 16, the same on all): reduce-scatter by slices -- rank q collects
 * slice q of everybody and reduces it with the OR kernel -- then all-gather of the reduced slices: 2 (N-1)/N of a bitmap crosses each
 * rank's links per call.  RCCL has no bitwise-OR reduction (rccl.h: ncclSum/Prod/Max/Min/Avg).  bloo2 after pass 1. */
int fgpu_group_or_allreduce(fgpu_group* g, int rank, void* bitmap_dev, uint64_t nbytes);
/* buf := every rank's part of it, in place: bounds[0..N] are byte offsets into buf, ascending, bounds[N] <= nbytes, the same on all ranks; rank q
 * holds [bounds[q], bounds[q+1]) and afterwards every rank holds [bounds[0], bounds[N]).  Empty ranges are allowed; no alignment is asked for.  The
 * all-gather half of fgpu_group_or_allreduce with the caller's ranges: the filters after a sliced pass 1, by the slices' byte ranges.
 * FGPU_ERR_ARG: null arguments, bounds that descend or pass nbytes. */
int fgpu_group_allgather(fgpu_group* g, int rank, void* buf_dev, uint64_t nbytes, const uint64_t* bounds);
/* out := OR of the bitmaps of all ranks below `rank` (zero on rank 0); bitmap is left as it is.  The carried-in bloo1 of a read shard
 * (what the sequential run has in bloo1 when it reaches the shard). */
int fgpu_group_exclusive_prefix_or(fgpu_group* g, int rank, const void* bitmap_dev, void* out_dev, uint64_t nbytes);
/* point to point.  send: the buffer must stay as it is until the matching receive has run; the call returns once the receiver has
 * queued its copy (its thread has called fgpu_group_recv) and orders the sender's stream behind that copy.  send_async returns at once --
 * for a buffer nothing writes again before fgpu_group_flush (the table preview of DESIGN.md section 5).  probe: is a send from src waiting
 * (*nbytes its size)?  Never blocks. */
int fgpu_group_send(fgpu_group* g, int rank, int dst, const void* dev, uint64_t nbytes);
int fgpu_group_send_async(fgpu_group* g, int rank, int dst, const void* dev, uint64_t nbytes);
int fgpu_group_flush(fgpu_group* g, int rank);
int fgpu_group_recv(fgpu_group* g, int rank, int src, void* dev, uint64_t nbytes);
int fgpu_group_probe(fgpu_group* g, int rank, int src, int* waiting, uint64_t* nbytes);
/* the transport moves nbytes from a buffer of this rank to another buffer of this rank (RCCL: a send to itself and its receive in one group)
 * and the result is compared on the host: *ok = 1 iff every byte arrived.  What a box with one device can show of the RCCL transport. */
int fgpu_group_selftest(fgpu_group* g, int rank, uint64_t nbytes, int* ok);
/* The collective end of pass 0: every rank has sketched its shard of the reads on its own context (fgpu_estimate_begin / _batch with the same
 * r_bits) and its thread calls this in place of fgpu_estimate_end.  Every rank returns the same fgpu_estimate, that of ONE sketch of all the
 * reads, to the last counter:
 *   1  the ranks agree: a rank that is not in an estimate pass gives EVERY rank FGPU_ERR_STATE, ranks with different r_bits FGPU_ERR_ARG;
 *   2  the planes are cut into N ranges of 16-byte granules, as fgpu_group_or_allreduce slices a bitmap (uneven and empty ranges allowed);
 *      rank q collects range q of every other rank -- the reduce-scatter half of that call, through the group's own sends and receives --
 *      into a staging buffer, chunk by chunk, and merges each chunk into its planes (fgpu_estimate_merge).  The staging buffer holds one
 *      chunk per peer and never more than 128 MiB in all, whatever r_bits and N; FGPU_ESTIMATE_MERGE_CHUNK = bytes per peer and step (read
 *      at every call, rounded down to 16, the same for all ranks of the process) overrides the chunk size, for tests;
 *   3  rank q counts its merged range; empty[], once[] and kmers are summed over the ranks on the host (counts add over disjoint ranges of
 *      cells: no rank ever holds the whole merged sketch), and every rank runs fgpu_estimate_solve on the sums.
 * The pass ends on every rank whatever the status: planes given back, the context idle.  A rank's planes are freed only once every rank has
 * waited for its device -- a peer's copy out of them has been queued, not finished, when the send returns -- and, after a failure, only by
 * fgpu_group_destroy.  FGPU_ERR_CAPACITY comes back on every rank with the counts filled in, as from fgpu_estimate_end.  A failure of one rank
 * inside steps 2 and 3 aborts the group (fgpu_group_abort): the others return FGPU_ERR_STATE.  A group of one rank: fgpu_estimate_end. */
int fgpu_group_estimate_end(fgpu_group* g, int rank, fgpu_estimate* out);

/* ---- probes for tests (pure, no state change) ------------------------------------------------- */
/* For each of n k-mers (2-bit encoded, utils/Kmer.cpp:82-88,410-425): canonical form and
 * hA = oldHash(canon,0), hB = oldHash(canon,1) masked with tai-1 (utils/Bloom.h:134-145). */
int fgpu_probe_hash(fgpu_ctx* ctx, const uint64_t* kmers_host, uint64_t n, uint64_t* canon_out, uint64_t* hA_out, uint64_t* hB_out);
/* Bloom::oldContains (utils/Bloom.h:162-173) of n canonical k-mers against filter `which`. */
int fgpu_probe_contains(fgpu_ctx* ctx, int which, const uint64_t* canon_host, uint64_t n, uint8_t* out);

/* ---- Stage 3's Bloom probes, batched -----------------------------------------
 * The contig-graph stage walks the filter from every junction (JunctionMap::findNeighbor, utils/JunctionMap.cpp:231-412); its map
 * look-ups and its control flow stay on the host, its filter work is these pure functions of bloo2, here for n forward-strand
 * k-mers at once (one walk step of many junctions in lock-step):
 *   jcheck            JChecker::jcheck(kmer_type)              utils/JChecker.cpp:51-80      -> 0 / 1
 *   valid_extension   JunctionMap::getValidJExtension          utils/JunctionMap.cpp:474-490 -> -1 none, -2 several, else 0..3
 *   bloom_junction    JunctionMap::isBloomJunction             utils/JunctionMap.cpp:494-504 -> 0 / 1
 * (Bloom::oldContains itself is fgpu_probe_contains.) */
int fgpu_probe_jcheck(fgpu_ctx* ctx, const uint64_t* kmers_host, uint64_t n, int8_t* out);
int fgpu_probe_valid_extension(fgpu_ctx* ctx, const uint64_t* kmers_host, uint64_t n, int8_t* out);
int fgpu_probe_bloom_junction(fgpu_ctx* ctx, const uint64_t* kmers_host, uint64_t n, int8_t* out);

/* ---- Stage 3's walks, whole ------------------------------------------------------
 * JunctionMap::findNeighbor(Junction junc, kmer_type startKmer, int index) (utils/JunctionMap.cpp:231-412) for n (junction, extension)
 * pairs at once, one device lane per walk: every getValidJExtension, every DoubleKmer step and every junctionMap.find of the walk happens
 * on the device, against bloo2 as it stands (after a load, or fgpu_bloom_upload) and against the junction map handed over by
 * fgpu_stage3_set_junctions (k-mers as JunctionMap keys them, i.e. as fgpu_scan_download_junctions / a .junctions file give them; only the
 * five distances of a record are read, as in the reference).  The map stays on the device until it is set again.
 * Result per walk = the reference's return value: the BaseNode* it would build -- `node` 1: a junction was reached (`kmer` its key, `rindex`
 * the index it was entered through, 4 = backward), 0: a sink (`rindex` as the reference sets it) -- with the distance and the contig
 * length the reference reports through its pointer arguments.  `abort` 1 marks the calls in which the reference trips one of its asserts
 * (dist <= maxDist after the first k-mers; validExtension >= 0 at every step up to maxDist; getValidJExtension >= 0 at a junction met
 * before maxDist, :355 and :370) instead of returning; 2 = startKmer is not in the map or index is not 0..4.
 * n_probes (may be NULL): getValidJExtension evaluations made (the one of an early junction's assert included), each up to 4 x
 * (Bloom::oldContains + JChecker::jcheck).
 * contigs_out (may be NULL): BfSearchResult::contig of every walk, the sequence getContig (utils/JunctionMap.cpp:133-227) appends to its
 * contig string: walk w's string is `len` bases in contigs_out[w * contig_stride_words ..], 2 bits per base in the reference's code
 * (A 0, C 1, T 2, G 3), 32 bases per word, the first base in the lowest bits; contig_stride_words >= fgpu_stage3_contig_words(k,
 * max_read_length). */
typedef struct {
    uint64_t kmer;
    int32_t  dist;
    int32_t  len;
    int8_t   node;
    int8_t   rindex;
    int8_t   abort;
    int8_t   reserved;
    int32_t  reserved2;
} fgpu_neighbor;
int fgpu_stage3_set_junctions(fgpu_ctx* ctx, const uint64_t* keys_host, const fgpu_junction* recs_host, uint64_t n);
int fgpu_stage3_find_neighbors(fgpu_ctx* ctx, const uint64_t* start_kmers_host, const int8_t* indices_host, uint64_t n,
                               int32_t max_read_length, fgpu_neighbor* out, uint64_t* n_probes, uint64_t* contigs_out,
                               uint64_t contig_stride_words);
uint64_t fgpu_stage3_contig_words(int32_t k, int32_t max_read_length);

/* ---- Stage 3's contigs: whole getContig chains -------------------------------------
 * JunctionMap::getContig(junctionMap[start], start, index) (utils/JunctionMap.cpp:133-221) for n starts at once, against bloo2 and the map of
 * fgpu_stage3_set_junctions as they stand (here the four coverages of a record are read as well): findNeighbor after findNeighbor through
 * every junction with one path out (Junction::numPathsOut() == 1; on at getOppositeIndex(result.index): 4 after a forward entry, the covered
 * extension after a backward one) until a complex junction, a sink, or the start k-mer again.  The map is static within the call -- the
 * reference kills the junctions of a chain only behind its loop (:210-216) -- so every chain is a function of (map, filter, start) alone,
 * and which answers a graph build may still use after the kills of earlier ones is not this call's business: fgpu_stage3_build below.
 * Cost: one call walks every directed segment it can need once -- the n first calls, and up to two per junction with one path out --
 * whatever n is, and keeps nothing for the next call: hand over all starts of a stage in one call.
 * Per chain: the string (print_kmer(start), its reverse complement for index 4, then result.contig.substr(k) of every segment longer than
 * k), distances (one byte per findNeighbor call), coverages (getCoverage(startIndex), then nextJunc.getCoverage(result.index) of every
 * call that ended at a junction; getCoverage(4) is the sum of the four; each a byte) and the k-mer every call ended at: seg_kmers of all
 * segments but the last ARE kmers_to_destroy.  The string starts at a word of its own, 2 bits per base in fgpu_stage3_find_neighbors' code,
 * 32 bases per word, first base lowest, the bits behind `len` zero.
 * status 0: the reference returns; 1: a call of the chain trips one of the reference's asserts (fgpu_neighbor.abort == 1); 2: the start is
 * not in the map, or the index is not 0..4; 3: the chain runs into a cycle that does not hold the start k-mer -- the reference's
 * while(!done) never returns (found in a number of hops proportional to the chain's own tail and cycle).  With a status other than 0,
 * len, n_seg and n_cov are 0 and nothing of the chain is stored.
 * fgpu_stage3_contigs keeps the arrays on the device and says how long they are (totals: text words, segments, coverages; all 0 for
 * n == 0); fgpu_stage3_contigs_take copies them out and frees them.  An array with fewer entries than the totals is FGPU_ERR_ARG: nothing
 * is copied, and the results are still there.  Results that were not taken are dropped by the next fgpu_stage3_contigs or
 * fgpu_stage3_build. */
typedef struct {
    uint64_t end_kmer;    /* BfSearchResult::kmer of the chain's last findNeighbor call */
    uint64_t text_word;   /* first word of this contig's string in the text array */
    uint64_t seg_first;   /* first entry of this chain in the per-segment arrays */
    uint64_t cov_first;   /* first entry of this chain in the coverage array */
    uint32_t len;         /* bases of contigString */
    uint32_t n_seg;       /* findNeighbor calls made = distances.size() */
    uint32_t n_cov;       /* coverages.size() */
    int8_t   ind1, ind2;  /* setIndices(startIndex, result.index or 4), :201-208 */
    int8_t   end_node;    /* the last result's isNode */
    int8_t   status;
} fgpu_contig;
int fgpu_stage3_contigs(fgpu_ctx* ctx, const uint64_t* start_kmers_host, const int8_t* indices_host, uint64_t n, int32_t max_read_length,
                        fgpu_contig* out, uint64_t totals[3], uint64_t* n_probes);
int fgpu_stage3_contigs_take(fgpu_ctx* ctx, uint64_t* text, uint64_t text_words, uint64_t* seg_kmers, uint8_t* seg_dist, uint64_t n_seg,
                             uint8_t* cov, uint64_t n_cov);

/* ---- Stage 3's graph build: the order-dependent contig list ----------------------
 * Every getContig call JunctionMap::buildContigGraph (utils/JunctionMap.cpp:11-129) makes, each on the map as it stands at that moment, in the
 * reference's order, in one call: buildBranchingPaths' map-order loop (:34-82: every covered index 0..4 of every junction with more than one
 * path out that has no contig yet, :50; the homopolymer rule :43-47 on the start's own copy), destroyComplexJunctions (:90-102), and
 * buildLinearRegions' loop (:104-129: of every junction still there, the call on its covered extension and then the one on 4), with every
 * getContig erasing the inner junctions of its chain behind itself (:210-216) and Contig::setEnds (src/Contig.cpp:123-133) taking contigs[]
 * of the start node and, where isJunction(Contig::getSideKmer(2)) holds on the map behind the call's own kills (:54-74;
 * src/Contig.cpp:229-241), of the far node.  Map order is the order of the keys handed to fgpu_stage3_set_junctions.  The graph itself
 * (ContigGraph, concatenate :120) stays with the caller: the two chains of a linear region come back as two calls, forward then backward.
 * Per call that is made: an fgpu_contig as fgpu_stage3_contigs fills it (status 0; the shared arrays in fgpu_stage3_contigs_take's
 * layout) and an fgpu_build_call beside it.  Calls that are skipped -- the start is gone, or its (node, index) has a contig -- are not
 * output.
 * The build ends at the first call that is made on which the reference does not return (fgpu_build_info.status 1: it trips an assert; 3:
 * while(!done) never ends; 0: the build ran to its end); the calls before it are output, stop_call is their number.
 * fgpu_stage3_build keeps the results on the device and gives totals (calls made, text words, segments, coverages);
 * fgpu_stage3_build_take copies them out and frees them.  An array with fewer entries than the totals is FGPU_ERR_ARG: nothing is copied and
 * the results are still there.  Results that were not taken are dropped by the next fgpu_stage3_build or fgpu_stage3_contigs.
 * The call is a fixed point over rounds; more than calls + 1 rounds is FGPU_ERR_INTERNAL. */
#define FGPU_BUILD_BRANCHING       0
#define FGPU_BUILD_LINEAR_FORWARD  1
#define FGPU_BUILD_LINEAR_BACKWARD 2
#define FGPU_BUILD_ROUNDS_KEPT     32
typedef struct {
    uint64_t start_kmer;
    uint64_t far_kmer;         /* Contig::getSideKmer(2) */
    uint32_t time;             /* the call's place among all calls the reference could make (skipped ones and destroyComplexJunctions count) */
    uint8_t  phase;            /* FGPU_BUILD_* */
    uint8_t  far_is_junction;  /* isJunction(far_kmer), :56 */
    uint8_t  far_is_start;     /* ... and far_kmer == kmer, :58 */
    uint8_t  reserved;
} fgpu_build_call;
typedef struct {
    int32_t  status;
    uint32_t rounds;           /* rounds of the fixed point, the last one (in which nothing changed) included */
    uint64_t stop_call;        /* calls output = the number of the call the build stopped at, if it did */
    uint64_t calls_possible;   /* time slots: calls the reference could make, and one for destroyComplexJunctions */
    uint64_t rewalked;         /* getContig evaluations over all rounds (round 0 evaluates every call) */
    uint64_t probes;           /* getValidJExtension evaluations in them */
    uint64_t table_hits;       /* junction-map hits the evaluations recorded (what each answer depends on), all rounds */
    uint64_t regrown;          /* times a round outgrew the room for them and was run again with twice as much */
    uint64_t rewalked_by_round[FGPU_BUILD_ROUNDS_KEPT];   /* ... of the first rounds */
} fgpu_build_info;
int fgpu_stage3_build(fgpu_ctx* ctx, int32_t max_read_length, uint64_t totals[4], fgpu_build_info* info);
int fgpu_stage3_build_take(fgpu_ctx* ctx, fgpu_contig* contigs, fgpu_build_call* calls, uint64_t n_calls, uint64_t* text, uint64_t text_words,
                           uint64_t* seg_kmers, uint8_t* seg_dist, uint64_t n_seg, uint8_t* cov, uint64_t n_cov);

/* ---- Stage 3's first product: the build's contigs as FASTA ------------------------
 * ContigGraph::printContigs (src/ContigGraph.cpp:1532-1645) on the graph JunctionMap::buildContigGraph returns: the file the reference
 * names <prefix>.raw_contigs.fasta (src/Faucet.cpp:314).  Three layers, each callable alone.
 *
 * fgpu_raw_plan -- host only, no device, no text: WHAT is printed, and in which order.  From the map (keys and records in map order) and a
 * finished build's fgpu_contig / fgpu_build_call arrays it makes the reference's graph -- nodeMap, a real std::unordered_map<uint64_t, ...>
 * that takes the reference's inserts in the reference's order (ContigGraph::createContigNode, src/ContigGraph.cpp:1656: the start of every
 * complex junction the branching loop visits, utils/JunctionMap.cpp:42, and the far junction of a call whose far_is_junction holds and whose
 * far_is_start does not, :66; an insert of a key that is there changes nothing), every node a copy of its junction's four coverages (the
 * homopolymer rule :43-47 zeroes one of a node visited as a start), Contig::setEnds (src/Contig.cpp:123-133) filling contigs[ind1] of the
 * start node and contigs[ind2] of the far node (far_is_start: both of the start node), and isolated_contigs, one per linear region in call
 * order (utils/JunctionMap.cpp:120) -- and then walks it as the two printing passes do:
 *   printAndMarkBubbleContigs (:1543-1580), over nodeMap in the container's order: a node with exactly two covered extensions whose two
 *     contigs have the same other-end node, and have one (isBubbleNode :490-503, allSame :153-162) and whose contigs[4] is shorter than 250
 *     bases prints getNewConcatenatedContig(contigs[4], contigs[i], node) (:1509-1530) for every unmarked contigs[i], i = 0..3, while
 *     contigs[4] is unmarked, and marks contigs[i]; contigs[4] is marked behind the node.  contigs[4] is reversed if Contig::getSide(node)
 *     is 1 (node1_p is tested first, src/Contig.cpp:243-253), contigs[i] if it is 2.
 *   printUnmarkedUnitigs (:1605-1645), over nodeMap again: every unmarked contigs[0..4], marked as printed; then every isolated contig
 *     of at least read_length bases, backward->concatenate(forward, 1, 1): the backward chain reversed, then the forward one.
 * One fgpu_fasta_seq per record, in file order: one or two pieces of the text (first word, bases, flip = reverse-complemented); the
 * second piece is appended behind the first WITHOUT ITS LAST k BASES (ContigJuncList::concatenate, utils/ContigJuncList.cpp:107-123).
 * `number` is the n of ">Contig<n>", counting from 1 through both passes.  The 250 test and the read_length test read the len fields only.
 * The canonical orientation (canon_contig) is not decided here.
 * Returns FGPU_PLAN_OK; FGPU_PLAN_UNSET: the reference would read a contig pointer nobody set (a bubble test on a node with a covered
 * extension or a back that has no contig; the reference's behaviour is undefined there) -- nothing is guessed; FGPU_PLAN_INPUT: the arrays
 * are not a finished build of this map (a start that is not a key of the map, a linear forward call without its backward one, a branching
 * call behind a linear one, an index outside 0..4, a contig shorter than k); FGPU_PLAN_SHORT: more than cap records (*n_out says how many;
 * n_calls always suffices).  With FGPU_PLAN_OK and FGPU_PLAN_SHORT `info` is filled.
 *
 * fgpu_stage3_fasta -- the device: join, orient and print n records.  text_host == NULL: the pieces index the text of the last
 * fgpu_stage3_build whose results are still on the device (FGPU_ERR_STATE if there is none); the build's results are neither freed nor
 * changed.  text_host != NULL: text_words words of 2-bit text (fgpu_stage3_contigs_take's layout and code) are uploaded first.  A piece
 * that reaches past the text, a piece of no bases, a first piece of two that is shorter than k, or `pieces` other than 1 or 2 is
 * FGPU_ERR_ARG.  Every record is ">Contig<number>\n<sequence>\n", the sequence or its reverse complement, whichever is not greater AS A
 * STRING OF LETTERS (canon_contig, utils/Kmer.cpp:345-351: A < C < G < T, not the order of the 2-bit codes; a reverse-complement
 * palindrome stays as it is).  The bytes stay on the device, *bytes says how many (0 for n == 0); fgpu_stage3_fasta_take copies them out
 * and frees them.  A buffer shorter than that is FGPU_ERR_ARG: nothing is copied, and the results are still there.  Results that were not
 * taken are dropped by the next fgpu_stage3_fasta or fgpu_stage3_raw_contigs.
 *
 * fgpu_stage3_raw_contigs -- both, on a finished build that has not been taken and whose status is 0 (otherwise FGPU_ERR_ARG and a message:
 * with status 1 or 3 the reference itself does not get as far as printing).  Only the two record arrays of the build come to the host;
 * fgpu_raw_plan's status other than FGPU_PLAN_OK is FGPU_ERR_STATE with a message.  Afterwards fgpu_stage3_build_take still returns the
 * build, unchanged, and fgpu_stage3_fasta_take the file. */
#define FGPU_PLAN_OK    0
#define FGPU_PLAN_UNSET 1
#define FGPU_PLAN_INPUT 2
#define FGPU_PLAN_SHORT 3
typedef struct {
    uint64_t text_word[2];   /* first word of each piece's string in the text */
    uint32_t len[2];         /* bases of each piece */
    uint8_t  flip[2];        /* 1: the piece is reverse-complemented before it is joined */
    uint8_t  pieces;         /* 1 or 2 */
    uint8_t  reserved;
    uint32_t number;         /* >Contig<number> */
} fgpu_fasta_seq;
typedef struct {
    uint64_t records;           /* records of the file */
    uint64_t bubble_records;    /* ... printed by printAndMarkBubbleContigs (two pieces each) */
    uint64_t node_contigs;      /* ... printed by printUnmarkedUnitigs off a node */
    uint64_t isolated_kept;     /* ... isolated contigs of at least read_length bases */
    uint64_t isolated_dropped;  /* isolated contigs below read_length: not printed */
    uint64_t nodes;             /* entries of nodeMap */
} fgpu_raw_info;
int fgpu_raw_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                  uint64_t n_calls, int32_t k, int32_t read_length, fgpu_fasta_seq* out, uint64_t cap, uint64_t* n_out, fgpu_raw_info* info);
int fgpu_stage3_fasta(fgpu_ctx* ctx, const fgpu_fasta_seq* seqs_host, uint64_t n, const uint64_t* text_host, uint64_t text_words, uint64_t* bytes);
int fgpu_stage3_fasta_take(fgpu_ctx* ctx, char* out, uint64_t bytes);
int fgpu_stage3_raw_contigs(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_raw_info* info);

/* ---- Stage 3's contigs joined: ContigJuncList::concatenate over piece lists, on the device ----
 * What ContigGraph's cleaning steps make of the build's contigs are JOINS of them: Contig::concatenate (src/Contig.cpp:83-109) reverses either
 * side where it has to (ContigJuncList::reverse, utils/ContigJuncList.cpp:98-103: both lists reversed, the sequence reverse-complemented) and
 * calls ContigJuncList::concatenate (utils/ContigJuncList.cpp:107-123), again and again as collapseNode (src/ContigGraph.cpp:709-736) takes
 * node after node out.  A contig of the cleaned graph is therefore an ordered list of PIECES (a contig of the build, flip), consecutive
 * pieces overlapping by k bases, and its three members are functions of that list alone:
 *   seq        every piece but the last gives its first len - k bases as it is read (flip: reverse-complemented) -- which may be none --,
 *              the last piece all of them (:121)
 *   distances  the pieces' lists one behind the other, a flipped piece's reversed (:119-120)
 *   coverages  ... likewise, but the last entry of the left side and the first of the right become ONE entry, the smaller of the two (:109-117).
 *              Applied left to right an output entry is the minimum over a run of the concatenated oriented inputs: of length 1 inside a
 *              piece, 2 at a join, and longer where middle pieces hold a single coverage entry (that entry is the left side's last AND,
 *              one call on, the result's last again).  n_cov = the sum of the pieces' n_cov minus (pieces - 1).
 *   cov_sum    the sum of the joined coverages: cov_sum / (double) n_cov IS ContigJuncList::getAvgCoverage (:166-176) -- every partial sum of
 *              at most 2^53 / 255 bytes is exact in double -- which chimera removal, bulge collapsing and disentangling read.
 * fgpu_stage3_join: n lists as a CSR -- list i is pieces[list_first[i] .. list_first[i + 1]), list_first[0] = 0, list_first[n] = n_pieces, no
 * list empty.  contigs_host == NULL: `call` indexes the calls of the last fgpu_stage3_build whose results are still on the device
 * (FGPU_ERR_STATE if there is none), and its text, distances and coverages are read where they lie; only its fgpu_contig records come to the
 * host, to be checked.  The build is neither freed nor changed.  The other five array arguments must then be NULL / 0.  contigs_host !=
 * NULL: n_contigs records and the three arrays they index, in fgpu_stage3_contigs_take's layout, are uploaded first (end_kmer, ind1, ind2,
 * end_node, status are not read).  FGPU_ERR_ARG, with a message, totals 0, nothing launched and earlier results untouched (out[] may hold the lists checked so far): a CSR that is not one; a `call` that is no record; a
 * flip other than 0 / 1; a piece that reaches past one of the arrays, has no bases or 2^30 and more, or has no coverage entry; a piece
 * other than a list's last that is shorter than k; a joined string of 2^32 bases and more.
 * Per list an fgpu_joined in out[i]; the joined strings (each from a word of its own, first base lowest, the bits behind `len` zero: what
 * fgpu_stage3_fasta's kernels print from), distances and coverages stay on the device, totals says how long they are (text words,
 * distances, coverages; all 0 for n == 0).  fgpu_stage3_join_take copies them out and frees them; an array with fewer entries than the
 * totals is FGPU_ERR_ARG: nothing is copied, and the results are still there.  Results that were not taken are dropped by the next
 * fgpu_stage3_join. */
typedef struct {
    uint32_t call;        /* the piece: record `call` of the contigs */
    uint32_t flip;        /* 1: read reversed (ContigJuncList::reverse) */
} fgpu_join_piece;
typedef struct {
    uint64_t text_word;   /* first word of the joined string in the joined text */
    uint64_t dist_first;  /* first entry in the joined distances */
    uint64_t cov_first;   /* first entry in the joined coverages */
    uint64_t cov_sum;     /* sum of the joined coverages */
    uint32_t len;         /* bases */
    uint32_t n_dist;
    uint32_t n_cov;
    uint32_t reserved;
} fgpu_joined;
int fgpu_stage3_join(fgpu_ctx* ctx, const uint64_t* list_first, uint64_t n, const fgpu_join_piece* pieces, uint64_t n_pieces,
                     const fgpu_contig* contigs_host, uint64_t n_contigs, const uint64_t* text_host, uint64_t text_words,
                     const uint8_t* dist_host, uint64_t n_dist, const uint8_t* cov_host, uint64_t n_cov, fgpu_joined* out, uint64_t totals[3]);
int fgpu_stage3_join_take(fgpu_ctx* ctx, uint64_t* text, uint64_t text_words, uint8_t* dist, uint64_t n_dist, uint8_t* cov, uint64_t n_cov);

/* ---- Stage 3's coverage summaries: what a cleaning step reads of a contig's coverages, without joining anything ----
 * removeChimericExtensions (src/ContigGraph.cpp:642-707) and the steps behind it decide on ContigJuncList::getAvgCoverage
 * (utils/ContigJuncList.cpp:162-172) of a few contigs per node.  A coverage list enters that, and ContigJuncList::concatenate (:107-123) and
 * reverse (:98-103), through four numbers -- sum, entries, first entry, last entry: struct fgpu_cov_summary, 16 bytes, defined with its two
 * operations in faucet_amd/csrc/cov_summary.h (concatenate: m = min(A.last, B.first); sum = A.sum + B.sum - A.last - B.first + m; n = A.n + B.n
 * - 1; first = A.n == 1 ? m : A.first; last = B.n == 1 ? m : B.last.  reverse swaps first and last.  concatenate is associative).  So the
 * average of any contig of a cleaned graph is a fold over its piece list of the summaries of the build's calls, which is all the device has
 * to hand over: no string, distance or coverage of a joined contig is made for it.
 * fgpu_stage3_cov_calls: one summary per contig record into out_host[0 .. n).  contigs_host == NULL: the records are the calls of the last
 * fgpu_stage3_build whose results are still on the device (FGPU_ERR_STATE if there is none; out_host has room for totals[0] records), and its
 * records and coverages are read where they lie: the build wrote both itself, so nothing of it comes to the host.  The build is neither freed nor changed.
 * n_contigs, cov_host and n_cov must then be 0 / NULL.  contigs_host != NULL: n_contigs records (cov_first and n_cov are read, nothing else)
 * and the n_cov coverage bytes they index, in fgpu_stage3_contigs_take's layout, are uploaded first; the records may lie in any order and
 * may share entries.  A record of no entries gives (0, 0, 0, 0).  FGPU_ERR_ARG with a message and nothing launched: a record that reaches
 * past the coverages, a coverage array of some entries that is NULL, records and no out_host.  Nothing stays on the device.
 * The record's layout, for a caller that does not include cov_summary.h (C++): 16 bytes, 8-byte aligned -- uint64_t sum at 0, uint32_t n at 8,
 * uint8_t first at 12, uint8_t last at 13, two reserved bytes (0).
 * fgpu_stage3_build_totals: the four totals of the last fgpu_stage3_build whose results are still on the device (calls, text words, segments,
 * coverages; totals[0] is how many records the on-device form of fgpu_stage3_cov_calls writes); FGPU_ERR_STATE if there is none. */
struct fgpu_cov_summary;
int fgpu_stage3_build_totals(fgpu_ctx* ctx, uint64_t totals[4]);
int fgpu_stage3_cov_calls(fgpu_ctx* ctx, const fgpu_contig* contigs_host, uint64_t n_contigs, const uint8_t* cov_host, uint64_t n_cov,
                          struct fgpu_cov_summary* out_host);

/* ---- Stage 3's first cleaning step: ContigGraph::deleteTipsAndClean on the build ----
 * The first step of ContigGraph::cleanGraph (src/ContigGraph.cpp:211-215) on the graph fgpu_raw_plan makes, and printContigs behind it.
 * Three layers, each callable alone.
 *
 * fgpu_tips_plan -- host only, no device, no text, no coverage list: WHICH piece lists the step leaves.  The graph is fgpu_raw_plan's, nodeMap
 * a real std::unordered_map that took the same inserts, so that the two loops go over it in the reference's order and erase as they go
 * (it = nodeMap.erase(it); nothing is inserted).  A contig is an ordered list of fgpu_join_piece; its length is the sum of the pieces' len
 * minus (pieces - 1) k.
 *   deleteTipsAndClean (:168-175): deleteTips, then validateNoneCollapsible only if deleteTips counted a tip; returns whether it did.
 *   deleteTips (:575-615), per node: for i = 0..3, a contigs[i] that isTip while numPathsOut() > 1 (tested anew at every i) goes through
 *     cutPath and deleteContig and is counted; a contigs[4] that isTip likewise, NOT counted; then isCollapsible -> collapseNode and the node
 *     is erased, else testAndCutIfDegenerate -> the node is erased.
 *   isTip (:324-330): fewer bases than read_length (size_t < int: the int goes to unsigned) and no node at the other end, or this node.
 *   numPathsOut (src/ContigNode.cpp:217-225) counts coverages, of which a node has four: breakPath(4) (:280-283) clears contigs[4] only.
 *   cutPath (:364-384): the contig forgets the node on the side Contig::getSide(node, index) names and the node breaks the path; a contig
 *     whose two ends are the same node forgets both and the node breaks both paths.  deleteContig (:346-361) breaks what is left.
 *   isCollapsible (:617-640): one path out, a back, a front (the FIRST contigs[0..3] that is set), neither with both ends on one node.
 *   collapseNode (:1418-1467): back and the LAST contigs[0..3] that is set become back->concatenate(front, backSide, frontSide)
 *     (src/Contig.cpp:83-109: back reversed if its side is 1, front if its side is 2 -- the list reversed, every flip toggled --, then the
 *     lists appended; ends and indices are node1_p, ind1 of the oriented left and node2_p, ind2 of the oriented right, and setEnds
 *     (:123-133) writes the result into those nodes' slots); with no node at either end the result becomes an isolated contig.
 *   testAndCutIfDegenerate (:403-425): no path out -> cutPath(4); no back -> cutPath of every front.  It leaves contigs hanging on one node,
 *     or on none: those are in no node's slot, are not isolated contigs, and are never printed.
 *   validateNoneCollapsible (:709-736), per node: no path out and no back -> erased; isCollapsible -> collapseNode, erased;
 *     testAndCutIfDegenerate -> erased.
 * Then printContigs' two passes as fgpu_raw_plan walks them, the < 250 and >= read_length tests on joined lengths; a bubble record is the
 * back's list as getNewConcatenatedContig (:1509-1530) orients it followed by the extension's.
 * Outputs go into the arrays an fgpu_tips_out names; each n_* says how many entries are needed, whatever the room:
 *   nodes       the nodes left, in map order: key, four coverages, per slot the number of a record of `contigs` or -1
 *   contigs     the contigs in some node's slot (in order of first appearance), then the isolated ones in the list's order; contig c's list is
 *               pieces[list_first[c] .. list_first[c + 1]): a CSR in fgpu_stage3_join's input form over the calls of the build
 *   print       the records of the file in file order: print_pieces[print_first[r] .. print_first[r + 1]), print_number[r]
 * Returns FGPU_PLAN_OK; FGPU_PLAN_UNSET wherever the reference would read or write through a pointer nobody set or that points to a node
 * or contig that is gone (nothing is guessed); FGPU_PLAN_INPUT as fgpu_raw_plan; FGPU_PLAN_SHORT: an array has too little room (the n_*
 * say how much is needed; nothing written is to be used).  With FGPU_PLAN_OK and FGPU_PLAN_SHORT `info` is filled.
 *
 * fgpu_stage3_fasta_joined -- the device: orient and print n strings that are joined already.  Record i is joined[i].len bases from word
 * joined[i].text_word of the text (dist_first, cov_first, cov_sum, n_dist, n_cov are not read) and is numbered numbers[i].  text_host ==
 * NULL: the text is the joined text of the last fgpu_stage3_join whose results are still on the device, read where it lies
 * (FGPU_ERR_STATE if there is none) -- it is in the layout the printing kernels read, so nothing is copied; it is neither freed nor
 * changed.  text_host != NULL: text_words words are uploaded first.  FGPU_ERR_ARG with nothing launched and earlier results untouched: a
 * record that reaches past the text, a record of no bases or of 2^31 and more, n of 2^32 and more.  The file is fgpu_stage3_fasta's, record
 * for record (canon_contig, ">Contig<number>"), and fgpu_stage3_fasta_take takes it; a file that was not taken is dropped.
 *
 * fgpu_stage3_detip -- all of it on a finished build that has not been taken and whose status is 0 (fgpu_stage3_raw_contigs'
 * preconditions and messages): only the two record arrays of the build come to the host; fgpu_tips_plan; fgpu_stage3_join of the print
 * records' lists over the build where it lies; fgpu_stage3_fasta_joined of the joined text where it lies.  A plan status other than
 * FGPU_PLAN_OK is FGPU_ERR_STATE with a message.  THE CALL DROPS join results and a file that were not taken before it.  Afterwards
 * fgpu_stage3_fasta_take gives the file (what printContigs writes after the first deleteTipsAndClean), fgpu_stage3_join_take the print
 * records' strings, distances and coverages, fgpu_stage3_build_take the build, unchanged, and fgpu_stage3_graph_take the graph left.
 *
 * fgpu_stage3_graph_take -- copies the graph of the last fgpu_stage3_detip into the arrays `out` names (nodes, contigs, list_first,
 * pieces and their caps; the print fields are not read) and forgets it; n_nodes, n_contigs, n_pieces are set whatever the room, and an
 * array that is too small is FGPU_ERR_ARG: nothing is copied and the graph is still there (so caps of 0 ask for the sizes).
 * FGPU_ERR_STATE if there is none.  list_first / pieces are valid input to fgpu_stage3_join on the same build: that is how a caller gets the
 * sequences, distances, coverages and cov_sum of the cleaned graph's contigs for the next cleaning step. */
typedef struct {
    uint64_t key;
    uint8_t  cov[4];
    int32_t  slot[5];        /* record of fgpu_tips_out.contigs in contigs[0..4], -1: none */
} fgpu_tips_node;
typedef struct {
    uint64_t node1, node2;   /* node1_p, node2_p as keys of nodeMap (has1 / has2 = 0: nullptr) */
    uint32_t len;            /* joined bases */
    uint8_t  has1, has2;
    uint8_t  ind1, ind2;
    uint8_t  isolated;       /* 1: an entry of isolated_contigs, in no node's slot */
    uint8_t  reserved[7];
} fgpu_tips_contig;
typedef struct {
    fgpu_tips_node*   nodes;        uint64_t nodes_cap, n_nodes;
    fgpu_tips_contig* contigs;      uint64_t* list_first;  /* contigs_cap + 1 entries */  uint64_t contigs_cap, n_contigs;
    fgpu_join_piece*  pieces;       uint64_t pieces_cap, n_pieces;
    uint64_t*         print_first;  /* print_cap + 1 entries */  uint32_t* print_number;  uint64_t print_cap, n_print;
    fgpu_join_piece*  print_pieces; uint64_t print_pieces_cap, n_print_pieces;
} fgpu_tips_out;
typedef struct {
    uint64_t nodes_before;      /* entries of nodeMap before the step */
    uint64_t tips;              /* what deleteTips returns */
    uint64_t back_tips;         /* contigs[4] tips deleted, which it does not count */
    uint64_t collapsed[2];      /* nodes collapseNode took out in deleteTips, in validateNoneCollapsible */
    uint64_t degenerate[2];     /* nodes erased otherwise in the two loops */
    uint32_t validated;         /* 1: validateNoneCollapsible ran */
    uint32_t changed;           /* what deleteTipsAndClean returns */
    fgpu_raw_info print;        /* the records of the file; nodes = the nodes left */
} fgpu_tips_info;
int fgpu_tips_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                   uint64_t n_calls, int32_t k, int32_t read_length, fgpu_tips_out* out, fgpu_tips_info* info);
int fgpu_stage3_fasta_joined(fgpu_ctx* ctx, const fgpu_joined* joined_host, const uint32_t* numbers_host, uint64_t n, const uint64_t* text_host,
                             uint64_t text_words, uint64_t* bytes);
int fgpu_stage3_detip(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_tips_info* info);
int fgpu_stage3_graph_take(fgpu_ctx* ctx, fgpu_tips_out* out);

/* ---- Stage 3's second cleaning step: ContigGraph::removeChimerasAndClean on the detipped graph ----
 * The second step of ContigGraph::cleanGraph (src/ContigGraph.cpp:218-220), on the graph the first one left -- the SAME graph object
 * (faucet_amd/csrc/clean_graph.h): nothing is made again between the steps -- and printContigs behind it.  The first step whose decisions read
 * coverages: Contig::getAvgCoverage of a node's two extreme extensions and of its far node's, each the sum / n of an fgpu_cov_summary that
 * collapseNode folds as it folds the piece lists (the section on coverage summaries above).
 *   removeChimerasAndClean (:177-184): removeChimericExtensions(150), then validateNoneCollapsible only if it counted one; returns whether.
 *   removeChimericExtensions (:642-707), per node in map order:
 *     more than one path out: (P, Q) = getMinMaxForwardExtensions(node, "coverage") (:295-320: over getIndicesOut(), the indices with cov > 0
 *       in order, the contig of the FIRST smallest and the LAST largest average -- std::minmax_element).  far = P->otherEndNode(node); the node
 *       is left alone if far is null or the node itself, if far->indexOf(P) == 4 or if far has fewer than two paths out.  (P2, Q2) likewise
 *       at far; ratio1 = avg(Q) / avg(P), ratio2 = avg(Q2) / avg(P2), in double, a zero average following IEEE.  If P has fewer than 150
 *       bases, ratio1 >= 3 and P == P2: ratio1 > ratio2 -> cutPath(node, indexOf(P)); ratio2 > ratio1 -> cutPath(far, indexOf(P)); otherwise
 *       both and deleteContig(P).  Then isCollapsible(node) -> collapseNode, the node erased.  Counted.
 *     at most one path out: isCollapsible -> collapseNode, the node erased.
 * fgpu_chimera_plan -- host only, no device: from the build (fgpu_tips_plan's arguments and cov_calls, one fgpu_cov_summary per call:
 * fgpu_stage3_cov_calls' output) the graph, deleteTipsAndClean, removeChimerasAndClean, and printContigs' two passes.  `out` is filled as
 * fgpu_tips_plan fills it, with the graph left and the print records after the second step; tips_info (may be NULL) is the first step's
 * account without its print part.  Statuses are fgpu_tips_plan's; a call with a summary of no entries is FGPU_PLAN_INPUT; a covered slot
 * without a contig, or an indexOf that throws, is FGPU_PLAN_UNSET.
 * fgpu_stage3_dechimera -- the step on the LIVE graph of the last fgpu_stage3_detip (FGPU_ERR_STATE with a message if there is none, if its
 * graph has been taken, or if the step has run on it already): fgpu_stage3_cov_calls on the build where it lies; the summaries folded into the
 * live contigs; removeChimerasAndClean; fgpu_stage3_join of the print records; fgpu_stage3_fasta_joined of the joined text where it lies.
 * Join results and a file that were not taken before it are dropped.  Afterwards fgpu_stage3_fasta_take gives the file (printContigs after the
 * two steps), fgpu_stage3_join_take the records' strings, distances and coverages, fgpu_stage3_graph_take the graph after the step and
 * fgpu_stage3_build_take the build, unchanged.  A plan status other than FGPU_PLAN_OK is FGPU_ERR_STATE with a message. */
#define FGPU_CHIMERA_SKIP_NO_FAR    0   /* P has no far node, or it is the node itself */
#define FGPU_CHIMERA_SKIP_BACK      1   /* P sits in the far node's slot 4 */
#define FGPU_CHIMERA_SKIP_FAR_PATHS 2   /* the far node has fewer than two paths out */
#define FGPU_CHIMERA_SKIP_LONG      3   /* P has 150 bases or more */
#define FGPU_CHIMERA_SKIP_RATIO     4   /* ... is short, and ratio1 is below 3 (or no number) */
#define FGPU_CHIMERA_SKIP_OTHER_P   5   /* ... and ratio1 is 3 or more, but P is not the far node's lowest extension */
typedef struct {
    uint64_t nodes_before;         /* entries of nodeMap before the step */
    uint64_t removed;              /* what removeChimericExtensions returns */
    uint64_t cut_near, cut_far, cut_both;   /* ... by outcome: cut at the node, at the far node, at both and P deleted */
    uint64_t collapsed[2];         /* nodes collapseNode took out in the loop, in validateNoneCollapsible */
    uint64_t degenerate[2];        /* nodes erased otherwise (the loop erases none) */
    uint64_t collapsed_after_cut;  /* ... of collapsed[0]: right behind a cut at the same node; the rest had one path out when the loop came to them */
    uint64_t skipped[6];           /* nodes with more than one path out that were left alone, by FGPU_CHIMERA_SKIP_* */
    uint32_t validated;            /* 1: validateNoneCollapsible ran */
    uint32_t changed;              /* what removeChimerasAndClean returns */
    fgpu_raw_info print;           /* the records of the file; nodes = the nodes left */
} fgpu_chimera_info;
int fgpu_chimera_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                      uint64_t n_calls, const struct fgpu_cov_summary* cov_calls, int32_t k, int32_t read_length, fgpu_tips_out* out,
                      fgpu_tips_info* tips_info, fgpu_chimera_info* info);
int fgpu_stage3_dechimera(fgpu_ctx* ctx, uint64_t* bytes, fgpu_chimera_info* info);

/* ---- Stage 3's graph as FASTG: ContigGraph::printGraph on the device ----
 * The other half of what the reference ends with (src/Faucet.cpp:325-326, and commented out behind the build, :313-314): who is connected to
 * whom, which printContigs' files cannot say (they fold bubbles and canonicalise).  ContigGraph::printGraph (src/ContigGraph.cpp:1470-1503)
 * writes four lines per contig -- getFastGHeader(true), getSeq(), getFastGHeader(false), revcomp_string(getSeq()): the PRIMED header goes
 * with the forward sequence, and nothing is canonicalised.
 *   which contigs  ContigIterator (src/ContigIterator.cpp) over nodeMap in the container's order and contigs[0..4]: a contig with a null end
 *     wherever it is met; one whose ends are the same node at the slot getMinIndex() names; any other where Contig::getSide(node, index) is 1.
 *     Then isolated_contigs in list order, those of at least read_length bases (size_t >= int).
 *   name    Contig::getFastGName (src/Contig.cpp:378-385): NODE_<this>_length_<bases>_cov_<getAvgCoverage()>, and ' when RC.  <this> is a heap
 *     address there; here it is 0x and the contig's index in the live graph's contig array in hexadecimal: unique, unchanged for a contig
 *     that survives a step (the files of one run can be laid side by side), and of the reference's shape.  The coverage goes through
 *     operator<< of a double, which is printf's %g: six significant digits of (double) sum / (double) n, trailing zeros stripped, exponent
 *     form below 1e-4, glibc's digit for digit (faucet_amd/csrc/fastg_name.h: integers only, shared by the kernel and the host).
 *   header  getFastGHeader (:387-411): '>' name, then ';' without neighbours, else ':' and the neighbours' names joined by ',' and closed by
 *     ';'.  The neighbours of the header with RC = false are node2_p->getFastGNeighbors(ind2), those of the primed one
 *     node1_p->getFastGNeighbors(ind1) (src/ContigNode.cpp:179-202: index 4 gives the set slots 0..3 in order, any other index slot 4 if
 *     set); a neighbour is primed iff its getSide(thatNode, slot) is 2 -- under BOTH headers: the flag is not inverted for the primed one.
 *
 * fgpu_stage3_fastg -- the device: print n records that are joined already, over a text in fgpu_stage3_join's layout.  Record i is
 * recs[i].len bases from word recs[i].text_word; its headers' neighbours are nbr[nbr_first[2i] .. nbr_first[2i + 1]) (primed header, first
 * line) and nbr[nbr_first[2i + 1] .. nbr_first[2i + 2]), each entry a record's index, | FGPU_FASTG_PRIMED for a primed name.  text_host ==
 * NULL: the joined text of the last fgpu_stage3_join whose results are still on the device, read where it lies (FGPU_ERR_STATE if there is
 * none); text_host != NULL: text_words words are uploaded first.  FGPU_ERR_ARG with a message, nothing launched and earlier results
 * untouched: a record that reaches past the text, a record of no bases or of 2^31 and more, a summary of no entries or with sum > 255 n,
 * n of 2^31 and more, a neighbour CSR that is not one (nbr_first[0] != 0, descending, more than four entries in a list, nbr_first[2n] !=
 * n_nbr), a neighbour index >= n.  Three kernels (faucet_amd/csrc/stage3_fastg.hip): the names, one lane per record; the sizes, scanned by
 * rocPRIM; the text by tiles of FGPU_FASTG_TILE bytes of OUTPUT, the second strand read from the same 2-bit string.  The file stays on the
 * device, *bytes says how long it is (0 for n == 0), and fgpu_stage3_fasta_take takes it: it is THE file slot of the context, so a file that
 * was not taken before the call is dropped, as every Stage-3 call drops it.
 *
 * fgpu_stage3_raw_graph -- <prefix>.raw_graph.fastg (src/Faucet.cpp:313) on a finished build that has not been taken and whose status is 0
 * (fgpu_stage3_raw_contigs' preconditions and messages): the graph is made with fgpu_stage3_cov_calls' summaries, walked (a plan status
 * other than FGPU_PLAN_OK is FGPU_ERR_STATE with a message), the records' piece lists joined by fgpu_stage3_join over the build where it
 * lies, and printed.  The build is left as it was found, and so is a live graph.  Join results and a file that were not taken before the
 * call are dropped.
 *
 * fgpu_stage3_graph_fastg -- the same of the LIVE graph of the last fgpu_stage3_detip or fgpu_stage3_dechimera: FGPU_ERR_STATE with a
 * message if there is none, if it was taken, or if its build is gone.  A graph that has no summaries yet is given them (what
 * fgpu_stage3_dechimera would give it); nothing else of it changes: an fgpu_stage3_dechimera behind the call behaves as if it had not been
 * made, and the call may be made again.  Join results and a file that were not taken before the call are dropped.
 *
 * info: printGraph's counts -- "printed %d node-connected unitigs" is node_records, "printed %d isolated contigs" is isolated_listed, the size
 * of the whole list, not the number printed. */
#define FGPU_FASTG_PRIMED 0x80000000u
#define FGPU_FASTG_TILE   4096          /* bytes of output per workgroup of the text kernel */
typedef struct {
    uint64_t tig;          /* <this>: printed as 0x and hexadecimal */
    uint64_t text_word;    /* first word of the record's 2-bit string in the text */
    uint64_t cov_sum;      /* getAvgCoverage = (double) cov_sum / (double) cov_n */
    uint32_t len;          /* bases */
    uint32_t cov_n;
} fgpu_fastg_rec;
typedef struct {
    uint64_t node_records;      /* records ContigIterator gave */
    uint64_t isolated_printed;  /* isolated contigs of at least read_length bases */
    uint64_t isolated_listed;   /* entries of isolated_contigs */
    uint64_t nodes;             /* entries of nodeMap */
} fgpu_fastg_info;
int fgpu_stage3_fastg(fgpu_ctx* ctx, const fgpu_fastg_rec* recs, uint64_t n, const uint64_t* nbr_first, const uint32_t* nbr, uint64_t n_nbr,
                      const uint64_t* text_host, uint64_t text_words, uint64_t* bytes);
int fgpu_stage3_raw_graph(fgpu_ctx* ctx, int32_t read_length, uint64_t* bytes, fgpu_fastg_info* info);
int fgpu_stage3_graph_fastg(fgpu_ctx* ctx, uint64_t* bytes, fgpu_fastg_info* info);
/* The last fgpu_stage3_raw_graph / fgpu_stage3_graph_fastg of the context by parts, host clock, ms (measurement; 0 for a part the call did not
 * have): [0] the build's record arrays and the map to the host, [1] the summaries (fgpu_stage3_cov_calls, and folding them into a live graph),
 * [2] the graph made of the build, [3] the walk (CleanGraph::fastg_records), [4] the records' lists and fgpu_stage3_join, [5] fgpu_stage3_fastg:
 * its checks, the records' way to the device, the three kernels. */
int fgpu_diag_fastg_times(fgpu_ctx* ctx, double ms[6]);

/* ---- profiling --------------------------------------------------------------------------------- */
typedef struct {
    char     name[48];
    uint64_t launches;
    double   total_ms;       /* sum of HIP-event durations on the context's stream */
} fgpu_kernel_time;
/* Requires FGPU_FLAG_PROFILE.  Returns the number of distinct kernels; fills up to cap entries. */
int fgpu_kernel_times(fgpu_ctx* ctx, fgpu_kernel_time* out, int cap);
int fgpu_kernel_times_reset(fgpu_ctx* ctx);
/* Switch the event bracketing on or off between passes (what FGPU_FLAG_PROFILE sets at creation): the events cost 1.5 % of a step
 * (profiles/r04_profile_flag_ab.txt), so a caller times its steps without them and takes kernel times from separate, bracketed steps. */
int fgpu_profile_enable(fgpu_ctx* ctx, int on);

/* ---- measured ceilings (no reference counterpart) ---------------------------------
 * Streaming device-to-device copy of `bytes` (read + write counted), GB/s. */
int fgpu_diag_stream_copy(fgpu_ctx* ctx, uint64_t bytes, int iters, double* gb_per_s);
/* n_access independent random 32-bit accesses into a table of table_bytes (power of two) per iteration.
 * mode 0 = load, 1 = atomicMin (the load pass' first-set times), 2 = test-then-atomicOr (Bloom::add). */
/* NS1 as a whole probe CHAIN (round 3): n_items x Bloom::contains (n_hash dependent bit tests, early exit) directly, and with the first
 * level binned by filter slice and the survivors handed back as a dense list (faucet_amd/csrc/diag.hip).  Times per pass in ms; *equal = 1 iff
 * both forms give the same answers bit for bit (n_hash 2..8: with one hash function there is no chain).  Diagnostic: nothing of the path calls it. */
int fgpu_diag_binned_chain(fgpu_ctx* ctx, uint64_t table_bytes, uint64_t n_items, uint64_t slice_bytes, int n_hash, int fill_byte, int iters,
                           double* direct_ms, double* bin_ms, double* first_ms, double* rest_ms, double* survivors_share, int* equal);
/* Per-piece records of the key-ordered walk (measurement builds with -DFGPU_KO_TRACE; *n = 0 otherwise): 4 words per walked piece --
 * global piece number, start and end in 10 ns ticks, ticks waited for turns | lk positions << 48.  scripts/ko_trace.py reads them. */
int fgpu_diag_ko_trace(fgpu_ctx* ctx, uint64_t* out, uint64_t cap_records, uint64_t* n);
int fgpu_diag_ko_stamps(fgpu_ctx* ctx, uint64_t* out, uint64_t cap_words, uint64_t* n_pieces);   /* per-step stamps of one piece in 16 (-DFGPU_KO_TRACE) */
int fgpu_diag_random_access(fgpu_ctx* ctx, uint64_t table_bytes, uint64_t n_access, int mode, int iters, double* access_per_s);
/* The two access patterns of the marking kernel on the context's own tables of the last load pass (pair layout): random loads from the interleaved
 * filter words, random atomicMin into the first-set times; accesses per second; and both together as the kernel mixes them (three loads per item, three
 * atomics for six items in ten; items per second, may be NULL).  Between passes (the tables are rewritten by the next load). */
int fgpu_diag_load_tables(fgpu_ctx* ctx, uint64_t n_access, double* pair_loads_per_s, double* first_atomics_per_s, double* mixed_items_per_s);
/* The mixed pattern with k other allocations of the filter pair (held at once, then freed) against the context's first-set times: does the pair's place
 * decide the marking kernel's speed?  items_per_s[k].  Measurement (scripts/kinds_probe.py). */
int fgpu_diag_pair_placements(fgpu_ctx* ctx, int k, uint64_t n_items, double* items_per_s);
/* NS1's query-side blocking, measured: n_probes single-bit probes at pseudo-random positions of a table of table_bytes (power of two, <= 512 MiB),
 * once directly (one random load each, what the path's kernels do) and once binned by slice of slice_bytes (LDS-staged buckets per 4096 probes,
 * one queue per slice, slices probed by the workgroups of the XCD whose L2 then holds them).  Rates in probes/s; the binned one covers both of
 * its kernels, whose mean times come back separately. */
int fgpu_diag_binned_probes(fgpu_ctx* ctx, uint64_t table_bytes, uint64_t n_probes, uint64_t slice_bytes, int iters, double* direct_per_s,
                            double* binned_per_s, double* bin_ms, double* probe_ms);
/* How often the library has scanned a pass's batches again by itself (lazy junction tests, see fgpu_scan_batch) since the context was made. */
/* Kept for the ABI: the out-of-order walk of large clusters whose probed pieces this counted by outcome is retired (measured: it did not pay);
 * out[0..3] = 0. */
int fgpu_diag_walk_probe(fgpu_ctx* ctx, uint64_t out[4]);
int fgpu_diag_scan_replays(fgpu_ctx* ctx, uint64_t* replays);
/* How often the host thread has waited for the device (hipStreamSynchronize / hipEventSynchronize inside the library) since the current or last pass
 * began (fgpu_load_begin / fgpu_scan_begin), and for how long in all (ms, may be NULL).  Every wait is also a chance for a busy host to schedule the
 * thread late: what a pass costs beside other tenants of the box grows with this count, not with the device's work. */
int fgpu_diag_host_waits(fgpu_ctx* ctx, uint64_t* waits, double* ms);
/* after fgpu_scan_end: [0] junction tests the walk had to run itself (the preview had left the position out) that came out TRUE at a
 * k-mer no piece of the window had registered -- the walk goes on and the window is checked afterwards --, [1] of those, the ones whose
 * k-mer was then found on another piece of the same window: only these void a lazy scan (the library scans its journal again, see above),
 * [2] noted positions the check itself passed over (= [0] when it works: a self-test of the sweep). */
int fgpu_diag_late_flags(fgpu_ctx* ctx, uint64_t out[3]);
/* after a scan with the long pair filter on the device: [0] items (first-end k-mers of read pairs with two non-empty lists), [1] of those, found
 * paired against the filter as their batch found it, [2] addPair calls, [3] evaluation rounds over all batches, [4] most rounds one batch
 * needed, [5] batches */
int fgpu_diag_long_pairs(fgpu_ctx* ctx, uint64_t out[6]);
/* after fgpu_scan_long_pairs: the form of the filter's first-set times.  [0] 0 no filter on the device, 1 dense, 2 sparse, [1] bytes of working
 * state the filter holds beyond its tai / 8 bytes of bits, [2] sparse: most slots a batch's table had in the last scan (a power of two),
 * [3] sparse: the internal-error flag (a table that ran full or missed a key; fgpu_scan_end then answers FGPU_ERR_STATE) */
int fgpu_diag_long_pairs_state(fgpu_ctx* ctx, uint64_t out[4]);
/* after fgpu_scan_end: the optimistic walk of large clusters: [0] pieces it walked, [1] rounds it ran, [2] windows it settled,
 * [3] windows it left to the key-ordered walk (rounds that did not settle, full tables), [4] piece-rounds in which a piece kept its log (no
 * earlier piece had changed what it reads), [5] windows whose large clusters outgrew the tables of both walks (walked by cluster) */
int fgpu_diag_ovw(fgpu_ctx* ctx, uint64_t out[6]);
/* ... and how full its event tables got: *high_water = the most entries a round of any window of the scan held, *capacity = entries per table as
 * they stand.  The library grows the tables (x 2 up to 2^27 entries, 32 bytes each) once a round has filled a quarter, so that coverage of many
 * hundred-fold inside repeats does not first overflow them (exact either way: an overflowing window goes to the key-ordered walk, slowly).
 * FGPU_OVW_EV_LOG2 = log2 of the entries a context starts with (default 23). */
int fgpu_diag_ovw_tables(fgpu_ctx* ctx, uint64_t* high_water, uint64_t* capacity);
/* Where the last load pass settled its occurrences (measurement: which kernel performs the reference's bloo2 sets): *in_mark = occurrences
 * whose bits were all in the carried-in state and that the marking kernel itself routed to bloo2, *pending = occurrences left to the
 * first-set-time resolution.  Valid after fgpu_load_end, until the next pass begins. */
int fgpu_diag_load_split(fgpu_ctx* ctx, uint64_t* in_mark, uint64_t* pending);
/* Memory clock (kHz), bus width (bits), L2 bytes and CU count as the HIP runtime reports them. */
int fgpu_diag_device_attr(fgpu_ctx* ctx, int32_t* mem_clock_khz, int32_t* mem_bus_bits, int32_t* l2_bytes, int32_t* compute_units);

#ifdef __cplusplus
}
#endif
#endif /* FAUCET_GPU_H */
