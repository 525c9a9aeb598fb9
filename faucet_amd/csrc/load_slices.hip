// load_slices.hip — pass 1 by FILTER SLICES: one rank, the WHOLE stream, a slice [lo, lo + n) of the filter's bit
// positions.  Kernels, stages and the fgpu_load_slice_* entry points; the view of the slice, Bloom::add on it and --mercy's state machine are
// the plain pass' (load_common.h).
//
// "Bit b was first set at time t" is a property of bit b alone (the min over all occurrences that hash to it), so the rank that owns b finds it
// from the stream without the other slices.  What it cannot decide alone is the routing of an occurrence -- that needs ALL of its bits -- so the
// pass writes, per stream position, "one of MY bits of this occurrence was not set before it" (the fail plane); the OR of the ranks' planes is the
// sequential run's decision, and k_slice_commit sets the own bloo2 bits of the occurrences nobody failed.  The working state is sized by the
// slice (load_common.h, Slice).
#include <algorithm>
#include <string>

#include "fgpu_ctx.h"
#include "fgpu_flags.h"
#include "load_common.h"

namespace {

// k_load_mark on a slice: the carry words of the own positions; an occurrence without an own bit touches no memory
__global__ void __launch_bounds__(256) k_slice_mark(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T, uint64_t n_words,
                                                    FdParams fp, Slice s, uint32_t tb, uint64_t* __restrict__ pending, uint64_t plane_stride,
                                                    uint64_t* __restrict__ fail, DevCounters* cnt) {
    unsigned long long n_ok = 0, n_pend = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const bool ok = p < T && fd_window_ok(bad, p, fp.k);
        uint32_t missing = 0;
        if (ok) {
            n_ok++;
            uint64_t hA, hB;
            fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
            missing = filt_missing<0>(s, hA, hB, fp);
            if (missing) {
                n_pend++;
                fd_each_bit(hA, hB, fp, [&](int i, uint64_t h) {
                    if (missing & (1u << i)) atomicMin(s.time(h), tb + (uint32_t)p);
                    return true;
                });
            }
        }
        const uint64_t pm = __ballot(missing != 0);
        uint64_t mm[MISS_PLANES];
#pragma unroll
        for (int i = 0; i < MISS_PLANES; i++) mm[i] = __ballot((missing >> i) & 1u);
        if (fd_lane() == 0) {
            pending[p >> 6] = pm;
            fail[p >> 6] = 0;        // k_slice_resolve fills in the words that have pending occurrences
            if (pm) {
#pragma unroll
                for (int i = 0; i < MISS_PLANES; i++) pending[(i + 1) * plane_stride + (p >> 6)] = mm[i];
            }
        }
    }
    block_add(&cnt->kmers, n_ok);
    block_add(&cnt->mark_pending, n_pend);
}

// own bits that were missing from the carry: set before the occurrence iff first[bit] < its time.  One that was not -> the fail bit.
__global__ void __launch_bounds__(256) k_slice_resolve(const uint64_t* __restrict__ codes, uint64_t n_words, FdParams fp, Slice s, uint32_t tb,
                                                       const uint64_t* __restrict__ pending, uint64_t plane_stride, uint64_t* __restrict__ fail) {
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pw = pending[p >> 6];   // wave-uniform: the 64 lanes of a wave cover one word
        if (!pw) continue;
        bool failed = false;
        if ((pw >> (p & 63)) & 1ULL) {
            uint32_t missing = 0;
#pragma unroll
            for (int i = 0; i < MISS_PLANES; i++)
                missing |= (uint32_t)((pending[(i + 1) * plane_stride + (p >> 6)] >> (p & 63)) & 1ULL) << i;
            uint64_t hA, hB;
            fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
            fd_each_bit(hA, hB, fp, [&](int i, uint64_t h) {
                // hash functions beyond the planes are tested against the carry again (it does not change between the two kernels)
                const bool was_missing = i < MISS_PLANES ? ((missing >> i) & 1u) != 0 : s.owns(h) && !((s.word(h)[0] >> (h & 31)) & 1u);
                if (was_missing && !(*s.time(h) < tb + (uint32_t)p)) failed = true;
                return !failed;
            });
        }
        const uint64_t fm = __ballot(failed);
        if (fd_lane() == 0) fail[p >> 6] = fm;
    }
}

// carry |= own bits of the batch's occurrences (the re-hashing alternative to a sweep of the slice's first[], see k_carry_set).  Every valid
// occurrence leaves all of its bits set in bloo1, and the ones whose own bits were all in the carry already are not pending: only those are hashed.
// (k_carry_set's body on another view, not k_carry_set itself: that one takes "valid and not routed to bloo2" from `bad` and `sure`, and a
// slice has no `sure` plane before the ranks' planes have been ORed -- its selection is the pending plane.)
__global__ void __launch_bounds__(256) k_slice_carry_set(const uint64_t* __restrict__ codes, uint64_t n_words, FdParams fp, Slice s,
                                                         const uint64_t* __restrict__ pending, uint64_t plane_stride) {
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t pw = pending[p >> 6];
        if (!((pw >> (p & 63)) & 1ULL)) continue;
        filt_set_window<0>(s, codes, p, fp);
    }
}

// After the ranks' fail planes have been ORed in place: a valid window whose fail bit is 0 is an occurrence the sequential run routes to bloo2.
// Its OWN bits are set here; `sure` = valid & ~fail is the global routing decision (what the scan of the same reads reuses), and the count is the
// global one -- the same on every rank.
__global__ void __launch_bounds__(256) k_slice_commit(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T, uint64_t n_words,
                                                      FdParams fp, Slice s, const uint64_t* __restrict__ fail, uint64_t* __restrict__ sure,
                                                      DevCounters* cnt) {
    unsigned long long n_go = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        const bool go = p < T && fd_window_ok(bad, p, fp.k) && !((fail[p >> 6] >> (p & 63)) & 1ULL);
        if (go) {
            n_go++;
            uint64_t hA, hB;
            fd_hash_pair(fd_canon(fd_kmer_at(codes, p, fp.k), fp.k), fp.tai_mask, hA, hB);
            const uint32_t b2_missing = filt_missing<1>(s, hA, hB, fp);
            if (b2_missing) filt_set<1, false>(s, hA, hB, fp, b2_missing);
        }
        const uint64_t sm = __ballot(go);
        if (fd_lane() == 0) sure[p >> 6] = sm;
    }
    block_add(&cnt->to_bloo2, n_go);
}

// ---- --mercy under filter slices -------------------------------------------------------------------------------------
// isJunction asks bloo1, as of occurrence t, about k-mers whose bits lie in any slice.  "Bit b was set by time t" (in the carry, or
// first[b] <= t: bloo1_contains_at) concerns b alone, so its owner answers it, and a candidate is contained iff NO rank finds an own bit of it
// unset: one miss bit per (position, nt) per rank, ORed over the ranks, is "the candidate was not in bloo1".  Which tests the reference makes
// depends on earlier answers; a miss bit where no test is made is never read, so the probe evaluates a superset that follows from `bad` and the
// ORed fail plane alone: every window but the first of its segment that is not contained, or is contained behind one that is not.  The
// direction is the reference's (mercy_each_candidate).  Must run while first[] still answers "<= t" for this batch: before the batch is folded
// into the carry.
__global__ void __launch_bounds__(256) k_slice_mercy_probe(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t T,
                                                           uint64_t n_words, FdParams fp, Slice s, uint32_t tb, const uint64_t* __restrict__ fail,
                                                           uint64_t* __restrict__ miss, uint64_t plane_stride, DevCounters* cnt) {
    unsigned long long n_probed = 0;
    const uint64_t total = n_words * 64;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t missed = 0;
        // not the first window of its segment: position p - 1 is good, so window p - 1 is valid and its fail bit is its routing
        if (p && p < T && fd_window_ok(bad, p, fp.k) && !((bad[(p - 1) >> 6] >> ((p - 1) & 63)) & 1ULL)) {
            const bool contained = !((fail[p >> 6] >> (p & 63)) & 1ULL);
            const bool prev_contained = !((fail[(p - 1) >> 6] >> ((p - 1) & 63)) & 1ULL);
            if (!contained || !prev_contained) {
                n_probed++;
                mercy_each_candidate(codes, p, contained, fp, [&](int nt, uint64_t e) {
                    if (!bloo1_contains_at(s, fd_canon(e, fp.k), tb + (uint32_t)p, fp)) missed |= 1u << nt;
                    return true;
                });
            }
        }
        uint64_t mm[MERCY_NT];
#pragma unroll
        for (int nt = 0; nt < MERCY_NT; nt++) mm[nt] = __ballot((missed >> nt) & 1u);
        if (fd_lane() == 0) {
#pragma unroll
            for (int nt = 0; nt < MERCY_NT; nt++) miss[nt * plane_stride + (p >> 6)] = mm[nt];
        }
    }
    block_add(&cnt->slice_mercy[0], n_probed);
}

// After the ranks' miss planes have been ORed in place and k_slice_commit has written `sure` = valid & ~fail: the state machine of k_load_mercy,
// one thread per 64-position word for the segments that START in it, with isJunction answered as "some nt != real_ext whose ORed miss bit is 0".
// The OWN bloo2 bits of the k-mers of every accepted run are set; the five counts are global ones, the same on every rank.
__global__ void __launch_bounds__(256) k_slice_mercy_commit(const uint64_t* __restrict__ codes, const uint64_t* __restrict__ bad, uint64_t n_words,
                                                            FdParams fp, Slice s, const uint64_t* __restrict__ sure,
                                                            const uint64_t* __restrict__ miss, uint64_t plane_stride, DevCounters* cnt) {
    MercyCounts c;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x)
        fd_each_segment(bad, w, (uint64_t)fp.k, ~0ULL, [&](uint64_t p, uint64_t len) {
            mercy_segment(sure, p, len, fp.k, c,
                          [&](uint64_t pos, bool extend_rc) {
                              bool junction = false;
                              mercy_each_candidate(codes, pos, extend_rc, fp, [&](int nt, uint64_t) {
                                  if (!((miss[nt * plane_stride + (pos >> 6)] >> (pos & 63)) & 1ULL)) junction = true;
                                  return true;
                              });
                              return junction;
                          },
                          [&](uint64_t q) { filt_set_window<1>(s, codes, q, fp); });
        });
    block_add(&cnt->slice_mercy[1], c.hl_junction);
    block_add(&cnt->slice_mercy[2], c.opened);
    block_add(&cnt->slice_mercy[3], c.lh_junction);
    block_add(&cnt->slice_mercy[4], c.added);
    block_add(&cnt->slice_mercy[5], c.kmers);
}

// Read offsets that came from another rank, against the block they are said to belong to, before any scan uses them: sends and receives pair
// up by order, and offsets in the wrong slot would be silently wrong stop lists.  By the format (faucet_gpu.h) read i occupies stream positions
// offs[i] + i .. offs[i + 1] + i - 1 and the separator behind it, position offs[i + 1] + i, is a bad position; offs[0] = 0, the offsets do not
// descend, offs[n] + n = T.  One lane per read; every position is compared with T before the bad plane is read, so garbage reads nothing out
// of bounds (the plane holds ceil(T / 64) + FGPU_PADW words).  A violation: out->failed, and the lowest such batch.
__global__ void __launch_bounds__(256) k_offs_check(const uint64_t* __restrict__ offs, uint64_t n, uint64_t T, const uint64_t* __restrict__ bad,
                                                    uint64_t batch, OffsCheck* out) {
    bool wrong = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = offs[i], b = offs[i + 1];
        if (i == 0 && a != 0) wrong = true;
        if (b < a || b >= T) {             // (b < T: then b + i < 2 T cannot wrap, and n <= T)
            wrong = true;
        } else {
            const uint64_t sep = b + i;    // the separator behind read i
            if (sep >= T || !((bad[sep >> 6] >> (sep & 63)) & 1ULL)) wrong = true;
            if (i == n - 1 && sep + 1 != T) wrong = true;
        }
    }
    if (__ballot(wrong) && fd_lane() == 0) {
        atomicOr(&out->failed, 1ULL);
        atomicMin(&out->batch, (unsigned long long)batch);
    }
}

}  // namespace

// (see fgpu_touch_load)
void fgpu_touch_load_slices() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)k_slice_mark);
}

// ---- the stages ------------------------------------------------------------------------------------------------------------------------
static Slice slice_of(const fgpu_ctx* ctx) { return Slice{ctx->slice_pair, ctx->slice_first, ctx->slice_lo, ctx->slice_n}; }

// The batch joins the carry: by re-hashing its pending occurrences (their planes are still those of the batch in hand) or, once the epoch has
// grown enough, by a sweep.  Right behind mark + resolve in a plain sliced pass, behind the probe in a mercy one.
static int slice_fold_batch(fgpu_ctx* ctx, const void* codes, uint64_t n_words, uint64_t span) {
    if (ctx->carry_by_set)
        FGPU_LAUNCH("slice_carry_update", k_slice_carry_set, fgpu_grid(span, 256), 256, (const uint64_t*)codes, n_words, ctx->fd, slice_of(ctx),
                    (const uint64_t*)ctx->cur->pending.p, n_words + FGPU_PADW);
    return fgpu_epoch_after_batch(ctx, span);
}

// mark + resolve of a packed stream (codes, bad: T positions) against the slice, into the fail plane of resident slot r; the pending planes
// are the scratch of the batch in hand
static int slice_mark_resolve(fgpu_ctx* ctx, const void* codes, const void* bad, uint64_t T, uint64_t n_words, ResidentBatch& r) {
    const uint64_t plane_stride = n_words + FGPU_PADW;
    int rc = fgpu_ensure_b(ctx, &ctx->cur->pending, (MISS_PLANES + 1) * plane_stride * 8);
    if (rc) return rc;
    if ((rc = fgpu_util_count_segments(ctx, bad, n_words, ctx->fd.k))) return rc;
    // times are positions within the epoch, as in fgpu_stage_load: a sweep before the 32-bit clock would wrap
    const uint64_t span = n_words * 64;
    if ((rc = fgpu_epoch_before_batch(ctx, span))) return rc;
    const uint32_t tb = ctx->carry_by_set ? 0u : (uint32_t)ctx->epoch_positions;
    const unsigned grid = fgpu_grid(span, 256);
    const Slice s = slice_of(ctx);
    uint64_t* pending = (uint64_t*)ctx->cur->pending.p;
    uint64_t* fail = (uint64_t*)r.fail.p;
    FGPU_HIP(hipMemsetAsync(fail + n_words, 0, FGPU_PADW * 8, ctx->stream));   // the plane is ORed in 16-byte granules: zero past its last word
    FGPU_LAUNCH("slice_mark", k_slice_mark, grid, 256, (const uint64_t*)codes, (const uint64_t*)bad, T, n_words, ctx->fd, s, tb, pending, plane_stride,
                fail, ctx->counters);
    FGPU_LAUNCH("slice_resolve", k_slice_resolve, grid, 256, (const uint64_t*)codes, n_words, ctx->fd, s, tb, (const uint64_t*)pending, plane_stride, fail);
    if (ctx->slice_mercy) {
        // the fold is left to fgpu_stage_slice_mercy_probe: until then first[] answers "set by time t" for this batch's positions
        ctx->slice_probe_owed = true;
        ctx->slice_owed_span = span;
    } else if ((rc = slice_fold_batch(ctx, codes, n_words, span))) {
        return rc;
    }
    r.T = T;
    r.n_words = n_words;
    r.tb = tb;
    return FGPU_OK;
}

// mark + resolve of one batch against the slice.  The batch is kept in HBM first (codes, bad, its fail plane, room for `sure`): the commit
// needs every batch again once the planes have been ORed across the ranks, so a batch that cannot be kept is an error, not a silent skip.
static int fgpu_stage_slice_load(fgpu_ctx* ctx) {
    BatchBufs& bb = *ctx->cur;
    if (bb.T == 0) return FGPU_OK;
    const uint64_t pb = (bb.n_words + FGPU_PADW) * 8;
    // a mercy pass keeps the four miss planes of the probe too: 9 instead of 5 bits per stream position
    const uint64_t parts[5] = {2 * pb, pb, pb, pb, ctx->slice_mercy ? MERCY_NT * pb : 0};
    ResidentBatch* r;
    uint64_t kept;
    // a pass that keeps its reads: the batch's offsets beside its planes, charged with them
    const uint64_t ob = ctx->keep_reads ? (bb.n_reads + 1) * 8 : 0;
    const bool no_room = ob && ctx->resident_bytes + parts[0] + parts[1] + parts[2] + parts[3] + parts[4] + ob > ctx->resident_budget;
    switch (no_room ? (int)FGPU_TAKE_NO_BUDGET : fgpu_resident_take(ctx, parts, true, &r, &kept)) {
    case FGPU_TAKE_NO_BUDGET:
        ctx->err = "load_slice_batch: the batch" + (ob ? " and its " + std::to_string(ob) + " bytes of read offsets do" : std::string(" does")) +
                   " not fit the budget for resident batches (" + std::to_string(ctx->resident_budget) +
                   " bytes, " + std::to_string(ctx->resident_bytes) + " in use; FGPU_FLAG_NO_RESIDENT sets it to 0): a sliced pass keeps every batch" +
                   (ctx->slice_mercy ? ", under --mercy with four miss planes (9 bits per stream position)" : "");
        return FGPU_ERR_NOMEM;
    case FGPU_TAKE_NO_MEMORY:
        ctx->err = "load_slice_batch: no device memory to keep the batch resident (budget " + std::to_string(ctx->resident_budget) + " bytes): " + ctx->err;
        return FGPU_ERR_NOMEM;
    }
    if (int rc = slice_mark_resolve(ctx, bb.codes.p, bb.bad.p, bb.T, bb.n_words, *r)) return rc;
    FGPU_HIP(hipMemcpyAsync(r->codes.p, bb.codes.p, parts[0], hipMemcpyDeviceToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(r->bad.p, bb.bad.p, pb, hipMemcpyDeviceToDevice, ctx->stream));
    if (ob) {
        if (int rc = fgpu_ensure_b(ctx, &r->offs, ob)) return rc;
        if (int rc = fgpu_offs_keep(ctx, r->offs.p, bb.d_offs, bb.n_reads + 1)) return rc;
        r->n_reads = bb.n_reads;
        ctx->kept_reads_total += bb.n_reads;
        kept += ob;
    }
    ctx->resident_count++;
    ctx->resident_bytes += kept;
    return FGPU_OK;
}

// The same for a packed block (fgpu_load_slice_batch_packed): the block becomes the resident batch's codes / bad -- no copy --, and its
// share of the budget was taken when it was made (fgpu_packed_acquire).  A block that was filled by the caller is checked against its
// trailer first (error flag 64, reported by the pass' next synchronising call).
static int fgpu_stage_slice_load_packed(fgpu_ctx* ctx, PackedBlock* b) {
    const uint64_t plane_stride = b->n_words + FGPU_PADW, pb = plane_stride * 8;
    const uint64_t parts[5] = {0, 0, pb, pb, ctx->slice_mercy ? MERCY_NT * pb : 0};
    int rc;
    if (b->state == 2 && (rc = fgpu_packed_digest(ctx, b, true))) return rc;
    ResidentBatch* r;
    uint64_t kept;
    if (fgpu_resident_take(ctx, parts, false, &r, &kept)) {
        ctx->err = "load_slice_batch_packed: no device memory for the batch's planes (budget " + std::to_string(ctx->resident_budget) + " bytes): " + ctx->err;
        return FGPU_ERR_NOMEM;
    }
    uint64_t* words = (uint64_t*)b->buf.p;
    r->packed_codes = words;
    r->packed_bad = words + 2 * plane_stride;
    if ((rc = slice_mark_resolve(ctx, r->packed_codes, r->packed_bad, b->T, b->n_words, *r))) return rc;
    b->state = 3;
    b->resident_index = ctx->resident_count;
    if (b->offs_state == 1) {      // packed here by a pass that keeps its reads: the offsets go with the batch (a peer's come later, fgpu_load_slice_adopt_reads)
        r->packed_offs = b->offs.p;
        r->n_reads = b->n_reads;
        ctx->kept_reads_total += b->n_reads;
    }
    ctx->resident_count++;
    return FGPU_OK;
}

// The probe of the latest batch of a mercy pass, then the fold that fgpu_stage_slice_load left out.  The batch's fail plane holds the OR over
// the ranks by now (the caller's exchange, ordered before this call).
static int fgpu_stage_slice_mercy_probe(fgpu_ctx* ctx) {
    ResidentBatch& r = *ctx->resident[ctx->resident_count - 1];
    const uint64_t plane_stride = r.n_words + FGPU_PADW;
    uint64_t* miss = (uint64_t*)r.miss.p;
    for (int nt = 0; nt < MERCY_NT; nt++)     // the planes are ORed in 16-byte granules: zero past their last word
        FGPU_HIP(hipMemsetAsync(miss + nt * plane_stride + r.n_words, 0, FGPU_PADW * 8, ctx->stream));
    FGPU_LAUNCH("slice_mercy_probe", k_slice_mercy_probe, fgpu_grid(r.n_words * 64, 256), 256, (const uint64_t*)r.codes_p(), (const uint64_t*)r.bad_p(),
                r.T, r.n_words, ctx->fd, slice_of(ctx), r.tb, (const uint64_t*)r.fail.p, miss, plane_stride, ctx->counters);
    ctx->slice_probe_owed = false;
    return slice_fold_batch(ctx, r.codes_p(), r.n_words, ctx->slice_owed_span);
}

static int fgpu_stage_slice_commit(fgpu_ctx* ctx) {
    const Slice s = slice_of(ctx);
    for (uint64_t i = 0; i < ctx->resident_count; i++) {
        ResidentBatch& r = *ctx->resident[i];
        FGPU_LAUNCH("slice_commit", k_slice_commit, fgpu_grid(r.n_words * 64, 256), 256, (const uint64_t*)r.codes_p(), (const uint64_t*)r.bad_p(), r.T,
                    r.n_words, ctx->fd, s, (const uint64_t*)r.fail.p, (uint64_t*)r.sure.p, ctx->counters);
        if (ctx->slice_mercy)     // the runs between solid k-mers, from the ORed miss planes and the `sure` plane just written
            FGPU_LAUNCH("slice_mercy_commit", k_slice_mercy_commit, fgpu_grid(r.n_words, 256), 256, (const uint64_t*)r.codes_p(),
                        (const uint64_t*)r.bad_p(), r.n_words, ctx->fd, s, (const uint64_t*)r.sure.p, (const uint64_t*)r.miss.p,
                        r.n_words + FGPU_PADW, ctx->counters);
    }
    return FGPU_OK;
}

// the slice's working state: an empty carry, an empty bloo2, every time "never"
static int fgpu_slice_pair_begin(fgpu_ctx* ctx) {
    if (!ctx->slice_n) return FGPU_OK;
    FGPU_HIP(hipMemsetAsync(ctx->slice_pair, 0, ctx->slice_n / 4, ctx->stream));
    FGPU_HIP(hipMemsetAsync(ctx->slice_first, 0xFF, ctx->slice_n * 4, ctx->stream));
    return FGPU_OK;
}

// ---- the entry points: pass 1 by filter slices, the whole stream into one slice of the bit positions -----------------------------------
// What the calls inside a pass ask of its state.  Each implies the ones before it.
enum SliceNeed {
    SLICE_MERCY = -1,  // a sliced pass opened by fgpu_load_slice_mercy_begin is open
    SLICE_OPEN = 0,    // a sliced pass is open
    SLICE_LOADING,     // ... and not committed: it still takes batches
    SLICE_PROBED,      // ... and, under --mercy, its latest batch has been probed: the next one may be marked
    SLICE_COMMIT,      // ... the same two for the commit itself, in its own words
};
static int slice_check(fgpu_ctx* ctx, const char* who, SliceNeed need) {
    const std::string w(who);
    if (need == SLICE_MERCY) {
        if (ctx->phase != 3 || !ctx->slice_mercy) { ctx->err = w + " outside a pass opened by load_slice_mercy_begin"; return FGPU_ERR_STATE; }
        return FGPU_OK;
    }
    if (ctx->phase != 3) { ctx->err = w + " outside load_slice_begin/load_slice_end"; return FGPU_ERR_STATE; }
    if (need >= SLICE_LOADING && ctx->slice_committed) {
        ctx->err = w + (need == SLICE_COMMIT ? " twice in one pass" : " after load_slice_commit: the pass can only be ended");
        return FGPU_ERR_STATE;
    }
    if (need >= SLICE_PROBED && ctx->slice_probe_owed) {
        ctx->err = w + (need == SLICE_COMMIT ? ": the last batch of this mercy pass has not been probed (fgpu_load_slice_mercy_probe)"
                                             : ": the previous batch of this mercy pass has not been probed (fgpu_load_slice_mercy_probe, after its fail plane "
                                               "has been ORed): its first-set times must be read before the next batch is marked");
        return FGPU_ERR_STATE;
    }
    return FGPU_OK;
}

static void packed_describe(const PackedBlock* b, uint64_t n_reads, fgpu_packed* out) {
    out->block_dev = b ? b->buf.p : nullptr;
    out->nbytes = b ? fgpu_packed_bytes(b->n_words) : 0;
    out->T = b ? b->T : 0;
    out->n_reads = n_reads;
}

extern "C" {

// `mercy`: the pass is opened by fgpu_load_slice_mercy_begin (batch, exchange, probe in lockstep; four miss planes per batch)
static int slice_begin(fgpu_ctx* ctx, uint64_t bit_lo, uint64_t bit_hi, bool mercy) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "load_slice_begin while another pass is open"; return FGPU_ERR_STATE; }
    if (!mercy && (ctx->prm.flags & FGPU_FLAG_MERCY)) {
        ctx->err = "load_slice_begin: --mercy needs time-aware membership tests of the other slices' bits: a probe of every batch between its "
                   "exchange and the next batch -- open the pass with fgpu_load_slice_mercy_begin and drive the five-step protocol";
        return FGPU_ERR_STATE;
    }
    if (mercy && !(ctx->prm.flags & FGPU_FLAG_MERCY)) {
        ctx->err = "load_slice_mercy_begin: the context was created without FGPU_FLAG_MERCY (fgpu_load_slice_begin opens the plain sliced pass)";
        return FGPU_ERR_STATE;
    }
    if ((bit_lo & 511) || (bit_hi & 511) || bit_lo > bit_hi || bit_hi > ctx->prm.tai) {
        ctx->err = "load_slice_begin: a slice is [bit_lo, bit_hi) with both bounds multiples of 512, bit_lo <= bit_hi <= tai";
        return FGPU_ERR_ARG;
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (int rc = fgpu_bloom_download_wait(ctx)) return rc;
    // the working state is sized by the SLICE (4 bytes of time + 2 x 1/8 byte of filter per own bit), always in the pair layout
    const uint64_t n = bit_hi - bit_lo, fbytes = n * 4, pbytes = n / 4;
    if (ctx->slice_first_bytes < fbytes || ctx->slice_pair_bytes < pbytes) {
        FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        if (ctx->slice_first) (void)hipFree(ctx->slice_first);
        if (ctx->slice_pair) (void)hipFree(ctx->slice_pair);
        ctx->slice_first = nullptr;
        ctx->slice_pair = nullptr;
        ctx->slice_first_bytes = ctx->slice_pair_bytes = 0;
        hipError_t e = hipMalloc(&ctx->slice_first, fbytes);
        if (e == hipSuccess) e = hipMalloc(&ctx->slice_pair, pbytes);
        if (e != hipSuccess) {
            ctx->err = std::string("hipMalloc of the slice state (4.25 bytes per own filter bit) failed: ") + hipGetErrorString(e);
            if (ctx->slice_first) (void)hipFree(ctx->slice_first);
            ctx->slice_first = nullptr;
            ctx->slice_pair = nullptr;
            return FGPU_ERR_NOMEM;
        }
        ctx->slice_first_bytes = fbytes;
        ctx->slice_pair_bytes = pbytes;
    }
    ctx->slice_lo = bit_lo;
    ctx->slice_n = n;
    ctx->slice_committed = false;
    ctx->slice_mercy = mercy;
    ctx->slice_probe_owed = false;
    ctx->slice_owed_span = 0;
    ctx->scan_resident_base = 0;
    for (PackedBlock* b : ctx->packed) b->state = 0;      // blocks of earlier passes: their buffers serve this one
    ctx->shard_times = ctx->shard_planes = ctx->fixup_ready = false;
    ctx->rec_layout = false;
    ctx->pass_positions = ctx->pass_batches = 0;
    ctx->pass_empty_carry = true;
    // carry and sweeps as in a plain pass (fgpu_load_pass_policy).  The bar on an epoch's size, sweep_min, is taken over unchanged: a sweep of the
    // slice streams 1/N of what a whole-filter sweep streams, and the epoch's accesses INTO the slice are 1/N as well, so the ratio the bar
    // stands for is the same -- but the value was measured on whole filters only; for slices it is an unmeasured choice.
    fgpu_load_pass_policy(ctx);
    fgpu_resident_reset(ctx, true);
    int rc = fgpu_slice_pair_begin(ctx);
    if (rc) return rc;
    if ((rc = fgpu_load_pass_counters(ctx))) return rc;
    ctx->phase = 3;
    return FGPU_OK;
}

int fgpu_load_slice_begin(fgpu_ctx* ctx, uint64_t bit_lo, uint64_t bit_hi) { return slice_begin(ctx, bit_lo, bit_hi, false); }
int fgpu_load_slice_mercy_begin(fgpu_ctx* ctx, uint64_t bit_lo, uint64_t bit_hi) { return slice_begin(ctx, bit_lo, bit_hi, true); }

int fgpu_load_slice_batch(fgpu_ctx* ctx, const fgpu_reads* reads) {
    if (!ctx) return FGPU_ERR_ARG;
    int rc = slice_check(ctx, "load_slice_batch", SLICE_PROBED);
    if (rc || (rc = fgpu_check_reads(ctx, reads))) return rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if ((rc = fgpu_stage_pack(ctx, reads))) return rc;
    if ((rc = fgpu_stage_slice_load(ctx))) return rc;
    if (ctx->cur->T) ctx->pass_batches++;
    ctx->load_stats.reads_processed += reads->n_reads;
    return fgpu_host_batch_done(ctx, reads);
}

// ---- packed batches of a sliced pass: made here or by a peer, loaded from the packed form (faucet_gpu.h) --------------------------------
int fgpu_load_slice_pack(fgpu_ctx* ctx, const fgpu_reads* reads, fgpu_packed* out) {
    if (!ctx || !out) return FGPU_ERR_ARG;
    int rc = slice_check(ctx, "load_slice_pack", SLICE_LOADING);
    if (rc || (rc = fgpu_check_reads(ctx, reads))) return rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    PackedBlock* b = nullptr;
    if ((rc = fgpu_stage_pack_block(ctx, reads, &b))) return rc;
    packed_describe(b, reads->n_reads, out);
    return fgpu_host_batch_done(ctx, reads);
}

int fgpu_load_slice_expect(fgpu_ctx* ctx, uint64_t T, uint64_t n_reads, fgpu_packed* out) {
    if (!ctx || !out) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_expect", SLICE_LOADING)) return rc;
    // a stream holds one separator per read: T >= n_reads, and T = 0 exactly for a batch without reads
    if (n_reads > T || (T && !n_reads) || T > ctx->prm.max_batch_bases || T >= 0xFFFFFF00ULL) {
        ctx->err = "load_slice_expect: T stream positions (bases + one separator per read, at most max_batch_bases) of n_reads <= T reads";
        return FGPU_ERR_ARG;
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    PackedBlock* b = nullptr;
    if (T)
        if (int rc = fgpu_packed_acquire(ctx, T, n_reads, 2, "load_slice_expect", &b)) return rc;
    packed_describe(b, n_reads, out);
    return FGPU_OK;
}

int fgpu_load_slice_batch_packed(fgpu_ctx* ctx, const fgpu_packed* pk) {
    if (!ctx || !pk) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_batch_packed", SLICE_PROBED)) return rc;
    if (!pk->block_dev) {                        // a batch without reads has no block
        if (pk->T || pk->nbytes || pk->n_reads) { ctx->err = "load_slice_batch_packed: a description without a block must be empty"; return FGPU_ERR_ARG; }
        return FGPU_OK;
    }
    PackedBlock* b = nullptr;
    for (PackedBlock* q : ctx->packed)
        if (q->buf.p == pk->block_dev) b = q;
    if (!b || (b->state != 1 && b->state != 2)) {
        ctx->err = !b ? "load_slice_batch_packed: not a block of fgpu_load_slice_pack / fgpu_load_slice_expect"
                      : b->state == 3 ? "load_slice_batch_packed: the block has been loaded already"
                                      : "load_slice_batch_packed: the block belongs to an earlier pass";
        return FGPU_ERR_STATE;
    }
    if (pk->T != b->T || pk->nbytes != fgpu_packed_bytes(b->n_words) || pk->n_reads != b->n_reads) {
        ctx->err = "load_slice_batch_packed: T, nbytes or n_reads are not those the block was made with";
        return FGPU_ERR_ARG;
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (int rc = fgpu_stage_slice_load_packed(ctx, b)) return rc;
    ctx->pass_batches++;
    ctx->load_stats.reads_processed += b->n_reads;
    return FGPU_OK;
}

// ---- a sliced pass that keeps reads: the offsets of its packed batches, beside the blocks (faucet_gpu.h) ----------------------------------------
int fgpu_load_slice_keep_reads(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_keep_reads", SLICE_LOADING)) return rc;
    bool any = ctx->pass_batches != 0 || ctx->resident_count != 0;
    for (const PackedBlock* b : ctx->packed) any = any || b->state != 0;
    if (any) { ctx->err = "load_slice_keep_reads after the pass' first batch or block: a pass keeps the reads of all the batches it packs or of none"; return FGPU_ERR_STATE; }
    ctx->keep_reads = ctx->kept_sliced = true;
    return FGPU_OK;
}

// the block of the latest sliced pass a description speaks of, with the resident batch it became (null: not loaded yet)
static int kept_block_of(fgpu_ctx* ctx, const char* who, const fgpu_packed* pk, PackedBlock** out, ResidentBatch** res) {
    const std::string w(who);
    if (ctx->phase != 0 && ctx->phase != 3) { ctx->err = w + " inside a pass that is not a sliced load pass"; return FGPU_ERR_STATE; }
    if (!ctx->kept_sliced) { ctx->err = w + ": the latest load pass was not a sliced pass that keeps its reads (fgpu_load_slice_keep_reads)"; return FGPU_ERR_STATE; }
    PackedBlock* b = nullptr;
    if (pk->block_dev)
        for (PackedBlock* q : ctx->packed)
            if (q->buf.p == pk->block_dev && q->state != 0) b = q;
    if (!b) { ctx->err = w + ": not a block of this pass' fgpu_load_slice_pack / fgpu_load_slice_expect"; return FGPU_ERR_STATE; }
    if (pk->T != b->T || pk->nbytes != fgpu_packed_bytes(b->n_words) || pk->n_reads != b->n_reads) {
        ctx->err = w + ": T, nbytes or n_reads are not those the block was made with";
        return FGPU_ERR_ARG;
    }
    *out = b;
    *res = nullptr;
    if (b->state == 3 && b->resident_index < ctx->resident_count && ctx->resident[b->resident_index]->packed_codes == b->buf.p) *res = ctx->resident[b->resident_index];
    return FGPU_OK;
}

int fgpu_load_slice_packed_reads(fgpu_ctx* ctx, const fgpu_packed* pk, fgpu_kept_reads* out) {
    if (!ctx || !pk || !out) return FGPU_ERR_ARG;
    PackedBlock* b;
    ResidentBatch* r;
    if (!pk->block_dev && !pk->T && !pk->n_reads) { *out = fgpu_kept_reads{nullptr, 0, 0}; return FGPU_OK; }      // a batch without reads has neither
    if (int rc = kept_block_of(ctx, "load_slice_packed_reads", pk, &b, &r)) return rc;
    if (b->offs_state != 1 && b->offs_state != 3) { ctx->err = "load_slice_packed_reads: the block has no read offsets (it was not packed here, and none have been adopted)"; return FGPU_ERR_STATE; }
    out->offsets_dev = b->offs.p;
    out->n_reads = b->n_reads;
    out->max_read_len = ctx->kept_max_read_len;
    return FGPU_OK;
}

int fgpu_load_slice_expect_reads(fgpu_ctx* ctx, const fgpu_packed* pk, fgpu_kept_reads* out) {
    if (!ctx || !pk || !out) return FGPU_ERR_ARG;
    PackedBlock* b;
    ResidentBatch* r;
    if (!pk->block_dev && !pk->T && !pk->n_reads) { *out = fgpu_kept_reads{nullptr, 0, 0}; return FGPU_OK; }      // a batch without reads has neither
    if (int rc = kept_block_of(ctx, "load_slice_expect_reads", pk, &b, &r)) return rc;
    if (b->offs_state == 1 || b->offs_state == 3) { ctx->err = "load_slice_expect_reads: the block has its read offsets already"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const uint64_t ob = (b->n_reads + 1) * 8;
    if (b->offs_state == 0) {
        if (ctx->resident_bytes + ob > ctx->resident_budget) {
            ctx->err = "load_slice_expect_reads: the " + std::to_string(ob) + " bytes of read offsets of a batch of " + std::to_string(b->n_reads) +
                       " reads do not fit the budget for resident batches (" + std::to_string(ctx->resident_budget) + " bytes, " + std::to_string(ctx->resident_bytes) + " in use)";
            return FGPU_ERR_NOMEM;
        }
        if (int rc = fgpu_ensure(ctx, &b->offs, ob)) {
            ctx->err = "load_slice_expect_reads: no device memory for the read offsets (budget " + std::to_string(ctx->resident_budget) + " bytes): " + ctx->err;
            return rc;
        }
        ctx->resident_bytes += ob;
        b->offs_state = 2;
    }
    out->offsets_dev = b->offs.p;
    out->n_reads = b->n_reads;
    out->max_read_len = 0;
    return FGPU_OK;
}

int fgpu_load_slice_adopt_reads(fgpu_ctx* ctx, const fgpu_packed* pk, const fgpu_kept_reads* kr) {
    if (!ctx || !pk || !kr) return FGPU_ERR_ARG;
    PackedBlock* b;
    ResidentBatch* r;
    if (!pk->block_dev && !pk->T && !pk->n_reads && !kr->offsets_dev) return FGPU_OK;
    if (int rc = kept_block_of(ctx, "load_slice_adopt_reads", pk, &b, &r)) return rc;
    if (b->offs_state != 2) { ctx->err = "load_slice_adopt_reads: no allocation of fgpu_load_slice_expect_reads waits beside this block"; return FGPU_ERR_STATE; }
    if (!r) { ctx->err = "load_slice_adopt_reads: the block has not been loaded yet (fgpu_load_slice_batch_packed): its bad plane is what the offsets are checked against"; return FGPU_ERR_STATE; }
    if (kr->offsets_dev != b->offs.p || kr->n_reads != b->n_reads) { ctx->err = "load_slice_adopt_reads: not the allocation fgpu_load_slice_expect_reads made for this block"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (!ctx->offs_check.p) {
        if (int rc = fgpu_ensure(ctx, &ctx->offs_check, sizeof(OffsCheck))) return rc;
        FGPU_HIP(hipMemsetAsync(ctx->offs_check.p, 0, 8, ctx->stream));
        FGPU_HIP(hipMemsetAsync((char*)ctx->offs_check.p + 8, 0xFF, 8, ctx->stream));
    }
    FGPU_LAUNCH("offs_check", k_offs_check, fgpu_grid(b->n_reads, 256), 256, (const uint64_t*)b->offs.p, b->n_reads, b->T, (const uint64_t*)r->bad_p(),
                b->resident_index, (OffsCheck*)ctx->offs_check.p);
    ctx->offs_unchecked.push_back(b->resident_index);
    b->offs_state = 3;
    r->packed_offs = b->offs.p;
    r->n_reads = b->n_reads;
    ctx->kept_reads_total += b->n_reads;
    ctx->kept_max_read_len = std::max<uint64_t>(ctx->kept_max_read_len, kr->max_read_len);
    return FGPU_OK;
}

}  // extern "C"

// The checks of the offsets adopted since the last look: waits for the context's stream.  A failure takes the offsets of every batch adopted
// since then away again (only the lowest failing batch is known by name) and leaves the context usable.
int fgpu_offs_check_report(fgpu_ctx* ctx) {
    if (ctx->offs_unchecked.empty()) return FGPU_OK;
    OffsCheck oc = {0, 0};
    FGPU_HIP(hipMemcpyAsync(&oc, ctx->offs_check.p, sizeof(oc), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    std::vector<uint64_t> unchecked;
    unchecked.swap(ctx->offs_unchecked);
    if (!oc.failed) return FGPU_OK;
    FGPU_HIP(hipMemsetAsync(ctx->offs_check.p, 0, 8, ctx->stream));
    FGPU_HIP(hipMemsetAsync((char*)ctx->offs_check.p + 8, 0xFF, 8, ctx->stream));
    for (uint64_t i : unchecked) {
        if (i >= ctx->resident_count || !ctx->resident[i]->n_reads) continue;
        ResidentBatch& r = *ctx->resident[i];
        ctx->kept_reads_total -= r.n_reads;
        r.n_reads = 0;
        r.packed_offs = nullptr;
        for (PackedBlock* b : ctx->packed)
            if (b->resident_index == i && b->offs_state == 3) b->offs_state = 2;      // (the allocation stays, charged: it may be filled and adopted again)
    }
    ctx->err = "fgpu_load_slice_adopt_reads: the read offsets adopted for batch " + std::to_string(oc.batch) + " are not those of its block (offsets[0] = 0, "
               "ascending, offsets[n] + n = T, a separator behind every read in the block's bad plane): another batch's offsets, or damaged on their way";
    return FGPU_ERR_ARG;
}

extern "C" {

int fgpu_load_slice_plane(fgpu_ctx* ctx, uint64_t batch, void** fail_dev, uint64_t* nbytes) {
    if (!ctx || !fail_dev) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_plane", SLICE_OPEN)) return rc;
    if (batch >= ctx->resident_count) { ctx->err = "load_slice_plane: no such batch (empty batches keep no plane)"; return FGPU_ERR_ARG; }
    const ResidentBatch& r = *ctx->resident[batch];
    *fail_dev = r.fail.p;
    if (nbytes) *nbytes = (r.n_words * 8 + 15) & ~15ULL;
    return FGPU_OK;
}

int fgpu_load_slice_mercy_probe(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_mercy_probe", SLICE_MERCY)) return rc;
    if (!ctx->slice_probe_owed) return FGPU_OK;      // an empty batch, or nothing since the last probe
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    return fgpu_stage_slice_mercy_probe(ctx);
}

int fgpu_load_slice_mercy_planes(fgpu_ctx* ctx, uint64_t batch, void** miss_dev, uint64_t* nbytes) {
    if (!ctx || !miss_dev) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_mercy_planes", SLICE_MERCY)) return rc;
    if (batch >= ctx->resident_count) { ctx->err = "load_slice_mercy_planes: no such batch (empty batches keep no planes)"; return FGPU_ERR_ARG; }
    if (ctx->slice_probe_owed && batch == ctx->resident_count - 1) {
        ctx->err = "load_slice_mercy_planes: this batch has not been probed yet (fgpu_load_slice_mercy_probe)";
        return FGPU_ERR_STATE;
    }
    const ResidentBatch& r = *ctx->resident[batch];
    *miss_dev = r.miss.p;
    if (nbytes) *nbytes = 4 * (r.n_words + FGPU_PADW) * 8;      // four planes of the fail plane's padded stride, one block
    return FGPU_OK;
}

int fgpu_diag_slice_mercy(fgpu_ctx* ctx, uint64_t out[6]) {
    if (!ctx || !out) return FGPU_ERR_ARG;
    for (int i = 0; i < 6; i++) out[i] = ctx->slice_mercy_diag[i];
    return FGPU_OK;
}

int fgpu_load_slice_commit(fgpu_ctx* ctx) {
    if (!ctx) return FGPU_ERR_ARG;
    if (int rc = slice_check(ctx, "load_slice_commit", SLICE_COMMIT)) return rc;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    int rc = fgpu_stage_slice_commit(ctx);
    if (rc) return rc;
    ctx->slice_committed = true;
    return FGPU_OK;
}

int fgpu_load_slice_end(fgpu_ctx* ctx, fgpu_load_stats* stats) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ctx->phase != 3) { ctx->err = "load_slice_end without load_slice_begin"; return FGPU_ERR_STATE; }
    if (!ctx->slice_committed) { ctx->err = "load_slice_end before load_slice_commit"; return FGPU_ERR_STATE; }
    // bloo1 / bloo2 := the own slice at its place in the tai/8-byte arrays, zero outside it (fgpu_load_pair_end)
    if (int rc = fgpu_load_pass_end(ctx, stats)) return rc;
    ctx->load_mark_hits = 0;
    for (int i = 0; i < 6; i++) ctx->slice_mercy_diag[i] = ctx->slice_mercy ? ctx->counters_host->slice_mercy[i] : 0;
    return FGPU_OK;
}

int fgpu_load_slice_state(fgpu_ctx* ctx, int* ready, uint64_t* working_bytes, uint64_t* n_batches) {
    if (!ctx) return FGPU_ERR_ARG;
    if (ready) *ready = ctx->phase == 3 && !ctx->slice_committed ? 1 : 0;
    if (working_bytes) *working_bytes = ctx->slice_first_bytes + ctx->slice_pair_bytes;
    if (n_batches) *n_batches = ctx->phase == 3 ? ctx->resident_count : 0;
    return FGPU_OK;
}

}  // extern "C"
