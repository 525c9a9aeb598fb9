// scan_table.hip — the junction table's life cycle outside the walk: growing and emptying it, the export / import format of the multi-GPU
// hand-over (which growing goes through as well), the creation-ordered download and the reference's dump order.
// The table's layout and look-ups are in walk_tables.h; the walk that fills it is scan_walk.hip.
#include <algorithm>

#include "walk_tables.h"

#include <rocprim/rocprim.hpp>

namespace {

// ---- export: compact the present records ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_export(JTable jt, FdParams fp, ExportEntry* out, uint64_t* stamps_out, unsigned long long* n_out) {
    // Every block owns a contiguous range of slots and reserves its output space ONCE: a first pass over the key words counts the
    // records of the range, one atomic claims that many entries, a second pass writes them (ranks from ballots and wave totals).
    // One same-address atomic per 256 slots, as before, cost 5 ms at 2^27 slots -- they serialise at ~10 ns each -- and the export is
    // on the path of every hand-over between ranks; the key words read twice are 1 GiB of streaming there.
    __shared__ unsigned wave_total[4];
    __shared__ unsigned long long block_base;
    const uint64_t n_slots = jt.mask + 1;
    const uint64_t per_block = ((n_slots + gridDim.x - 1) / gridDim.x + 255) & ~255ULL;
    const uint64_t lo = (uint64_t)blockIdx.x * per_block;
    const uint64_t hi = lo + per_block < n_slots ? lo + per_block : n_slots;
    const int wave = (int)(threadIdx.x >> 6);
    unsigned long long mine = 0;
    for (uint64_t s = lo + threadIdx.x; s < hi; s += 256) {
        const uint64_t w = jt.keys[s];
        if (w != J_EMPTY) mine += ((w >> 62) & 1ULL) + ((w >> 63) & 1ULL);
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
    if (fd_lane() == 0) wave_total[wave] = (unsigned)mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long total = (unsigned long long)wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        block_base = total ? atomicAdd(n_out, total) : 0ULL;
    }
    __syncthreads();
    unsigned long long base = block_base;
    for (uint64_t s0 = lo; s0 < hi; s0 += 256) {     // uniform trip count: hi - lo is a multiple of 256 except in the last block
        const uint64_t s = s0 + threadIdx.x;
        const uint64_t w = s < hi ? jt.keys[s] : J_EMPTY;
        const bool has0 = w != J_EMPTY && ((w >> 62) & 1ULL), has1 = w != J_EMPTY && ((w >> 63) & 1ULL);
        const uint64_t m0 = __ballot(has0), m1 = __ballot(has1);
        const uint64_t below = (1ULL << fd_lane()) - 1;
        unsigned rank = (unsigned)(__popcll(m0 & below) + __popcll(m1 & below));
        __syncthreads();                               // the totals of the previous chunk have been read by everybody
        if (fd_lane() == 0) wave_total[wave] = (unsigned)(__popcll(m0) + __popcll(m1));
        __syncthreads();
        for (int q = 0; q < wave; q++) rank += wave_total[q];
        unsigned long long idx = base + rank;
        base += (unsigned long long)wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        const uint64_t canon = w & J_KEYMASK;
        for (int o = 0; o < 2; o++) {
            if (!(o == 0 ? has0 : has1)) continue;
            ExportEntry e;
            e.key = o == 0 ? canon : fd_revcomp(canon, fp.k);
            e.stamp = jt.stamps[s * 2 + o];
            const uint64_t* r = (const uint64_t*)(jt.recs + (s * 2 + o) * 16);
            ((uint64_t*)e.rec)[0] = r[0];
            ((uint64_t*)e.rec)[1] = r[1];
            out[idx] = e;
            stamps_out[idx] = e.stamp;
            idx++;
        }
    }
}

__global__ void __launch_bounds__(256) k_gather_sorted(const ExportEntry* in, const uint32_t* order, uint64_t n, uint64_t* keys,
                                                       fgpu_junction* recs) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ExportEntry e = in[order[i]];
    keys[i] = e.key;
    fgpu_junction r;
    for (int c = 0; c < 4; c++) r.cov[c] = e.rec[5 + c];
    for (int c = 0; c < 5; c++) { r.dist[c] = e.rec[c]; r.linked[c] = (e.rec[9] >> c) & 1; }
    recs[i] = r;
}

// what an import has to know about its entries beyond putting them into the table: the largest creation stamp (piece number) among them, and --
// when a preview is being replaced by a later state of the same table -- which keys are newer than the preview: counted, and put into the filter
__global__ void __launch_bounds__(256) k_import_probe(const ExportEntry* in, uint64_t n, FdParams fp, uint64_t after_seq, uint32_t* dfilter,
                                                      uint64_t dmask, unsigned long long* out) {
    // out[2], out[3]: a digest (XOR and sum of the mixed keys) of the entries that are NOT newer -- of a preview: of all its keys.  A table that is
    // a later state of a preview holds the preview's keys with their stamps, so its not-newer entries give the preview's digest (the
    // count alone could agree by coincidence for a table that is NOT such a state, e.g. after the sender replayed its scan)
    unsigned long long mx = 0, newer = 0, dx = 0, dsum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const ExportEntry e = in[i];
        const unsigned long long seq = e.stamp >> STAMP_SHIFT;
        mx = seq > mx ? seq : mx;
        if (seq <= after_seq) {
            const unsigned long long m = fd_mix(e.key ^ 0x9E3779B97F4A7C15ULL);
            dx ^= m;
            dsum += m;
        }
        if (seq > after_seq) {
            newer++;
            if (dfilter) {
                const uint64_t rc = fd_revcomp(e.key, fp.k);
                const uint32_t h32 = jt_h32(e.key < rc ? e.key : rc);
                atomicOr(&dfilter[delta_word(h32, dmask)], delta_bits(h32));
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_down(mx, o, 64);
        mx = t > mx ? t : mx;
        newer += __shfl_down(newer, o, 64);
        dx ^= __shfl_down(dx, o, 64);
        dsum += __shfl_down(dsum, o, 64);
    }
    if (fd_lane() == 0) {
        if (mx) atomicMax(&out[0], mx);
        if (newer) atomicAdd(&out[1], newer);
        if (dx) atomicXor(&out[2], dx);
        if (dsum) atomicAdd(&out[3], dsum);
    }
}

__global__ void __launch_bounds__(256) k_import(JTable jt, FdParams fp, const ExportEntry* in, uint64_t n, DevCounters* cnt) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ExportEntry e = in[i];
    uint64_t rc = fd_revcomp(e.key, fp.k);
    uint64_t canon = e.key < rc ? e.key : rc;
    int orient = e.key == canon ? 0 : 1;
    uint64_t slot;
    uint32_t present;
    const uint64_t home = fd_mix(canon) & jt.mask;
    if (!jt_find_or_claim(jt, canon, home, ld_agent(&jt.keys[home]), slot, present, cnt)) { atomicOr(&cnt->error_flags, 1ULL); return; }
    uint64_t* r = (uint64_t*)(jt.recs + (slot * 2 + orient) * 16);
    r[0] = ((const uint64_t*)e.rec)[0];
    r[1] = ((const uint64_t*)e.rec)[1];
    jt.stamps[slot * 2 + orient] = e.stamp;
    atomicOr((unsigned long long*)&jt.keys[slot], 1ULL << (62 + orient));
    const uint64_t hb = jt_filter_bit(jt, canon);
    atomicOr(&jt.filter[hb >> 5], 1u << (hb & 31));
}

// ---- the reference's dump order on the device (host/junction_order.h: the closed form of what std::unordered_map does to its node list) -----
// stretch j of the insertion sequence: position t holds node list[t] (t < c: the list as the last rehash found it) or node t itself (t >= c:
// inserted since); its bucket is key % B.  first[b] = the earliest position of bucket b.
__global__ void __launch_bounds__(256) k_dump_first(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ list, uint64_t c, uint64_t m, uint64_t B,
                                                    uint32_t* __restrict__ bucket, uint32_t* first) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t node = t < c ? list[t] : (uint32_t)t;
        const uint32_t b = (uint32_t)(keys[node] % B);
        bucket[t] = b;
        atomicMin(&first[b], (uint32_t)t);
    }
}
// sort key: (first time of the node's bucket, own time), both descending
__global__ void __launch_bounds__(256) k_dump_key(const uint32_t* __restrict__ list, uint64_t c, uint64_t m, const uint32_t* __restrict__ bucket,
                                                  const uint32_t* __restrict__ first, uint64_t* __restrict__ sortkey, uint32_t* __restrict__ node_out) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (uint64_t)gridDim.x * blockDim.x) {
        node_out[t] = t < c ? list[t] : (uint32_t)t;
        sortkey[t] = ((uint64_t)(0xFFFFFFFFu - first[bucket[t]]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)t);
    }
}
}  // namespace

// (see fgpu_touch_scan_walk)
void fgpu_touch_scan_table() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)k_export);
}

// ---- junction download / export / import -------------------------------------------------------------------------
int fgpu_scan_export_impl(fgpu_ctx* ctx, void* dev_entries, uint64_t cap_entries, uint64_t* d_stamps, uint64_t* n_entries) {
    unsigned long long* d_n = &ctx->counters->pad;
    FGPU_HIP(hipMemsetAsync(d_n, 0, 8, ctx->stream));
    (void)cap_entries;
    FGPU_LAUNCH("export", k_export, (unsigned)std::min<uint64_t>(fgpu_blocks(ctx->jcap, 256), 4096), 256, make_jt(ctx), ctx->fd, (ExportEntry*)dev_entries,
                d_stamps, d_n);
    FGPU_HIP(hipMemcpyAsync(&ctx->counters_host->pad, d_n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    *n_entries = ctx->counters_host->pad;
    return FGPU_OK;
}

int fgpu_scan_import_impl(fgpu_ctx* ctx, const void* dev_entries, uint64_t n) {
    if (!n) return FGPU_OK;
    FGPU_LAUNCH("import", k_import, fgpu_blocks(n, 256), 256, make_jt(ctx), ctx->fd, (const ExportEntry*)dev_entries, n, ctx->counters);
    return FGPU_OK;
}

int fgpu_scan_import_probe(fgpu_ctx* ctx, const void* dev_entries, uint64_t n, uint64_t after_seq, uint32_t* dfilter, uint64_t dfilter_bits,
                           uint64_t* max_seq, uint64_t* n_newer, uint64_t digest[2]) {
    *max_seq = *n_newer = 0;
    digest[0] = digest[1] = 0;
    if (!n) return FGPU_OK;
    if (int rc = fgpu_ensure(ctx, &ctx->import_probe, 32)) return rc;
    FGPU_HIP(hipMemsetAsync(ctx->import_probe.p, 0, 32, ctx->stream));
    FGPU_LAUNCH("import", k_import_probe, (unsigned)std::min<uint64_t>(fgpu_blocks(n, 256), 4096), 256, (const ExportEntry*)dev_entries, n, ctx->fd, after_seq, dfilter,
                dfilter_bits ? dfilter_bits - 1 : 0, (unsigned long long*)ctx->import_probe.p);
    unsigned long long out[4] = {0, 0, 0, 0};
    FGPU_HIP(hipMemcpyAsync(out, ctx->import_probe.p, 32, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    *max_seq = out[0];
    *n_newer = out[1];
    digest[0] = out[2];
    digest[1] = out[3];
    return FGPU_OK;
}

// empty junction table (a new scan, a new set of arrays, a preview that is being replaced by the real state); both streams idle
int fgpu_scan_clear_table(fgpu_ctx* ctx) {
    FGPU_HIP(hipMemsetAsync(ctx->jkeys, 0xFF, ctx->jcap * 8, ctx->stream));
    FGPU_HIP(hipMemsetAsync(ctx->jrecs, 0, ctx->jcap * 32, ctx->stream));
    FGPU_HIP(hipMemsetAsync(ctx->jfilter, 0, ctx->jcap * 2 / 8, ctx->stream));
    return FGPU_OK;
}

// The table's four arrays replaced by new ones of new_cap slots, whose contents are the caller's to set (both streams idle).
// `no_memory`: how the message begins when the device cannot hold the new arrays beside the old ones; the table is untouched then.
static int jt_replace_arrays(fgpu_ctx* ctx, uint64_t new_cap, const char* no_memory) {
    uint64_t* nk = nullptr; uint8_t* nr = nullptr; uint64_t* ns = nullptr; uint32_t* nf = nullptr;
    if (hipMalloc(&nk, new_cap * 8) != hipSuccess || hipMalloc(&nr, new_cap * 32) != hipSuccess || hipMalloc(&ns, new_cap * 16) != hipSuccess ||
        hipMalloc(&nf, new_cap * 2 / 8) != hipSuccess) {
        (void)hipGetLastError();
        hipFree(nk); hipFree(nr); hipFree(ns); hipFree(nf);
        ctx->err = no_memory + std::to_string(new_cap) + " slots";
        return FGPU_ERR_NOMEM;
    }
    hipFree(ctx->jkeys); hipFree(ctx->jrecs); hipFree(ctx->jstamps); hipFree(ctx->jfilter);
    ctx->jkeys = nk; ctx->jrecs = nr; ctx->jstamps = ns; ctx->jfilter = nf;
    ctx->jcap = new_cap;
    return FGPU_OK;
}

// Rehash the junction table into new_cap slots.  Both streams are drained first; records, creation stamps and presence bits
// travel through the export format of the multi-GPU hand-over (k_export / k_import), so nothing about a junction changes.
int fgpu_scan_grow(fgpu_ctx* ctx, uint64_t new_cap) {
    if (new_cap <= ctx->jcap) return FGPU_OK;
    if (ctx->wstream) FGPU_HIP(fgpu_sync_stream(ctx, ctx->wstream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&ctx->counters_host->n_junctions, &ctx->counters->n_junctions, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&ctx->counters_host->error_flags, &ctx->counters->error_flags, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    if (ctx->counters_host->error_flags & 1ULL) return FGPU_OK;   // already overflowed: the scan is void, the caller reports it
    const uint64_t n_max = ctx->counters_host->n_junctions + ctx->scan_imported;
    int rc;
    if ((rc = fgpu_ensure(ctx, &ctx->dl_entries, (n_max + 1) * sizeof(ExportEntry))) || (rc = fgpu_ensure(ctx, &ctx->dl_stamps, (n_max + 1) * 8))) return rc;
    uint64_t n = 0;
    if (n_max && (rc = fgpu_scan_export_impl(ctx, ctx->dl_entries.p, n_max, (uint64_t*)ctx->dl_stamps.p, &n))) return rc;
    if (n != n_max) { ctx->err = "junction count mismatch between counters and table (grow)"; return FGPU_ERR_STATE; }
    if ((rc = jt_replace_arrays(ctx, new_cap, "junction table: no memory to grow to ")) || (rc = fgpu_scan_clear_table(ctx))) return rc;
    if ((rc = fgpu_scan_import_impl(ctx, ctx->dl_entries.p, n))) return rc;
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));   // the walk stream starts on the new table
    ctx->scan_grown++;
    return FGPU_OK;
}

// A batch outgrew the table (error bit 1): the scan's attempt is void and is made again from the journal -- on a table with new_cap slots, EMPTY
// (nothing of the void attempt is kept).  Both streams idle.  The reference's unordered_map just grows (utils/JunctionMap.h:61).
int fgpu_scan_regrow_empty(fgpu_ctx* ctx, uint64_t new_cap) {
    if (new_cap <= ctx->jcap) return FGPU_OK;
    if (int rc = jt_replace_arrays(ctx, new_cap, "junction table full, and no memory to grow it to ")) return rc;
    ctx->scan_grown++;
    return fgpu_scan_clear_table(ctx);
}

// called where the host holds a fresh count of the records (batch boundaries): keep the table below a quarter full
int fgpu_scan_reserve(fgpu_ctx* ctx, uint64_t records) {
    if (!ctx->jkeys || records * 4 <= ctx->jcap) return FGPU_OK;
    uint64_t want = ctx->jcap;
    while (want < records * 16 && want < (1ULL << 31)) want <<= 1;
    return fgpu_scan_grow(ctx, want);
}

// order_host[i] = index (in creation order) of the i-th junction of the reference's dump; d_keys: the junction keys in creation order on the device
int fgpu_scan_dump_order_impl(fgpu_ctx* ctx, const uint64_t* d_keys, const uint64_t* counts, const uint64_t* buckets, uint64_t n_phases, uint64_t n,
                              uint32_t* order_host) {
    // The whole schedule is checked here, on the host, before anything is allocated, set or launched: the first stretch reads list[t] for
    // t < counts[0] from a list no stretch has written yet, later ones from what the stretch before sorted (counts[j] <= counts[j + 1] entries),
    // and a bucket number is kept in 32 bits.
    bool any = false;
    for (uint64_t j = 0; j < n_phases; j++) {
        const uint64_t c = counts[j], m = j + 1 < n_phases ? counts[j + 1] : n, B = buckets[j];
        if (j == 0 && c != 0) { ctx->err = "fgpu_scan_dump_order: the schedule starts with the empty container (rehash_counts[0] = 0)"; return FGPU_ERR_ARG; }
        if (c > m || m > n) { ctx->err = "fgpu_scan_dump_order: rehash counts must not descend and must not exceed n"; return FGPU_ERR_ARG; }
        if (!B || B > 0xFFFFFFFFULL) { ctx->err = "fgpu_scan_dump_order: bucket counts must be in 1 .. 2^32 - 1"; return FGPU_ERR_ARG; }
        any = any || m > 0;
    }
    if (!n) return FGPU_OK;
    if (!any) { ctx->err = "fgpu_scan_dump_order: empty schedule"; return FGPU_ERR_ARG; }
    uint64_t max_b = 1;
    for (uint64_t j = 0; j < n_phases; j++) max_b = std::max(max_b, buckets[j]);
    DevBuf list_a, list_b, bucket, first, key_a, key_b, tmp;
    struct FreeAll { DevBuf* b[7]; ~FreeAll() { for (DevBuf* x : b) if (x->p) (void)hipFree(x->p); } } free_all{{&list_a, &list_b, &bucket, &first, &key_a, &key_b, &tmp}};
    auto alloc = [&](DevBuf& b, uint64_t bytes) -> int {
        if (hipMalloc(&b.p, bytes) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; ctx->err = "fgpu_scan_dump_order: out of device memory"; return FGPU_ERR_NOMEM; }
        b.bytes = bytes;
        return FGPU_OK;
    };
    int rc;
    if ((rc = alloc(list_a, n * 4)) || (rc = alloc(list_b, n * 4)) || (rc = alloc(bucket, n * 4)) || (rc = alloc(first, max_b * 4)) || (rc = alloc(key_a, n * 8)) ||
        (rc = alloc(key_b, n * 8)))
        return rc;
    size_t tmp_bytes = 0;
    FGPU_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint64_t*)key_a.p, (uint64_t*)key_b.p, (uint32_t*)list_a.p, (uint32_t*)list_b.p, n, 0, 64, ctx->stream));
    if ((rc = alloc(tmp, tmp_bytes + 16))) return rc;
    uint32_t* list = (uint32_t*)list_a.p;      // the list as the last stretch left it
    uint32_t* other = (uint32_t*)list_b.p;
    for (uint64_t j = 0; j < n_phases; j++) {
        const uint64_t c = counts[j], m = j + 1 < n_phases ? counts[j + 1] : n, B = buckets[j];
        if (m == 0) continue;
        FGPU_HIP(hipMemsetAsync(first.p, 0xFF, B * 4, ctx->stream));
        hipLaunchKernelGGL(k_dump_first, dim3(fgpu_grid(m, 256)), dim3(256), 0, ctx->stream, d_keys, (const uint32_t*)list, c, m, B, (uint32_t*)bucket.p, (uint32_t*)first.p);
        hipLaunchKernelGGL(k_dump_key, dim3(fgpu_grid(m, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)list, c, m, (const uint32_t*)bucket.p, (const uint32_t*)first.p,
                           (uint64_t*)key_a.p, other);
        // (`other` holds the nodes in sequence order now; sorted into `list`)
        size_t tb = tmp_bytes;
        FGPU_HIP(rocprim::radix_sort_pairs(tmp.p, tb, (uint64_t*)key_a.p, (uint64_t*)key_b.p, other, list, m, 0, 64, ctx->stream));
    }
    FGPU_HIP(hipMemcpyAsync(order_host, list, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}

// creation-ordered download: export, radix-sort the stamps (rocPRIM; not a hot step), gather
int fgpu_scan_download_impl(fgpu_ctx* ctx, uint64_t* keys_host, fgpu_junction* recs_host, uint64_t cap, uint64_t* n_out) {
    uint64_t n_max = ctx->scan_stats.n_junctions;
    FGPU_HIP(hipMemcpyAsync(&ctx->counters_host->n_junctions, &ctx->counters->n_junctions, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    n_max = ctx->counters_host->n_junctions + ctx->scan_imported;
    *n_out = n_max;
    if (!n_max || !keys_host || !recs_host) return FGPU_OK;
    if (cap < n_max) { ctx->err = "junction buffer too small"; return FGPU_ERR_CAPACITY; }
    // scratch lives with the context: eight hipMalloc / hipFree pairs per call cost more than the sort they served
    int rc;
    if ((rc = fgpu_ensure(ctx, &ctx->dl_entries, n_max * sizeof(ExportEntry))) || (rc = fgpu_ensure(ctx, &ctx->dl_stamps, n_max * 8)) ||
        (rc = fgpu_ensure(ctx, &ctx->dl_stamps_sorted, n_max * 8)) || (rc = fgpu_ensure(ctx, &ctx->dl_idx, n_max * 4)) ||
        (rc = fgpu_ensure(ctx, &ctx->dl_idx_sorted, n_max * 4)) || (rc = fgpu_ensure(ctx, &ctx->dl_keys, n_max * 8)) ||
        (rc = fgpu_ensure(ctx, &ctx->dl_recs, n_max * sizeof(fgpu_junction))))
        return rc;
    ExportEntry* d_entries = (ExportEntry*)ctx->dl_entries.p;
    uint64_t *d_stamps = (uint64_t*)ctx->dl_stamps.p, *d_stamps_sorted = (uint64_t*)ctx->dl_stamps_sorted.p, *d_keys = (uint64_t*)ctx->dl_keys.p;
    uint32_t *d_idx = (uint32_t*)ctx->dl_idx.p, *d_idx_sorted = (uint32_t*)ctx->dl_idx_sorted.p;
    fgpu_junction* d_recs = (fgpu_junction*)ctx->dl_recs.p;
    uint64_t n = 0;
    if ((rc = fgpu_scan_export_impl(ctx, d_entries, n_max, d_stamps, &n))) return rc;
    if (n != n_max) { ctx->err = "junction count mismatch between counters and table"; return FGPU_ERR_STATE; }
    hipLaunchKernelGGL(k_iota_u32, dim3(256), dim3(256), 0, ctx->stream, d_idx, n);
    size_t tmp_bytes = 0;
    FGPU_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_stamps, d_stamps_sorted, d_idx, d_idx_sorted, n, 0, 64, ctx->stream));
    if ((rc = fgpu_ensure(ctx, &ctx->dl_tmp, tmp_bytes ? tmp_bytes : 16))) return rc;
    FGPU_HIP(rocprim::radix_sort_pairs(ctx->dl_tmp.p, tmp_bytes, d_stamps, d_stamps_sorted, d_idx, d_idx_sorted, n, 0, 64, ctx->stream));
    hipLaunchKernelGGL(k_gather_sorted, dim3(fgpu_blocks(n, 256)), dim3(256), 0, ctx->stream, (const ExportEntry*)d_entries,
                       (const uint32_t*)d_idx_sorted, n, d_keys, d_recs);
    // page-locked destinations (fgpu_host_alloc) receive this at link speed; pageable ones through the runtime's staging
    FGPU_HIP(hipMemcpyAsync(keys_host, d_keys, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(recs_host, d_recs, n * sizeof(fgpu_junction), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    ctx->dl_keys_n = n;              // dl_keys holds the keys in creation order (fgpu_scan_dump_order works from them)
    return FGPU_OK;
}
