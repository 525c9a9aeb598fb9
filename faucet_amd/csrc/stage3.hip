// stage3.hip — JunctionMap::findNeighbor (utils/JunctionMap.cpp:231-412) for many (junction, extension) pairs at once, whole walks on the
// device.
//
// The reference's contig-graph stage (not part of this build) starts a walk at every junction along every extension it builds a contig on:
// getValidJExtension (:474-490; 4 x (Bloom::oldContains + JChecker::jcheck)) names the one next base, the DoubleKmer advances, the junction
// map is asked twice per step (backward- and forward-facing half step), until a junction or a sink is reached.  One call is a chain of
// dependent filter probes; different calls are independent -- one lane per walk.  The junction map the walks look into is handed over by the
// caller (fgpu_stage3_set_junctions: the scan's own result, or a parsed .junctions file) and kept as an open-addressing table in HBM: k-mer
// -> the five distances, which is all findNeighbor reads of a Junction.  The second half of the file chains such walks into whole
// JunctionMap::getContig calls (:133-221) for many starts at once (fgpu_stage3_contigs); for that the table holds the four coverages too.
//
// The control flow is the one of faucet_amd/stage3.py (findNeighbor in lock-step over fgpu_probe_valid_extension, one device call per step,
// bookkeeping in numpy), which is pinned on the reference's own findNeighbor (tests/golden/stage3_neighbors_*.jsonl.gz); this kernel is
// checked against both.  No filter bit and no map entry is looked at on the host.
//
// abort = 1 wherever the reference trips an assert instead of returning: dist <= maxDist after the first k-mers (:318), a valid extension
// at every step up to maxDist (:338-339), and a valid extension at a junction met before maxDist (:355, :370).  Past maxDist it has none.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

#include "fgpu_ctx.h"
#include "fgpu_flags.h"

namespace {

constexpr uint64_t S3_EMPTY = ~0ULL;

__device__ __forceinline__ uint64_t s3_slot(uint64_t key, uint64_t mask) { return (key * 0x9E3779B97F4A7C15ULL >> 20) & mask; }

// one junction per thread: key -> packed distances (byte i = dist[i]) and, in a second array that only the contig chains read, the four
// coverages (byte i = cov[i]) with the junction's row in the caller's arrays above them
__global__ void __launch_bounds__(256) k_s3_build(const uint64_t* __restrict__ keys, const fgpu_junction* __restrict__ recs, uint64_t n,
                                                  unsigned long long* __restrict__ tkeys, uint64_t* __restrict__ tdist, uint64_t* __restrict__ tcov,
                                                  uint64_t mask, unsigned int* __restrict__ repeated) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    uint64_t d = 0;
    for (int b = 0; b < 5; b++) d |= (uint64_t)recs[i].dist[b] << (8 * b);
    uint64_t c = i << 32;
    for (int b = 0; b < 4; b++) c |= (uint64_t)recs[i].cov[b] << (8 * b);
    uint64_t s = s3_slot(key, mask);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const unsigned long long old = atomicCAS(&tkeys[s], (unsigned long long)S3_EMPTY, (unsigned long long)key);
        if (old == S3_EMPTY) { tdist[s] = d; tcov[s] = c; return; }
        if (old == key) { atomicAdd(repeated, 1u); return; }
        s = (s + 1) & mask;
    }
}

// junctionMap.find(kmer): the packed distances, or false
__device__ __forceinline__ bool s3_find(const uint64_t* __restrict__ tkeys, const uint64_t* __restrict__ tdist, uint64_t mask, uint64_t key, uint64_t& dist) {
    uint64_t s = s3_slot(key, mask);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const uint64_t k = tkeys[s];
        if (k == key) { dist = tdist[s]; return true; }
        if (k == S3_EMPTY) return false;
        s = (s + 1) & mask;
    }
    return false;
}
__device__ __forceinline__ int s3_dist(uint64_t packed, int i) { return (int)((packed >> (8 * i)) & 0xFF); }

// JunctionMap::getValidJExtension (utils/JunctionMap.cpp:474-490): -1 none, -2 several, else the nucleotide
__device__ int s3_valid_extension(uint64_t km, const FdParams& fp, const uint32_t* __restrict__ bloom) {
    int r = -1;
    for (int nt = 0; nt < 4; nt++) {
        const uint64_t e = ((km << 2) | (uint64_t)nt) & fp.kmask;
        if (fd_bloom_contains_canon(bloom, fd_canon(e, fp.k), fp.tai_mask, fp.n_hash) && jcheck_dfs(e, fp, bloom)) {
            if (r != -1) return -2;
            r = nt;
        }
    }
    return r;
}

// one whole findNeighbor(junctionMap[start], start, idx) walk of one lane: the result, and with `text` its contig string (the reference's result
// :241,254-256,272-276,343), 2 bits per base, 32 bases per word, first base lowest, in at most `stride` words.  Shared by the per-pair kernel
// and by the segment walks of the contig chains below.
__device__ __forceinline__ fgpu_neighbor s3_walk(uint64_t start, int idx, const FdParams& fp, const uint32_t* __restrict__ bloom,
                                                 const uint64_t* __restrict__ tkeys, const uint64_t* __restrict__ tdist, uint64_t mask,
                                                 int max_read_length, uint64_t* __restrict__ text, uint64_t stride, unsigned long long& probes) {
    fgpu_neighbor res;
    res.kmer = 0; res.dist = 0; res.len = 0; res.node = 0; res.rindex = 0; res.abort = 0; res.reserved = 0; res.reserved2 = 0;
    {
        const int k = fp.k;
        uint64_t km = start & fp.kmask, rc = fd_revcomp(km, k);
        fgpu_neighbor sink = res;
        uint64_t packed = 0;
        bool done = false;
        if (idx < 0 || idx > 4 || !s3_find(tkeys, tdist, mask, km, packed)) {
            res.abort = 2;                                  // not a junction of the map, or no such extension: the caller's mistake, not the reference's
            done = true;
        }
        const int maxd = done ? 0 : s3_dist(packed, idx);
        int dist = 1, ln = 0, lastnuc = 0, retidx = 4, phase = 0;       // phase 0: up to maxDist, 1: past it, 3: at a junction met before it (2, "finished" in stage3.py, is a break here)
        auto forward = [&](int nuc) {                        // DoubleKmer::forward (utils/DoubleKmer.cpp:17-23)
            km = ((km << 2) | (uint64_t)nuc) & fp.kmask;
            rc = (rc >> 2) | ((uint64_t)(nuc ^ 2) << (2 * k - 2));
        };
        auto swap = [&]() { const uint64_t t = km; km = rc; rc = t; };
        uint64_t acc = 0;
        uint32_t pos = 0;
        auto emit = [&](int code) {
            if (!text) return;
            acc |= (uint64_t)code << (2 * (pos & 31));
            pos++;
            if ((pos & 31) == 0) {
                if ((pos >> 5) <= stride) text[(pos >> 5) - 1] = acc;
                acc = 0;
            }
        };
        auto emit_kmer = [&](uint64_t x) { for (int i = k - 1; i >= 0; i--) emit((int)((x >> (2 * i)) & 3)); };
        auto finish = [&](uint64_t kmer, int node, int rindex, int d, int len) {
            res.kmer = kmer; res.node = (int8_t)node; res.rindex = (int8_t)rindex; res.dist = d; res.len = len;
            done = true;
        };
        uint64_t other = 0;
        if (!done) {
            // ---- the first one or two k-mers (:251-302)
            if (idx == 4) {
                swap();                                     // doubleKmer.reverse()
                ln = k;
                emit_kmer(km);
                if (s3_find(tkeys, tdist, mask, km, other)) finish(km, 1, 4, 1, ln);
            } else {
                lastnuc = (int)(rc & 3);
                emit((int)((km >> (2 * (k - 1))) & 3));
                forward(idx);
                ln = 1 + k;
                emit_kmer(km);
                if (s3_find(tkeys, tdist, mask, rc, other)) finish(rc, 1, lastnuc, 1, ln);
                else if (maxd == 1) finish(rc, 0, lastnuc, 1, ln);
                else {
                    dist = 2;
                    if (s3_find(tkeys, tdist, mask, km, other)) finish(km, 1, 4, 2, ln);
                }
            }
            if (!done && dist > maxd) { res.abort = 1; done = true; }   // the reference's assert(dist <= maxDist)
        }
        while (!done) {
            // ---- leaving the first loop (:343-366): a junction exactly where expected, else this is (probably) a sink
            if (phase == 0 && dist >= maxd) {
                if (s3_find(tkeys, tdist, mask, km, other)) { finish(km, 1, retidx, dist, ln); break; }
                sink.kmer = km; sink.node = 0; sink.rindex = 4; sink.dist = dist; sink.len = ln;
                phase = 1;
            }
            if (phase == 1 && dist >= maxd + 2 * max_read_length) { res = sink; break; }   // :376, ran past every possible overlap
            const int ext = s3_valid_extension(km, fp, bloom);
            probes++;
            if (phase == 3) {                               // "this should be a spacer": assert(getValidJExtension(doubleKmer) >= 0), then the junction
                if (ext < 0) res.abort = 1;
                else finish(km, 1, retidx, dist, ln);
                break;
            }
            if (ext < 0) {
                if (phase == 0) res.abort = 1;              // assert(validExtension != -1 / -2)
                else res = sink;                            // off the real sequence: the sink stands
                break;
            }
            lastnuc = (int)(rc & 3);
            forward(ext);
            ln++;
            emit(ext);
            // backward-facing half step
            dist++;
            swap();
            retidx = lastnuc;
            bool isj = s3_find(tkeys, tdist, mask, km, other);
            if (phase == 0) {
                if (dist == maxd) continue;                 // break of the first loop: handled at the top of the next round
                if (isj) { phase = 3; continue; }           // a junction before maxDist: one more probe at the top of the next round (:355)
            } else if (isj) {                               // past maxDist: overlap test (:391-404)
                if (s3_dist(other, lastnuc) + maxd - dist >= 0) finish(km, 1, lastnuc, dist, ln);
                else res = sink;
                break;
            }
            // forward-facing half step
            dist++;
            swap();
            retidx = 4;
            isj = s3_find(tkeys, tdist, mask, km, other);
            if (phase == 0) {
                if (dist == maxd) continue;
                if (isj) { phase = 3; continue; }           // the same on the forward-facing k-mer (:370)
            } else if (isj) {
                if (s3_dist(other, 4) + maxd - dist >= 0) finish(km, 1, 4, dist, ln);
                else res = sink;
                break;
            }
        }
        if (text && (pos & 31) && (pos >> 5) < stride) text[pos >> 5] = acc;
    }
    return res;
}

__global__ void __launch_bounds__(256) k_s3_find_neighbors(const uint64_t* __restrict__ starts, const signed char* __restrict__ indices, uint64_t n,
                                                           FdParams fp, const uint32_t* __restrict__ bloom, const uint64_t* __restrict__ tkeys,
                                                           const uint64_t* __restrict__ tdist, uint64_t mask, int max_read_length,
                                                           fgpu_neighbor* __restrict__ out, unsigned long long* __restrict__ n_probes,
                                                           uint64_t* __restrict__ contigs, uint64_t stride) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long probes = 0;
    if (w < n) out[w] = s3_walk(starts[w], indices[w], fp, bloom, tkeys, tdist, mask, max_read_length, contigs ? contigs + w * stride : nullptr, stride, probes);
    // one atomic per wave
    for (int off = 32; off; off >>= 1) probes += __shfl_down(probes, off);
    if ((threadIdx.x & 63) == 0 && probes) atomicAdd(n_probes, probes);
}

// ---- JunctionMap::getContig (utils/JunctionMap.cpp:133-221) for many starts at once ------------------------------------------------------
// Within one getContig call the map is static (the kills come behind the loop, :210-216), so the chain from a start is a pure function of
// (map, filter, start), and every chain is a path through the same few directed segments: its own first findNeighbor call, then calls that
// leave a junction with one path out -- at 4 after a forward entry, at its covered extension after a backward one
// (Junction::getOppositeIndex).  One call walks each of those once (state 2 * row = (junction, 4), 2 * row + 1 = (junction, its covered
// extension), 2 * junctions + i = start i), links every result to the state it continues in, follows the links once per start to count
// and once to place, and gathers the strings.

constexpr uint32_t S3C_END = 0xFFFFFFFFu;                  // no continuation: a sink, a complex junction, or a state that is never entered
enum { S3C_NODE = 1, S3C_ABORT = 2, S3C_UNUSED = 4 };
struct __attribute__((aligned(16))) S3Link {               // what one hop of a chain reads
    uint32_t next;                                         // the state the chain continues in (S3C_END: it ends here)
    uint32_t add;                                          // bases the segment appends: result.contig.substr(k), :160-162
    uint8_t dist;                                          // (unsigned char) result.distance, :163
    uint8_t cov;                                           // nextJunc.getCoverage(result.index), :169
    int8_t rindex;
    uint8_t flags;
    uint32_t reserved;
};
static_assert(sizeof(S3Link) == 16, "one 16-byte read per hop");

__device__ __forceinline__ int s3c_paths_out(uint32_t cov) {   // Junction::numPathsOut
    return ((cov & 0xFF) != 0) + ((cov & 0xFF00) != 0) + ((cov & 0xFF0000) != 0) + ((cov & 0xFF000000u) != 0);
}
__device__ __forceinline__ int s3c_covered(uint32_t cov) {     // Junction::getOppositeIndex(4): the first covered extension
    for (int i = 0; i < 3; i++) if ((cov >> (8 * i)) & 0xFF) return i;
    return 3;
}
__device__ __forceinline__ uint8_t s3c_coverage(uint32_t cov, int index) {   // (unsigned char) Junction::getCoverage
    if (index < 4) return (uint8_t)(cov >> (8 * index));
    return (uint8_t)((cov & 0xFF) + ((cov >> 8) & 0xFF) + ((cov >> 16) & 0xFF) + (cov >> 24));
}
__device__ __forceinline__ uint32_t s3c_cov_of(const fgpu_junction& r) {
    return (uint32_t)r.cov[0] | (uint32_t)r.cov[1] << 8 | (uint32_t)r.cov[2] << 16 | (uint32_t)r.cov[3] << 24;
}
// junctionMap.find(kmer): the coverage word (coverages, row above them), or false
__device__ __forceinline__ bool s3c_find_cov(const uint64_t* __restrict__ tkeys, const uint64_t* __restrict__ tcov, uint64_t mask, uint64_t key, uint64_t& cov) {
    uint64_t s = s3_slot(key, mask);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const uint64_t k = tkeys[s];
        if (k == key) { cov = tcov[s]; return true; }
        if (k == S3_EMPTY) return false;
        s = (s + 1) & mask;
    }
    return false;
}

// one lane per state: the findNeighbor call that leaves it.  States of junctions that no chain continues through (numPathsOut != 1) are not walked.
__global__ void __launch_bounds__(256) k_s3c_segments(const uint64_t* __restrict__ keys, const fgpu_junction* __restrict__ recs, uint64_t nj,
                                                      const uint64_t* __restrict__ starts, const signed char* __restrict__ indices, uint64_t n,
                                                      FdParams fp, const uint32_t* __restrict__ bloom, const uint64_t* __restrict__ tkeys,
                                                      const uint64_t* __restrict__ tdist, uint64_t mask, int max_read_length,
                                                      fgpu_neighbor* __restrict__ seg, unsigned long long* __restrict__ n_probes,
                                                      uint64_t* __restrict__ text, uint64_t stride) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long probes = 0;
    if (s < 2 * nj + n) {
        uint64_t start = 0;
        int idx = -1;
        if (s < 2 * nj) {
            const uint32_t cov = s3c_cov_of(recs[s >> 1]);
            if (s3c_paths_out(cov) == 1) { start = keys[s >> 1]; idx = (s & 1) ? s3c_covered(cov) : 4; }
        } else {
            start = starts[s - 2 * nj];
            idx = indices[s - 2 * nj];
        }
        if (s >= 2 * nj || idx >= 0) seg[s] = s3_walk(start, idx, fp, bloom, tkeys, tdist, mask, max_read_length, text + s * stride, stride, probes);
        else {
            fgpu_neighbor none;
            none.kmer = 0; none.dist = 0; none.len = 0; none.node = 0; none.rindex = 0; none.abort = 2; none.reserved = 0; none.reserved2 = 0;
            seg[s] = none;
        }
    }
    for (int off = 32; off; off >>= 1) probes += __shfl_down(probes, off);
    if ((threadIdx.x & 63) == 0 && probes) atomicAdd(n_probes, probes);
}

// one lane per state: the result's junction looked up once -- its coverage, and the state the chain goes on in (:165-191)
__global__ void __launch_bounds__(256) k_s3c_link(const fgpu_neighbor* __restrict__ seg, uint64_t nj, uint64_t n, int k,
                                                  const uint64_t* __restrict__ starts, const signed char* __restrict__ indices,
                                                  const uint64_t* __restrict__ tkeys, const uint64_t* __restrict__ tcov, uint64_t mask, uint64_t kmask,
                                                  S3Link* __restrict__ link, uint64_t* __restrict__ start_info) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= 2 * nj + n) return;
    const fgpu_neighbor r = seg[s];
    S3Link l;
    l.next = S3C_END; l.add = r.len > k ? (uint32_t)(r.len - k) : 0u; l.dist = (uint8_t)r.dist; l.cov = 0; l.rindex = r.rindex; l.reserved = 0;
    l.flags = r.abort == 2 ? S3C_UNUSED : r.abort ? S3C_ABORT : r.node ? S3C_NODE : 0;
    uint64_t cv = 0;
    if (l.flags == S3C_NODE && s3c_find_cov(tkeys, tcov, mask, r.kmer, cv)) {
        const uint32_t cov = (uint32_t)cv;
        l.cov = s3c_coverage(cov, r.rindex);
        if (s3c_paths_out(cov) == 1) l.next = (uint32_t)(2 * (cv >> 32) + (r.rindex < 4 ? 0 : 1));
    }
    link[s] = l;
    if (s >= 2 * nj) {                                     // a start: its row (the end-of-chain test is on rows) and junc.getCoverage(startIndex), :148
        const uint64_t i = s - 2 * nj;
        const int idx = indices[i];
        uint64_t info = ~0ULL;
        if (idx >= 0 && idx <= 4 && s3c_find_cov(tkeys, tcov, mask, starts[i] & kmask, cv)) info = (cv >> 32) | (uint64_t)s3c_coverage((uint32_t)cv, idx) << 32;
        start_info[i] = info;
    }
}

// one lane per start, over the links.  FILL false: the status, the counts and the end of the chain.  A chain that never comes back to its start
// runs into a cycle of the states behind it; Brent's method finds that in a number of hops proportional to the chain's own tail and cycle.
// FILL true (after the scan of the counts): the chain's offsets, and per segment its state, its base offset in the string, its distance and
// the coverages.
template <bool FILL>
__global__ void __launch_bounds__(256) k_s3c_follow(const S3Link* __restrict__ link, const uint64_t* __restrict__ start_info,
                                                    const signed char* __restrict__ indices, const fgpu_neighbor* __restrict__ seg, uint64_t nj,
                                                    uint64_t n, int k, fgpu_contig* __restrict__ out, uint64_t* __restrict__ words,
                                                    uint64_t* __restrict__ segs, uint64_t* __restrict__ covs, uint32_t* __restrict__ seg_state,
                                                    uint32_t* __restrict__ seg_off, uint8_t* __restrict__ seg_dist, uint8_t* __restrict__ cov_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t info = start_info[i];
    const uint32_t row0 = (uint32_t)info;
    uint32_t s = (uint32_t)(2 * nj + i);
    if (FILL) {
        fgpu_contig c = out[i];
        c.text_word = words[i]; c.seg_first = segs[i]; c.cov_first = covs[i];
        out[i] = c;
        if (c.status) return;
        uint64_t t = c.seg_first, cv = c.cov_first;
        uint32_t len = (uint32_t)k;
        cov_out[cv++] = (uint8_t)(info >> 32);
        for (uint32_t h = 0; h < c.n_seg; h++) {
            const S3Link l = link[s];
            seg_state[t] = s; seg_off[t] = len; seg_dist[t] = l.dist;
            t++;
            len += l.add;
            if (l.flags & S3C_NODE) cov_out[cv++] = l.cov;
            s = l.next;
        }
        return;
    }
    fgpu_contig c;
    c.end_kmer = 0; c.text_word = 0; c.seg_first = 0; c.cov_first = 0; c.len = 0; c.n_seg = 0; c.n_cov = 0; c.ind1 = 0; c.ind2 = 0; c.end_node = 0; c.status = 0;
    if (info == ~0ULL) c.status = 2;
    uint32_t len = (uint32_t)k, n_seg = 0, n_cov = 1, last = s;
    uint32_t saved = S3C_END, power = 1, lam = 0;          // Brent: the state `lam` hops back, renewed at every power of two
    S3Link l = {};
    while (!c.status) {
        l = link[s];
        if (l.flags & (S3C_ABORT | S3C_UNUSED)) { c.status = 1; break; }
        last = s;
        n_seg++;
        len += l.add;
        if (l.flags & S3C_NODE) n_cov++;
        if (l.next == S3C_END || (l.next >> 1) == row0) break;     // a sink or a complex junction (:188-196); result.kmer == startKmer (:177)
        s = l.next;
        if (s == saved) { c.status = 3; break; }
        if (++lam == power) { saved = s; power <<= 1; lam = 0; }
    }
    if (!c.status) {
        c.end_kmer = seg[last].kmer;
        c.len = len; c.n_seg = n_seg; c.n_cov = n_cov;
        c.ind1 = indices[i];
        c.end_node = (l.flags & S3C_NODE) ? 1 : 0;
        c.ind2 = c.end_node ? l.rindex : 4;                // setIndices, :201-208
    }
    out[i] = c;
    words[i] = (c.len + 31) / 32; segs[i] = c.n_seg; covs[i] = c.n_cov;
}

// `count` <= 32 bases of a 2-bit text from base `base` on, in the low bits
__device__ __forceinline__ uint64_t s3c_bases(const uint64_t* __restrict__ text, uint32_t base, uint32_t count) {
    const uint32_t sh = 2 * (base & 31);
    uint64_t v = text[base >> 5] >> sh;
    if (sh && count > 32 - (base & 31)) v |= text[(base >> 5) + 1] << (64 - sh);
    return count < 32 ? v & ((1ULL << (2 * count)) - 1) : v;
}

// one lane per word of the text: the chain it belongs to, the segment its first base comes from, then piece by piece until the word is full
__global__ void __launch_bounds__(256) k_s3c_gather_text(const fgpu_contig* __restrict__ chains, uint64_t n, uint64_t total_words,
                                                         const uint64_t* __restrict__ starts, int k, uint64_t kmask, const uint32_t* __restrict__ seg_state,
                                                         const uint32_t* __restrict__ seg_off, const S3Link* __restrict__ link,
                                                         const uint64_t* __restrict__ text, uint64_t stride, uint64_t* __restrict__ out) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= total_words) return;
    uint64_t lo = 0, hi = n;                               // the last chain with text_word <= w (the empty ones before it share its offset)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (chains[mid].text_word <= w) lo = mid; else hi = mid;
    }
    const fgpu_contig c = chains[lo];
    uint32_t b = (uint32_t)(w - c.text_word) * 32;
    const uint32_t end = min(b + 32, c.len);
    uint64_t word = 0;
    uint32_t filled = 0;
    if (b < (uint32_t)k) {                                 // print_kmer(start), or of its reverse complement for index 4 (:149-151)
        uint64_t x = starts[lo] & kmask;
        if (c.ind1 == 4) x = fd_revcomp(x, k);
        uint64_t y = __builtin_bitreverse64(x);
        y = ((y >> 1) & 0x5555555555555555ULL) | ((y & 0x5555555555555555ULL) << 1);
        word = y >> (64 - 2 * k);
        filled = min((uint32_t)k, end) - b;
        b += filled;
    }
    if (b < end) {
        const uint32_t* off = seg_off + c.seg_first;
        uint32_t tl = 0, th = c.n_seg;                     // the last segment that begins at or before base b (those that append nothing share an offset)
        while (th - tl > 1) {
            const uint32_t mid = (tl + th) / 2;
            if (off[mid] <= b) tl = mid; else th = mid;
        }
        for (uint32_t t = tl; b < end && t < c.n_seg; t++) {
            const uint32_t st = seg_state[c.seg_first + t], o = off[t], add = link[st].add;
            if (b >= o + add) continue;
            const uint32_t cnt = min(o + add, end) - b;
            word |= s3c_bases(text + (uint64_t)st * stride, (uint32_t)k + (b - o), cnt) << (2 * filled);
            filled += cnt;
            b += cnt;
        }
    }
    out[w] = word;
}

// one lane per segment: BfSearchResult::kmer of its call
__global__ void __launch_bounds__(256) k_s3c_gather_kmers(const uint32_t* __restrict__ seg_state, const fgpu_neighbor* __restrict__ seg, uint64_t n,
                                                          uint64_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = seg[seg_state[t]].kmer;
}

}  // namespace

extern "C" int fgpu_stage3_set_junctions(fgpu_ctx* ctx, const uint64_t* keys_host, const fgpu_junction* recs_host, uint64_t n) {
    if (!ctx || (n && (!keys_host || !recs_host))) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_set_junctions while a pass is open"; return FGPU_ERR_STATE; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    ctx->s3_ready = false;
    uint64_t cap = 1024;
    while (cap < 2 * n + 2) cap <<= 1;
    int rc;
    if ((rc = fgpu_ensure(ctx, &ctx->s3_keys, cap * 8))) return rc;
    if ((rc = fgpu_ensure(ctx, &ctx->s3_dist, cap * 8))) return rc;
    if ((rc = fgpu_ensure(ctx, &ctx->s3_cov, cap * 8))) return rc;
    if ((rc = fgpu_ensure(ctx, &ctx->s3_in, n * (8 + sizeof(fgpu_junction)) + 64))) return rc;
    ctx->s3_mask = cap - 1;
    ctx->s3_count = 0;
    FGPU_HIP(hipMemsetAsync(ctx->s3_keys.p, 0xFF, cap * 8, ctx->stream));
    FGPU_HIP(hipMemsetAsync(ctx->s3_in.p, 0, 64, ctx->stream));
    if (n) {
        uint64_t* d_keys = (uint64_t*)((char*)ctx->s3_in.p + 64);
        fgpu_junction* d_recs = (fgpu_junction*)(d_keys + n);
        FGPU_HIP(hipMemcpyAsync(d_keys, keys_host, n * 8, hipMemcpyHostToDevice, ctx->stream));
        FGPU_HIP(hipMemcpyAsync(d_recs, recs_host, n * sizeof(fgpu_junction), hipMemcpyHostToDevice, ctx->stream));
        FGPU_LAUNCH("s3_build", k_s3_build, fgpu_blocks(n, 256), 256, (const uint64_t*)d_keys, (const fgpu_junction*)d_recs, n,
                    (unsigned long long*)ctx->s3_keys.p, (uint64_t*)ctx->s3_dist.p, (uint64_t*)ctx->s3_cov.p, ctx->s3_mask, (unsigned int*)ctx->s3_in.p);
    }
    unsigned int repeated = 0;
    FGPU_HIP(hipMemcpyAsync(&repeated, ctx->s3_in.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    if (repeated) { ctx->err = "fgpu_stage3_set_junctions: a k-mer occurs more than once"; return FGPU_ERR_ARG; }
    ctx->s3_count = n;
    ctx->s3_ready = true;
    return FGPU_OK;
}

// longest contig string a walk can return: the start (k + 1 bases) and one base per step, two half steps of distance each, up to
// maxDist (a byte) + 2 * max_read_length (:376)
extern "C" uint64_t fgpu_stage3_contig_words(int32_t k, int32_t max_read_length) {
    const uint64_t bases = (uint64_t)k + 1 + (255 + 2 * (uint64_t)max_read_length) / 2 + 2;
    return (bases + 31) / 32;
}

extern "C" int fgpu_stage3_find_neighbors(fgpu_ctx* ctx, const uint64_t* start_kmers_host, const int8_t* indices_host, uint64_t n,
                                          int32_t max_read_length, fgpu_neighbor* out, uint64_t* n_probes, uint64_t* contigs_out,
                                          uint64_t contig_stride_words) {
    if (!ctx || (n && (!start_kmers_host || !indices_host || !out)) || max_read_length < 1) return FGPU_ERR_ARG;
    if (contigs_out && contig_stride_words < fgpu_stage3_contig_words(ctx->prm.k, max_read_length)) {
        ctx->err = "fgpu_stage3_find_neighbors: contig_stride_words is less than fgpu_stage3_contig_words(k, max_read_length)";
        return FGPU_ERR_ARG;
    }
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_find_neighbors while a pass is open"; return FGPU_ERR_STATE; }
    if (!ctx->s3_ready) { ctx->err = "fgpu_stage3_find_neighbors before fgpu_stage3_set_junctions"; return FGPU_ERR_STATE; }
    if (n_probes) *n_probes = 0;
    if (!n) return FGPU_OK;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    int rc;
    const uint64_t in_bytes = (n * 9 + 15) & ~15ULL;
    const uint64_t stride = contigs_out ? contig_stride_words : 0;
    if ((rc = fgpu_ensure(ctx, &ctx->probe_buf, 64 + in_bytes + n * sizeof(fgpu_neighbor) + n * stride * 8))) return rc;
    char* base = (char*)ctx->probe_buf.p;
    unsigned long long* d_probes = (unsigned long long*)base;
    uint64_t* d_starts = (uint64_t*)(base + 64);
    signed char* d_idx = (signed char*)(d_starts + n);
    fgpu_neighbor* d_out = (fgpu_neighbor*)(base + 64 + in_bytes);
    uint64_t* d_contigs = stride ? (uint64_t*)(d_out + n) : nullptr;
    FGPU_HIP(hipMemsetAsync(d_probes, 0, 8, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_starts, start_kmers_host, n * 8, hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_idx, indices_host, n, hipMemcpyHostToDevice, ctx->stream));
    FGPU_LAUNCH("s3_find_neighbors", k_s3_find_neighbors, fgpu_blocks(n, 256), 256, (const uint64_t*)d_starts, (const signed char*)d_idx, n, ctx->fd,
                (const uint32_t*)ctx->bloo2, (const uint64_t*)ctx->s3_keys.p, (const uint64_t*)ctx->s3_dist.p, ctx->s3_mask, (int)max_read_length, d_out,
                d_probes, d_contigs, stride);
    unsigned long long probes = 0;
    FGPU_HIP(hipMemcpyAsync(out, d_out, n * sizeof(fgpu_neighbor), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&probes, d_probes, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (stride) FGPU_HIP(hipMemcpyAsync(contigs_out, d_contigs, n * stride * 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    if (n_probes) *n_probes = probes;
    return FGPU_OK;
}

namespace {
struct S3Scratch {                                         // device memory of one call, gone when it returns
    void* p = nullptr;
    ~S3Scratch() { if (p) (void)hipFree(p); }
};
inline uint64_t s3c_take(uint64_t& at, uint64_t bytes) {   // carve `bytes` out of one allocation, every part 16-byte aligned
    const uint64_t here = at;
    at += (bytes + 15) & ~15ULL;
    return here;
}
int s3c_alloc(fgpu_ctx* ctx, void** p, uint64_t bytes, const char* what) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        *p = nullptr;
        ctx->err = std::string("fgpu_stage3_contigs: hipMalloc of ") + std::to_string(bytes) + " bytes (" + what + ") failed: " + hipGetErrorString(e);
        return FGPU_ERR_NOMEM;
    }
    return FGPU_OK;
}
}  // namespace

extern "C" int fgpu_stage3_contigs(fgpu_ctx* ctx, const uint64_t* start_kmers_host, const int8_t* indices_host, uint64_t n, int32_t max_read_length,
                                   fgpu_contig* out, uint64_t totals[3], uint64_t* n_probes) {
    if (!ctx || !totals || (n && (!start_kmers_host || !indices_host || !out)) || max_read_length < 1) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_contigs while a pass is open"; return FGPU_ERR_STATE; }
    if (!ctx->s3_ready) { ctx->err = "fgpu_stage3_contigs before fgpu_stage3_set_junctions"; return FGPU_ERR_STATE; }
    const uint64_t nj = ctx->s3_count, states = 2 * nj + n;
    if (nj >= (1ULL << 31) || n >= (1ULL << 31) || states >= 0xFFFFFFFFULL) {
        ctx->err = "fgpu_stage3_contigs: two states per junction and one per start have to fit 32 bits";
        return FGPU_ERR_ARG;
    }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->s3c_out) {                                    // results nobody took
        FGPU_HIP(hipFree(ctx->s3c_out));
        ctx->s3c_out = nullptr;
    }
    totals[0] = totals[1] = totals[2] = ctx->s3c_totals[0] = ctx->s3c_totals[1] = ctx->s3c_totals[2] = 0;
    if (n_probes) *n_probes = 0;
    if (!n) return FGPU_OK;
    const int k = ctx->prm.k;
    const uint64_t stride = fgpu_stage3_contig_words(k, max_read_length);
    size_t scan_bytes = 0;
    FGPU_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t at = 0;
    const uint64_t o_probes = s3c_take(at, 16), o_starts = s3c_take(at, n * 8), o_idx = s3c_take(at, n), o_seg = s3c_take(at, states * sizeof(fgpu_neighbor)),
                   o_link = s3c_take(at, states * sizeof(S3Link)), o_info = s3c_take(at, n * 8), o_chain = s3c_take(at, n * sizeof(fgpu_contig)),
                   o_cnt = s3c_take(at, 3 * (n + 1) * 8), o_off = s3c_take(at, 3 * (n + 1) * 8), o_scan = s3c_take(at, scan_bytes), o_text = s3c_take(at, states * stride * 8);
    S3Scratch work;
    int rc;
    if ((rc = s3c_alloc(ctx, &work.p, at, "the segments"))) return rc;
    char* base = (char*)work.p;
    unsigned long long* d_probes = (unsigned long long*)(base + o_probes);
    uint64_t* d_starts = (uint64_t*)(base + o_starts);
    signed char* d_idx = (signed char*)(base + o_idx);
    fgpu_neighbor* d_seg = (fgpu_neighbor*)(base + o_seg);
    S3Link* d_link = (S3Link*)(base + o_link);
    uint64_t* d_info = (uint64_t*)(base + o_info);
    fgpu_contig* d_chain = (fgpu_contig*)(base + o_chain);
    uint64_t *d_words = (uint64_t*)(base + o_cnt), *d_segs = d_words + (n + 1), *d_covs = d_segs + (n + 1);      // counts per chain, and a zero behind them
    uint64_t *d_word0 = (uint64_t*)(base + o_off), *d_seg0 = d_word0 + (n + 1), *d_cov0 = d_seg0 + (n + 1);      // their exclusive sums: entry n is the total
    uint64_t* d_text = (uint64_t*)(base + o_text);
    const uint64_t* d_keys = (const uint64_t*)((const char*)ctx->s3_in.p + 64);
    const fgpu_junction* d_recs = (const fgpu_junction*)(d_keys + nj);
    const uint64_t *tkeys = (const uint64_t*)ctx->s3_keys.p, *tdist = (const uint64_t*)ctx->s3_dist.p, *tcov = (const uint64_t*)ctx->s3_cov.p;
    FGPU_HIP(hipMemsetAsync(d_probes, 0, 16, ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_words, 0, 3 * (n + 1) * 8, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_starts, start_kmers_host, n * 8, hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(d_idx, indices_host, n, hipMemcpyHostToDevice, ctx->stream));
    FGPU_LAUNCH("s3c_segments", k_s3c_segments, fgpu_blocks(states, 256), 256, d_keys, d_recs, nj, (const uint64_t*)d_starts, (const signed char*)d_idx, n, ctx->fd,
                (const uint32_t*)ctx->bloo2, tkeys, tdist, ctx->s3_mask, (int)max_read_length, d_seg, d_probes, d_text, stride);
    FGPU_LAUNCH("s3c_link", k_s3c_link, fgpu_blocks(states, 256), 256, (const fgpu_neighbor*)d_seg, nj, n, k, (const uint64_t*)d_starts, (const signed char*)d_idx,
                tkeys, tcov, ctx->s3_mask, ctx->fd.kmask, d_link, d_info);
    FGPU_LAUNCH("s3c_follow", k_s3c_follow<false>, fgpu_blocks(n, 256), 256, (const S3Link*)d_link, (const uint64_t*)d_info, (const signed char*)d_idx,
                (const fgpu_neighbor*)d_seg, nj, n, k, d_chain, d_words, d_segs, d_covs, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint8_t*)nullptr, (uint8_t*)nullptr);
    for (int i = 0; i < 3; i++)
        FGPU_HIP(rocprim::exclusive_scan(base + o_scan, scan_bytes, d_words + i * (n + 1), d_word0 + i * (n + 1), (uint64_t)0, n + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t tot[3] = {0, 0, 0};
    unsigned long long probes = 0;
    for (int i = 0; i < 3; i++) FGPU_HIP(hipMemcpyAsync(&tot[i], d_word0 + i * (n + 1) + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&probes, d_probes, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    // the arrays the caller takes: text | segment k-mers | distances | coverages; and, for the gather only, each segment's state and base offset
    uint64_t oat = 0;
    const uint64_t q_text = s3c_take(oat, tot[0] * 8), q_kmers = s3c_take(oat, tot[1] * 8), q_dist = s3c_take(oat, tot[1]), q_cov = s3c_take(oat, tot[2]);
    (void)q_text;
    uint64_t gat = 0;
    const uint64_t g_state = s3c_take(gat, tot[1] * 4), g_off = s3c_take(gat, tot[1] * 4);
    S3Scratch place;
    void* res = nullptr;
    if ((rc = s3c_alloc(ctx, &place.p, gat, "the segment lists"))) return rc;
    if ((rc = s3c_alloc(ctx, &res, oat, "the results"))) return rc;
    ctx->s3c_out = res;                                    // (freed with the context from here on)
    uint32_t *d_state = (uint32_t*)((char*)place.p + g_state), *d_off = (uint32_t*)((char*)place.p + g_off);
    uint64_t *r_text = (uint64_t*)res, *r_kmers = (uint64_t*)((char*)res + q_kmers);
    uint8_t *r_dist = (uint8_t*)res + q_dist, *r_cov = (uint8_t*)res + q_cov;
    FGPU_LAUNCH("s3c_follow", k_s3c_follow<true>, fgpu_blocks(n, 256), 256, (const S3Link*)d_link, (const uint64_t*)d_info, (const signed char*)d_idx,
                (const fgpu_neighbor*)d_seg, nj, n, k, d_chain, d_word0, d_seg0, d_cov0, d_state, d_off, r_dist, r_cov);
    if (tot[0])
        FGPU_LAUNCH("s3c_gather", k_s3c_gather_text, fgpu_blocks(tot[0], 256), 256, (const fgpu_contig*)d_chain, n, tot[0], (const uint64_t*)d_starts, k, ctx->fd.kmask,
                    (const uint32_t*)d_state, (const uint32_t*)d_off, (const S3Link*)d_link, (const uint64_t*)d_text, stride, r_text);
    if (tot[1])
        FGPU_LAUNCH("s3c_gather", k_s3c_gather_kmers, fgpu_blocks(tot[1], 256), 256, (const uint32_t*)d_state, (const fgpu_neighbor*)d_seg, tot[1], r_kmers);
    FGPU_HIP(hipMemcpyAsync(out, d_chain, n * sizeof(fgpu_contig), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    for (int i = 0; i < 3; i++) totals[i] = ctx->s3c_totals[i] = tot[i];
    if (n_probes) *n_probes = probes;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_contigs_take(fgpu_ctx* ctx, uint64_t* text, uint64_t text_words, uint64_t* seg_kmers, uint8_t* seg_dist, uint64_t n_seg,
                                        uint8_t* cov, uint64_t n_cov) {
    if (!ctx) return FGPU_ERR_ARG;
    const uint64_t* tot = ctx->s3c_totals;
    if (text_words < tot[0] || n_seg < tot[1] || n_cov < tot[2] || (tot[0] && !text) || (tot[1] && (!seg_kmers || !seg_dist)) || (tot[2] && !cov)) {
        ctx->err = "fgpu_stage3_contigs_take: an array is smaller than the totals fgpu_stage3_contigs gave";
        return FGPU_ERR_ARG;
    }
    if (!ctx->s3c_out) return FGPU_OK;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    uint64_t at = 0;
    const uint64_t q_text = s3c_take(at, tot[0] * 8), q_kmers = s3c_take(at, tot[1] * 8), q_dist = s3c_take(at, tot[1]), q_cov = s3c_take(at, tot[2]);
    const char* res = (const char*)ctx->s3c_out;
    if (tot[0]) FGPU_HIP(hipMemcpyAsync(text, res + q_text, tot[0] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tot[1]) FGPU_HIP(hipMemcpyAsync(seg_kmers, res + q_kmers, tot[1] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tot[1]) FGPU_HIP(hipMemcpyAsync(seg_dist, res + q_dist, tot[1], hipMemcpyDeviceToHost, ctx->stream));
    if (tot[2]) FGPU_HIP(hipMemcpyAsync(cov, res + q_cov, tot[2], hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    FGPU_HIP(hipFree(ctx->s3c_out));
    ctx->s3c_out = nullptr;
    ctx->s3c_totals[0] = ctx->s3c_totals[1] = ctx->s3c_totals[2] = 0;
    return FGPU_OK;
}
