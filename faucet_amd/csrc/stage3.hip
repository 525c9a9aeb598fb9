// stage3.hip — JunctionMap::findNeighbor (utils/JunctionMap.cpp:231-412) for many (junction, extension) pairs at once, whole walks on the
// device.
//
// The reference's contig-graph stage (not part of this build) starts a walk at every junction along every extension it builds a contig on:
// getValidJExtension (:474-490; 4 x (Bloom::oldContains + JChecker::jcheck)) names the one next base, the DoubleKmer advances, the junction
// map is asked twice per step (backward- and forward-facing half step), until a junction or a sink is reached.  One call is a chain of
// dependent filter probes; different calls are independent -- one lane per walk.  The junction map the walks look into is handed over by the
// caller (fgpu_stage3_set_junctions: the scan's own result, or a parsed .junctions file) and kept as an open-addressing table in HBM: k-mer
// -> the five distances, which is all findNeighbor reads of a Junction.  The second half of the file chains such walks into whole
// JunctionMap::getContig calls (:133-221) for many starts at once (fgpu_stage3_contigs); for that the table holds the four coverages too.  The
// third part is JunctionMap::buildContigGraph's order of such calls (:11-129), every call on the map as the calls before it left it
// (fgpu_stage3_build).
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
//
// `map` answers junctionMap.find: S3Static is the table as it stands; S3View (the graph build below) is the table as one getContig call sees it
// at its time -- a compile-time variant, so the static kernels keep their code.
struct S3Static {
    const uint64_t* __restrict__ tkeys;
    const uint64_t* __restrict__ tdist;
    uint64_t mask;
    __device__ __forceinline__ bool find(uint64_t key, uint64_t& dist) const { return s3_find(tkeys, tdist, mask, key, dist); }
};

template <class Map>
__device__ __forceinline__ fgpu_neighbor s3_walk(uint64_t start, int idx, const FdParams& fp, const uint32_t* __restrict__ bloom, const Map& map,
                                                 int max_read_length, uint64_t* __restrict__ text, uint64_t stride, unsigned long long& probes) {
    fgpu_neighbor res;
    res.kmer = 0; res.dist = 0; res.len = 0; res.node = 0; res.rindex = 0; res.abort = 0; res.reserved = 0; res.reserved2 = 0;
    {
        const int k = fp.k;
        uint64_t km = start & fp.kmask, rc = fd_revcomp(km, k);
        fgpu_neighbor sink = res;
        uint64_t packed = 0;
        bool done = false;
        if (idx < 0 || idx > 4 || !map.find(km, packed)) {
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
                if (map.find(km, other)) finish(km, 1, 4, 1, ln);
            } else {
                lastnuc = (int)(rc & 3);
                emit((int)((km >> (2 * (k - 1))) & 3));
                forward(idx);
                ln = 1 + k;
                emit_kmer(km);
                if (map.find(rc, other)) finish(rc, 1, lastnuc, 1, ln);
                else if (maxd == 1) finish(rc, 0, lastnuc, 1, ln);
                else {
                    dist = 2;
                    if (map.find(km, other)) finish(km, 1, 4, 2, ln);
                }
            }
            if (!done && dist > maxd) { res.abort = 1; done = true; }   // the reference's assert(dist <= maxDist)
        }
        while (!done) {
            // ---- leaving the first loop (:343-366): a junction exactly where expected, else this is (probably) a sink
            if (phase == 0 && dist >= maxd) {
                if (map.find(km, other)) { finish(km, 1, retidx, dist, ln); break; }
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
            bool isj = map.find(km, other);
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
            isj = map.find(km, other);
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
    if (w < n) out[w] = s3_walk(starts[w], indices[w], fp, bloom, S3Static{tkeys, tdist, mask}, max_read_length, contigs ? contigs + w * stride : nullptr, stride, probes);
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
        if (s >= 2 * nj || idx >= 0) seg[s] = s3_walk(start, idx, fp, bloom, S3Static{tkeys, tdist, mask}, max_read_length, text + s * stride, stride, probes);
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
    if (ctx->s3b_out) {                                    // ... of a build
        FGPU_HIP(hipFree(ctx->s3b_out));
        ctx->s3b_out = nullptr;
        for (int i = 0; i < 4; i++) ctx->s3b_totals[i] = 0;
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

namespace {

// ---- JunctionMap::buildContigGraph (utils/JunctionMap.cpp:11-129): every getContig call of the build, each on the map as it stands then -----
// The build is a strict order of getContig calls -- buildBranchingPaths' map-order loop (:36-77), destroyComplexJunctions (:90-102),
// buildLinearRegions' loop (:105-124) -- and each call erases the inner junctions of its chain behind itself (:210-216), so what a call
// finds depends on the calls before it.  Every call the reference COULD make gets its place in that order as its time t: the branching
// starts in map order, one slot for destroyComplexJunctions, then two per junction with one path out.  Two arrays hold what earlier calls
// did to later ones: dead_at[slot], the time of the call that erased the junction in that table slot (S3B_NEVER: nobody; a complex
// junction: the destroy slot), and claim_at[5 * row + i], the time of the call whose contig took contigs[i] of that junction's node
// (Contig::setEnds, src/Contig.cpp:123-133).  A call at time t sees a junction iff dead_at >= t (its own kills carry its own time), and is
// made iff its start is seen and, in the branching phase, claim_at of its (node, index) is >= t (:50).
//
// Timestamped fixed point (as pairs.hip and k_ovw_round): a round evaluates calls under the arrays of the round
// before, then rebuilds both arrays with atomicMin from the calls that are made and return.  A call keeps every table hit of its walks
// with what it saw there (S3Dep); it is evaluated again only when one of those looks different or when it newly becomes a made call.
// Whether dead_at[j] < t depends on calls before t alone, so the earliest call that is still wrong sees final state in the next round:
// at least one more call is final per round, and the fixed point is the sequential run.

constexpr uint32_t S3B_NEVER = 0xFFFFFFFFu;
enum { S3B_SEEN = 1, S3B_KILL = 2 };

struct __attribute__((aligned(16))) S3Dep {                // one table hit of one evaluation of one call
    uint32_t call, slot, gen, flags;                       // S3B_SEEN: the junction was visible; S3B_KILL: this call erases it behind its loop
};
struct __attribute__((aligned(8))) S3Call {                // one time slot of the build
    uint32_t row, slot;                                    // the start junction: its row in the caller's arrays, its table slot
    int8_t idx;                                            // -1: no call (the destroy slot)
    uint8_t phase;                                         // FGPU_BUILD_BRANCHING / _LINEAR_FORWARD / _LINEAR_BACKWARD
    uint8_t cov0;                                          // junc.getCoverage(startIndex) of the start's own copy (:43-47, :148)
    uint8_t reserved;
    uint32_t reserved2;
};
struct __attribute__((aligned(8))) S3Res {                 // what the last evaluation of a call gave
    uint64_t end_kmer, far_kmer;                           // BfSearchResult::kmer of the last segment; Contig::getSideKmer(2)
    uint32_t far_slot;                                     // far_kmer's table slot, S3B_NEVER: not in the table
    uint32_t len, n_seg, n_cov, gen;
    int8_t ind2, end_node, status;
    uint8_t valid;                                         // the evaluation still stands
    uint8_t far_junction, far_start, reserved, reserved2;  // isJunction(far_kmer) behind the call's own kills (:56); far_kmer == kmer (:58)
    uint32_t reserved3;
};

__device__ __forceinline__ uint32_t s3b_slot_of(const uint64_t* __restrict__ tkeys, uint64_t mask, uint64_t key) {
    uint64_t s = s3_slot(key, mask);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const uint64_t k = tkeys[s];
        if (k == key) return (uint32_t)s;
        if (k == S3_EMPTY) return S3B_NEVER;
        s = (s + 1) & mask;
    }
    return S3B_NEVER;
}

// the table as the call at time t sees it; every hit is noted for the fixed point (deps == nullptr: the placing pass, nothing is noted)
struct S3View {
    const uint64_t* __restrict__ tkeys;
    const uint64_t* __restrict__ tdist;
    uint64_t mask;
    const uint32_t* __restrict__ dead;
    uint32_t t, gen;
    S3Dep* __restrict__ deps;
    unsigned long long* __restrict__ dep_top;
    uint64_t dep_cap;
    __device__ __forceinline__ void note(uint32_t slot, uint32_t flags) const {
        if (!deps) return;
        const unsigned long long i = atomicAdd(dep_top, 1ULL);
        if (i < dep_cap) { S3Dep d; d.call = t; d.slot = slot; d.gen = gen; d.flags = flags; deps[i] = d; }
    }
    __device__ __forceinline__ bool find(uint64_t key, uint64_t& dist) const {
        const uint32_t s = s3b_slot_of(tkeys, mask, key);
        if (s == S3B_NEVER) return false;
        const bool seen = dead[s] >= t;
        note(s, seen ? S3B_SEEN : 0);
        if (seen) dist = tdist[s];
        return seen;
    }
};

__device__ __forceinline__ uint32_t s3b_start_cov(uint64_t key, uint32_t cov, int k, uint64_t kmask) {   // the start's own copy in the branching phase, :43-47
    const uint64_t b = key >> (2 * (k - 1));
    if (key == b * (kmask / 3)) cov &= ~(0xFFu << (8 * b));
    return cov;
}

// one lane per junction: the calls it can start -- branching: its covered indices 0..4 (:49-50); linear: its covered extension, then 4 (:111-118)
__global__ void __launch_bounds__(256) k_s3b_count(const uint64_t* __restrict__ keys, const fgpu_junction* __restrict__ recs, uint64_t nj, int k, uint64_t kmask,
                                                   uint64_t* __restrict__ n_branch, uint64_t* __restrict__ n_linear) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nj) return;
    uint32_t cov = s3c_cov_of(recs[r]);
    const int paths = s3c_paths_out(cov);
    uint64_t nb = 0;
    if (paths > 1) {
        cov = s3b_start_cov(keys[r], cov, k, kmask);
        nb = s3c_paths_out(cov) + (cov ? 1 : 0);
    }
    n_branch[r] = nb;
    n_linear[r] = paths == 1 ? 2 : 0;
}

__global__ void __launch_bounds__(256) k_s3b_list(const uint64_t* __restrict__ keys, const fgpu_junction* __restrict__ recs, uint64_t nj, int k, uint64_t kmask,
                                                  const uint64_t* __restrict__ branch0, const uint64_t* __restrict__ linear0,
                                                  const uint64_t* __restrict__ tkeys, uint64_t mask, S3Call* __restrict__ calls, uint32_t* __restrict__ row_slot) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nj) return;
    const uint64_t nb = branch0[nj];                       // the destroy slot's time
    S3Call c;
    c.row = 0; c.slot = S3B_NEVER; c.idx = -1; c.phase = 0; c.cov0 = 0; c.reserved = 0; c.reserved2 = 0;
    if (r == nj) { calls[nb] = c; return; }
    const uint64_t key = keys[r];
    uint32_t cov = s3c_cov_of(recs[r]);
    const int paths = s3c_paths_out(cov);
    c.row = (uint32_t)r;
    c.slot = s3b_slot_of(tkeys, mask, key);
    row_slot[r] = c.slot;
    if (c.slot == S3B_NEVER) return;                       // (every key is in the table: fgpu_stage3_set_junctions)
    if (paths > 1) {
        cov = s3b_start_cov(key, cov, k, kmask);
        uint64_t t = branch0[r];
        c.phase = FGPU_BUILD_BRANCHING;
        for (int i = 0; i < 5; i++)
            if (i < 4 ? ((cov >> (8 * i)) & 0xFF) != 0 : cov != 0) { c.idx = (int8_t)i; c.cov0 = s3c_coverage(cov, i); calls[t++] = c; }
    } else if (paths == 1) {
        const uint64_t t = nb + 1 + linear0[r];
        c.idx = (int8_t)s3c_covered(cov); c.phase = FGPU_BUILD_LINEAR_FORWARD; c.cov0 = s3c_coverage(cov, c.idx);
        calls[t] = c;
        c.idx = 4; c.phase = FGPU_BUILD_LINEAR_BACKWARD; c.cov0 = s3c_coverage(cov, 4);
        calls[t + 1] = c;
    }
}

// base b of a walk's string
__device__ __forceinline__ int s3b_base(const uint64_t* __restrict__ text, uint32_t b) { return (int)((text[b >> 5] >> (2 * (b & 31))) & 3); }

// one lane per getContig call (:133-221), the whole chain in the lane under its view.  PLACE false: a call that is made and has no standing
// evaluation -- status, end, counts, Contig::getSideKmer(2) (src/Contig.cpp:235-239, from the string), and the table hits and kills as S3Dep.
// PLACE true (the arrays are final, the sizes scanned): the calls that are output write their string, segment k-mers, distances and
// coverages in place.  A chain that never ends is found by Brent's method on (junction, entered forward or backward) in hops proportional
// to its own tail and cycle; the hop bound behind it only states that the loop is finite.
template <bool PLACE>
__global__ void __launch_bounds__(256) k_s3b_chain(const S3Call* __restrict__ calls, uint64_t n_calls, const uint64_t* __restrict__ keys, uint64_t nj,
                                                   const uint8_t* __restrict__ made, S3Res* __restrict__ res, uint32_t gen,
                                                   FdParams fp, const uint32_t* __restrict__ bloom, const uint64_t* __restrict__ tkeys,
                                                   const uint64_t* __restrict__ tdist, const uint64_t* __restrict__ tcov, uint64_t mask,
                                                   const uint32_t* __restrict__ dead, int max_read_length, uint64_t* __restrict__ walk_text, uint64_t stride,
                                                   S3Dep* __restrict__ deps, unsigned long long* __restrict__ counters, uint64_t dep_cap,
                                                   const uint64_t* __restrict__ out_at, const uint64_t* __restrict__ word0, const uint64_t* __restrict__ seg0,
                                                   const uint64_t* __restrict__ cov0, fgpu_contig* __restrict__ out, fgpu_build_call* __restrict__ out_calls,
                                                   uint64_t* __restrict__ out_text, uint64_t* __restrict__ out_kmers, uint8_t* __restrict__ out_dist,
                                                   uint8_t* __restrict__ out_cov) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long probes = 0;
    bool run = c < n_calls;
    S3Call call = {};
    if (run) { call = calls[c]; run = call.idx >= 0; }
    if (run) run = PLACE ? out_at[c + 1] != out_at[c] : (made[c] && !res[c].valid);
    if (run) {
        const int k = fp.k;
        const uint64_t start = keys[call.row];
        S3View view;
        view.tkeys = tkeys; view.tdist = tdist; view.mask = mask; view.dead = dead; view.t = (uint32_t)c; view.gen = gen;
        view.deps = PLACE ? nullptr : deps; view.dep_top = counters; view.dep_cap = dep_cap;
        uint64_t* text = walk_text + c * stride;
        uint64_t km = start, tail = call.idx == 4 ? fd_revcomp(start, k) : start;      // :149-151; the last k bases of contigString
        int idx = call.idx;
        uint32_t len = (uint32_t)k, n_seg = 0, n_cov = 1;
        int status = 0;
        fgpu_neighbor r = {};
        uint32_t saved = S3B_NEVER, power = 1, lam = 0;
        // the placing pass: where this call's output goes, and the string under way
        // (every write is held within the sizes the scan gave this call)
        uint64_t o = 0, seg_at = 0, seg_end = 0, cov_at = 0, cov_end = 0, words = 0, acc = 0, *otext = nullptr;
        uint32_t pos = 0;
        auto emit = [&](int code) {
            acc |= (uint64_t)code << (2 * (pos & 31));
            pos++;
            if ((pos & 31) == 0) {
                if ((pos >> 5) <= words) otext[(pos >> 5) - 1] = acc;
                acc = 0;
            }
        };
        if (PLACE) {
            o = out_at[c]; seg_at = seg0[o]; seg_end = seg0[o + 1]; cov_at = cov0[o]; cov_end = cov0[o + 1]; otext = out_text + word0[o]; words = word0[o + 1] - word0[o];
            for (int i = k - 1; i >= 0; i--) emit((int)((tail >> (2 * i)) & 3));
            if (cov_at < cov_end) out_cov[cov_at++] = call.cov0;
        }
        const uint64_t max_hops = 6 * nj + 16;
        for (uint64_t hop = 0;; hop++) {                                                 // :157
            if (hop >= max_hops) { status = 3; break; }
            r = s3_walk(km, idx, fp, bloom, view, max_read_length, text, stride, probes);     // :158
            if (r.abort) { status = 1; break; }
            const uint32_t add = r.len > k ? (uint32_t)(r.len - k) : 0u;                 // :160-162
            for (uint32_t b = (uint32_t)k + (PLACE ? 0u : add - min(add, (uint32_t)k)); b < (uint32_t)k + add; b++) {
                const int code = s3b_base(text, b);
                tail = ((tail << 2) | (uint64_t)code) & fp.kmask;
                if (PLACE) emit(code);
            }
            if (PLACE && seg_at < seg_end) { out_kmers[seg_at] = r.kmer; out_dist[seg_at] = (uint8_t)r.dist; seg_at++; }     // :163
            n_seg++;
            len += add;
            if (!r.node) break;                                                          // :193-196
            const uint32_t slot = s3b_slot_of(tkeys, mask, r.kmer);                     // *getJunction(result.kmer), :167
            if (slot == S3B_NEVER) { status = 1; break; }
            const uint32_t cov = (uint32_t)tcov[slot];
            if (PLACE && cov_at < cov_end) out_cov[cov_at++] = s3c_coverage(cov, r.rindex);   // :169
            n_cov++;
            if (s3c_paths_out(cov) != 1) break;                                          // :188-191
            km = r.kmer;
            idx = r.rindex < 4 ? 4 : s3c_covered(cov);                                  // getOppositeIndex, :174
            if (r.kmer == start) break;                                                  // :177-180
            view.note(slot, S3B_SEEN | S3B_KILL);                                        // :185
            const uint32_t state = 2 * slot + (idx == 4 ? 0u : 1u);
            if (state == saved) { status = 3; break; }
            if (++lam == power) { saved = state; power <<= 1; lam = 0; }
        }
        if (PLACE) {
            if ((pos & 31) && (pos >> 5) < words) otext[pos >> 5] = acc;
            const S3Res e = res[c];
            fgpu_contig oc;
            oc.end_kmer = e.end_kmer; oc.text_word = word0[o]; oc.seg_first = seg0[o]; oc.cov_first = cov0[o]; oc.len = e.len; oc.n_seg = e.n_seg; oc.n_cov = e.n_cov;
            oc.ind1 = call.idx; oc.ind2 = e.ind2; oc.end_node = e.end_node; oc.status = 0;
            out[o] = oc;
            fgpu_build_call bc;
            bc.start_kmer = start; bc.far_kmer = e.far_kmer; bc.time = (uint32_t)c; bc.phase = call.phase; bc.far_is_junction = e.far_junction;
            bc.far_is_start = e.far_start; bc.reserved = 0;
            out_calls[o] = bc;
        } else {
            S3Res e;
            e.end_kmer = 0; e.far_kmer = 0; e.far_slot = S3B_NEVER; e.len = 0; e.n_seg = 0; e.n_cov = 0; e.gen = gen; e.ind2 = 0; e.end_node = 0;
            e.status = (int8_t)status; e.valid = 1; e.far_junction = 0; e.far_start = 0; e.reserved = 0; e.reserved2 = 0; e.reserved3 = 0;
            if (!status) {
                e.end_kmer = r.kmer; e.len = len; e.n_seg = n_seg; e.n_cov = n_cov;
                e.end_node = r.node ? 1 : 0;
                e.ind2 = r.node ? r.rindex : 4;                                          // setIndices, :201-208
                e.far_kmer = e.ind2 == 4 ? tail : fd_revcomp(tail, k);                   // Contig::getSideKmer(2)
                e.far_slot = s3b_slot_of(tkeys, mask, e.far_kmer);
            }
            res[c] = e;
        }
    }
    if (!PLACE) {
        for (int off = 32; off; off >>= 1) probes += __shfl_down(probes, off);
        if ((threadIdx.x & 63) == 0 && probes) atomicAdd(counters + 1, probes);
        if (run) atomicAdd(counters + 2, 1ULL);
    }
}

// dead_at and claim_at again: destroyComplexJunctions' time for the complex junctions (no call's doing: it stands from the first round on),
// nobody for the others, no claim ...
__global__ void __launch_bounds__(256) k_s3b_seed(const fgpu_junction* __restrict__ recs, const uint32_t* __restrict__ row_slot, uint64_t nj, uint64_t destroy_time,
                                                  uint32_t* __restrict__ dead, uint32_t* __restrict__ claim) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nj) return;
    const uint32_t slot = row_slot[r];
    if (slot != S3B_NEVER) dead[slot] = s3c_paths_out(s3c_cov_of(recs[r])) > 1 ? (uint32_t)destroy_time : S3B_NEVER;
    for (int i = 0; i < 5; i++) claim[5 * r + i] = S3B_NEVER;
}

// ... and the kills of every call that is made and returns, from its standing evaluation
__global__ void __launch_bounds__(256) k_s3b_kills(const S3Dep* __restrict__ deps, uint64_t n_deps, const S3Res* __restrict__ res, const uint8_t* __restrict__ made,
                                                   uint32_t* __restrict__ dead) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_deps) return;
    const S3Dep d = deps[i];
    if (!(d.flags & S3B_KILL) || !made[d.call]) return;
    const S3Res e = res[d.call];
    if (e.valid && e.gen == d.gen && e.status == 0) atomicMin(&dead[d.slot], d.call);
}

// isJunction(far_kmer) on the map behind the call's own kills (:54-56) and the claims of Contig::setEnds (:58-74; src/Contig.cpp:123-133)
__global__ void __launch_bounds__(256) k_s3b_claims(const S3Call* __restrict__ calls, uint64_t n_calls, S3Res* __restrict__ res, const uint8_t* __restrict__ made,
                                                    const uint64_t* __restrict__ tcov, const uint32_t* __restrict__ dead, uint32_t* __restrict__ claim) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls) return;
    const S3Call call = calls[c];
    if (call.idx < 0 || !made[c]) return;
    S3Res e = res[c];
    if (!e.valid || e.status) return;
    e.far_junction = e.far_slot != S3B_NEVER && dead[e.far_slot] > (uint32_t)c;
    e.far_start = e.far_junction && e.far_slot == call.slot;
    res[c] = e;
    if (call.phase != FGPU_BUILD_BRANCHING) return;        // (buildLinearRegions sets no ends)
    atomicMin(&claim[5 * (uint64_t)call.row + call.idx], (uint32_t)c);
    if (e.far_junction) {
        const uint64_t far_row = tcov[e.far_slot] >> 32;
        if (s3c_paths_out((uint32_t)tcov[e.far_slot]) > 1) atomicMin(&claim[5 * far_row + e.ind2], (uint32_t)c);   // (only complex junctions start branching calls)
    }
}

// an evaluation stands as long as every table hit of it looks as it did
__global__ void __launch_bounds__(256) k_s3b_check(const S3Dep* __restrict__ deps, uint64_t n_deps, S3Res* __restrict__ res, const uint32_t* __restrict__ dead) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_deps) return;
    const S3Dep d = deps[i];
    const S3Res e = res[d.call];
    if (!e.valid || e.gen != d.gen) return;
    const bool seen = dead[d.slot] >= d.call;
    if (seen != ((d.flags & S3B_SEEN) != 0)) res[d.call].valid = 0;
}

// which calls are made under the new arrays (:50; a junction that is gone is never reached by the iterator); counters[3]: calls whose answer
// to that changed, counters[4]: made calls without a standing evaluation
__global__ void __launch_bounds__(256) k_s3b_made(const S3Call* __restrict__ calls, uint64_t n_calls, const S3Res* __restrict__ res, uint8_t* __restrict__ made,
                                                  const uint32_t* __restrict__ dead, const uint32_t* __restrict__ claim, unsigned long long* __restrict__ counters) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls) return;
    const S3Call call = calls[c];
    if (call.idx < 0) return;
    const bool now = dead[call.slot] >= (uint32_t)c && (call.phase != FGPU_BUILD_BRANCHING || claim[5 * (uint64_t)call.row + call.idx] >= (uint32_t)c);
    if (now != (made[c] != 0)) { made[c] = now; atomicAdd(counters + 3, 1ULL); }
    if (now && !res[c].valid) atomicAdd(counters + 4, 1ULL);
}

// behind the fixed point: the first made call on which the reference does not return
__global__ void __launch_bounds__(256) k_s3b_stop(const S3Call* __restrict__ calls, uint64_t n_calls, const S3Res* __restrict__ res, const uint8_t* __restrict__ made,
                                                  uint32_t* __restrict__ stop) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls || calls[c].idx < 0 || !made[c]) return;
    if (res[c].status) atomicMin(stop, (uint32_t)c);
}
// the calls that are output, and their sizes
__global__ void __launch_bounds__(256) k_s3b_sizes(const S3Call* __restrict__ calls, uint64_t n_calls, const S3Res* __restrict__ res, const uint8_t* __restrict__ made,
                                                   const uint32_t* __restrict__ stop, uint64_t* __restrict__ is_out) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls) return;
    is_out[c] = calls[c].idx >= 0 && made[c] && (uint32_t)c < *stop ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_s3b_counts(uint64_t n_calls, const S3Res* __restrict__ res, const uint64_t* __restrict__ out_at, uint64_t* __restrict__ words,
                                                    uint64_t* __restrict__ segs, uint64_t* __restrict__ covs) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_calls || out_at[c + 1] == out_at[c]) return;
    const S3Res e = res[c];
    const uint64_t o = out_at[c];
    words[o] = ((uint64_t)e.len + 31) / 32; segs[o] = e.n_seg; covs[o] = e.n_cov;
}
// a round that ran out of room for its table hits is taken back: its evaluations do not stand
__global__ void __launch_bounds__(256) k_s3b_undo(uint64_t n_calls, S3Res* __restrict__ res, uint32_t gen) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_calls && res[c].valid && res[c].gen == gen) res[c].valid = 0;
}

}  // namespace

namespace {
void s3b_drop(fgpu_ctx* ctx) {                             // results nobody took
    if (ctx->s3b_out) { (void)hipFree(ctx->s3b_out); ctx->s3b_out = nullptr; }
    for (int i = 0; i < 4; i++) ctx->s3b_totals[i] = 0;
    ctx->s3b_have = false;
    ctx->s3b_serial++;                                     // (whatever comes next is another build: a graph made of this one is stale)
}
struct S3bLayout { uint64_t contigs, calls, text, kmers, dist, cov, bytes; };
S3bLayout s3b_layout(const uint64_t tot[4]) {
    S3bLayout l;
    uint64_t at = 0;
    l.contigs = s3c_take(at, tot[0] * sizeof(fgpu_contig)); l.calls = s3c_take(at, tot[0] * sizeof(fgpu_build_call)); l.text = s3c_take(at, tot[1] * 8);
    l.kmers = s3c_take(at, tot[2] * 8); l.dist = s3c_take(at, tot[2]); l.cov = s3c_take(at, tot[3]);
    l.bytes = at;
    return l;
}
}  // namespace

int fgpu_s3b_view(fgpu_ctx* ctx, const fgpu_contig** contigs, const fgpu_build_call** calls, const uint64_t** text) {
    if (!ctx->s3b_have) return 0;
    const S3bLayout lay = s3b_layout(ctx->s3b_totals);
    const char* res = (const char*)ctx->s3b_out;          // (null only where every total is 0)
    if (contigs) *contigs = (const fgpu_contig*)(res + lay.contigs);
    if (calls) *calls = (const fgpu_build_call*)(res + lay.calls);
    if (text) *text = (const uint64_t*)(res + lay.text);
    return 1;
}

int fgpu_s3b_lists(fgpu_ctx* ctx, const uint8_t** seg_dist, const uint8_t** cov) {
    if (!ctx->s3b_have) return 0;
    const S3bLayout lay = s3b_layout(ctx->s3b_totals);
    const char* res = (const char*)ctx->s3b_out;
    if (seg_dist) *seg_dist = (const uint8_t*)(res + lay.dist);
    if (cov) *cov = (const uint8_t*)(res + lay.cov);
    return 1;
}

extern "C" int fgpu_stage3_build_totals(fgpu_ctx* ctx, uint64_t totals[4]) {
    if (!ctx || !totals) return FGPU_ERR_ARG;
    for (int i = 0; i < 4; i++) totals[i] = 0;
    if (!ctx->s3b_have) { ctx->err = "fgpu_stage3_build_totals: no fgpu_stage3_build whose results are still on the device"; return FGPU_ERR_STATE; }
    for (int i = 0; i < 4; i++) totals[i] = ctx->s3b_totals[i];
    return FGPU_OK;
}

extern "C" int fgpu_stage3_build(fgpu_ctx* ctx, int32_t max_read_length, uint64_t totals[4], fgpu_build_info* info) {
    if (!ctx || !totals || max_read_length < 1) return FGPU_ERR_ARG;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_build while a pass is open"; return FGPU_ERR_STATE; }
    if (!ctx->s3_ready) { ctx->err = "fgpu_stage3_build before fgpu_stage3_set_junctions"; return FGPU_ERR_STATE; }
    const uint64_t nj = ctx->s3_count;
    if (nj >= (1ULL << 29)) { ctx->err = "fgpu_stage3_build: five calls per junction and two states per table slot have to fit 32 bits"; return FGPU_ERR_ARG; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    if (ctx->s3c_out) {
        FGPU_HIP(hipFree(ctx->s3c_out));
        ctx->s3c_out = nullptr;
        ctx->s3c_totals[0] = ctx->s3c_totals[1] = ctx->s3c_totals[2] = 0;
    }
    s3b_drop(ctx);
    for (int i = 0; i < 4; i++) totals[i] = 0;
    fgpu_build_info inf;
    memset(&inf, 0, sizeof(inf));
    if (info) *info = inf;
    if (!nj) {
        ctx->s3b_have = true;
        ctx->s3b_status = 0;
        return FGPU_OK;
    }
    const int k = ctx->prm.k;
    const uint64_t stride = fgpu_stage3_contig_words(k, max_read_length);
    const uint64_t* d_keys = (const uint64_t*)((const char*)ctx->s3_in.p + 64);
    const fgpu_junction* d_recs = (const fgpu_junction*)(d_keys + nj);
    const uint64_t *tkeys = (const uint64_t*)ctx->s3_keys.p, *tdist = (const uint64_t*)ctx->s3_dist.p, *tcov = (const uint64_t*)ctx->s3_cov.p;
    const uint64_t slots = ctx->s3_mask + 1;
    int rc;
    // ---- the time slots: count per junction, scan, list
    size_t scan_bytes = 0;
    FGPU_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, 5 * nj + 3, rocprim::plus<uint64_t>(), ctx->stream));
    S3Scratch plan;
    uint64_t pat = 0;
    const uint64_t p_cnt = s3c_take(pat, 2 * (nj + 1) * 8), p_off = s3c_take(pat, 2 * (nj + 1) * 8), p_scan = s3c_take(pat, scan_bytes), p_slot = s3c_take(pat, nj * 4),
                   p_dead = s3c_take(pat, slots * 4), p_claim = s3c_take(pat, 5 * nj * 4), p_ctr = s3c_take(pat, 64);
    if ((rc = s3c_alloc(ctx, &plan.p, pat, "the build's arrays"))) return rc;
    char* pb = (char*)plan.p;
    uint64_t *d_nb = (uint64_t*)(pb + p_cnt), *d_nl = d_nb + (nj + 1), *d_b0 = (uint64_t*)(pb + p_off), *d_l0 = d_b0 + (nj + 1);
    uint32_t *d_row_slot = (uint32_t*)(pb + p_slot), *d_dead = (uint32_t*)(pb + p_dead), *d_claim = (uint32_t*)(pb + p_claim);
    unsigned long long* d_ctr = (unsigned long long*)(pb + p_ctr);     // table hits kept | probes | evaluations of the round | made flips | left to evaluate | stop
    FGPU_HIP(hipMemsetAsync(d_nb, 0, 2 * (nj + 1) * 8, ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_dead, 0xFF, slots * 4, ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_ctr, 0, 64, ctx->stream));
    FGPU_LAUNCH("s3b_count", k_s3b_count, fgpu_blocks(nj, 256), 256, d_keys, d_recs, nj, k, ctx->fd.kmask, d_nb, d_nl);
    FGPU_HIP(rocprim::exclusive_scan(pb + p_scan, scan_bytes, d_nb, d_b0, (uint64_t)0, nj + 1, rocprim::plus<uint64_t>(), ctx->stream));
    FGPU_HIP(rocprim::exclusive_scan(pb + p_scan, scan_bytes, d_nl, d_l0, (uint64_t)0, nj + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t n_branch = 0, n_linear = 0;
    FGPU_HIP(hipMemcpyAsync(&n_branch, d_b0 + nj, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&n_linear, d_l0 + nj, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    const uint64_t n_calls = n_branch + 1 + n_linear;      // (<= 5 * nj + 1 < 2^32)
    S3Scratch work;
    uint64_t wat = 0;
    const uint64_t w_calls = s3c_take(wat, n_calls * sizeof(S3Call)), w_res = s3c_take(wat, n_calls * sizeof(S3Res)), w_made = s3c_take(wat, n_calls),
                   w_isout = s3c_take(wat, (n_calls + 1) * 8), w_outat = s3c_take(wat, (n_calls + 1) * 8), w_cnt = s3c_take(wat, 3 * (n_calls + 1) * 8),
                   w_off = s3c_take(wat, 3 * (n_calls + 1) * 8), w_text = s3c_take(wat, n_calls * stride * 8);
    if ((rc = s3c_alloc(ctx, &work.p, wat, "the calls"))) return rc;
    char* wb = (char*)work.p;
    S3Call* d_calls = (S3Call*)(wb + w_calls);
    S3Res* d_res = (S3Res*)(wb + w_res);
    uint8_t* d_made = (uint8_t*)(wb + w_made);
    uint64_t *d_isout = (uint64_t*)(wb + w_isout), *d_outat = (uint64_t*)(wb + w_outat);
    uint64_t *d_words = (uint64_t*)(wb + w_cnt), *d_segs = d_words + (n_calls + 1), *d_covs = d_segs + (n_calls + 1);
    uint64_t *d_word0 = (uint64_t*)(wb + w_off), *d_seg0 = d_word0 + (n_calls + 1), *d_cov0 = d_seg0 + (n_calls + 1);
    uint64_t* d_text = (uint64_t*)(wb + w_text);
    FGPU_HIP(hipMemsetAsync(d_calls, 0xFF, n_calls * sizeof(S3Call), ctx->stream));       // idx -1: no call
    FGPU_HIP(hipMemsetAsync(d_res, 0, n_calls * sizeof(S3Res), ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_made, 0, n_calls, ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_isout, 0, (n_calls + 1) * 8, ctx->stream));
    FGPU_HIP(hipMemsetAsync(d_words, 0, 3 * (n_calls + 1) * 8, ctx->stream));
    FGPU_LAUNCH("s3b_list", k_s3b_list, fgpu_blocks(nj + 1, 256), 256, d_keys, d_recs, nj, k, ctx->fd.kmask, (const uint64_t*)d_b0, (const uint64_t*)d_l0, tkeys, ctx->s3_mask,
                d_calls, d_row_slot);
    FGPU_LAUNCH("s3b_seed", k_s3b_seed, fgpu_blocks(nj, 256), 256, d_recs, (const uint32_t*)d_row_slot, nj, n_branch, d_dead, d_claim);
    FGPU_LAUNCH("s3b_made", k_s3b_made, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, (const S3Res*)d_res, d_made, (const uint32_t*)d_dead,
                (const uint32_t*)d_claim, d_ctr);
    // ---- the fixed point
    S3Scratch hits;
    uint64_t dep_cap = 8 * n_calls + 1024, dep_top = 0;    // (a call of config 2's scanned map records six, profiles/stage3_build.txt)
    if ((rc = s3c_alloc(ctx, &hits.p, dep_cap * sizeof(S3Dep), "the table hits"))) return rc;
    bool settled = false;
    for (uint64_t round = 0; round <= n_calls + 1 && !settled; round++) {
        unsigned long long ctr[5] = {0, 0, 0, 0, 0};
        for (;;) {                                         // (again only after the table hits ran out of room: twice the room each time, until memory does)
            FGPU_HIP(hipMemsetAsync(d_ctr + 2, 0, 24, ctx->stream));
            FGPU_LAUNCH("s3b_chain", k_s3b_chain<false>, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, d_keys, nj, (const uint8_t*)d_made, d_res,
                        (uint32_t)round, ctx->fd, (const uint32_t*)ctx->bloo2, tkeys, tdist, tcov, ctx->s3_mask, (const uint32_t*)d_dead, (int)max_read_length, d_text,
                        stride, (S3Dep*)hits.p, d_ctr, dep_cap, (const uint64_t*)nullptr, (const uint64_t*)nullptr, (const uint64_t*)nullptr, (const uint64_t*)nullptr,
                        (fgpu_contig*)nullptr, (fgpu_build_call*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint8_t*)nullptr, (uint8_t*)nullptr);
            FGPU_HIP(hipMemcpyAsync(ctr, d_ctr, 24, hipMemcpyDeviceToHost, ctx->stream));
            FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
            if (ctr[0] <= dep_cap) break;
            FGPU_LAUNCH("s3b_undo", k_s3b_undo, fgpu_blocks(n_calls, 256), 256, n_calls, d_res, (uint32_t)round);
            S3Scratch more;
            const uint64_t cap2 = 2 * (uint64_t)ctr[0];
            if ((rc = s3c_alloc(ctx, &more.p, cap2 * sizeof(S3Dep), "the table hits"))) return rc;
            if (dep_top) FGPU_HIP(hipMemcpyAsync(more.p, hits.p, dep_top * sizeof(S3Dep), hipMemcpyDeviceToDevice, ctx->stream));
            const unsigned long long back[2] = {dep_top, inf.probes};
            FGPU_HIP(hipMemcpyAsync(d_ctr, back, 16, hipMemcpyHostToDevice, ctx->stream));
            FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
            void* old = hits.p; hits.p = more.p; more.p = old;
            dep_cap = cap2;
            inf.regrown++;
        }
        dep_top = ctr[0];
        inf.table_hits = dep_top;
        inf.rounds = (uint32_t)(round + 1);
        inf.rewalked += ctr[2];
        if (round < FGPU_BUILD_ROUNDS_KEPT) inf.rewalked_by_round[round] = ctr[2];
        inf.probes = ctr[1];
        FGPU_LAUNCH("s3b_seed", k_s3b_seed, fgpu_blocks(nj, 256), 256, d_recs, (const uint32_t*)d_row_slot, nj, n_branch, d_dead, d_claim);
        if (dep_top) FGPU_LAUNCH("s3b_kills", k_s3b_kills, fgpu_blocks(dep_top, 256), 256, (const S3Dep*)hits.p, dep_top, (const S3Res*)d_res, (const uint8_t*)d_made, d_dead);
        FGPU_LAUNCH("s3b_claims", k_s3b_claims, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, d_res, (const uint8_t*)d_made, tcov, (const uint32_t*)d_dead,
                    d_claim);
        if (dep_top) FGPU_LAUNCH("s3b_check", k_s3b_check, fgpu_blocks(dep_top, 256), 256, (const S3Dep*)hits.p, dep_top, d_res, (const uint32_t*)d_dead);
        FGPU_HIP(hipMemsetAsync(d_ctr + 3, 0, 16, ctx->stream));
        FGPU_LAUNCH("s3b_made", k_s3b_made, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, (const S3Res*)d_res, d_made, (const uint32_t*)d_dead,
                    (const uint32_t*)d_claim, d_ctr);
        FGPU_HIP(hipMemcpyAsync(ctr + 3, d_ctr + 3, 16, hipMemcpyDeviceToHost, ctx->stream));
        FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        settled = ctr[3] == 0 && ctr[4] == 0;
    }
    if (!settled) { ctx->err = "fgpu_stage3_build: the fixed point did not settle within calls + 1 rounds"; return FGPU_ERR_INTERNAL; }
    // ---- which calls are output; count, scan, place
    uint32_t* d_stop = (uint32_t*)(d_ctr + 5);
    FGPU_HIP(hipMemsetAsync(d_stop, 0xFF, 4, ctx->stream));
    FGPU_LAUNCH("s3b_stop", k_s3b_stop, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, (const S3Res*)d_res, (const uint8_t*)d_made, d_stop);
    FGPU_LAUNCH("s3b_sizes", k_s3b_sizes, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, (const S3Res*)d_res, (const uint8_t*)d_made, (const uint32_t*)d_stop,
                d_isout);
    FGPU_HIP(rocprim::exclusive_scan(pb + p_scan, scan_bytes, d_isout, d_outat, (uint64_t)0, n_calls + 1, rocprim::plus<uint64_t>(), ctx->stream));
    FGPU_LAUNCH("s3b_counts", k_s3b_counts, fgpu_blocks(n_calls, 256), 256, n_calls, (const S3Res*)d_res, (const uint64_t*)d_outat, d_words, d_segs, d_covs);
    for (int i = 0; i < 3; i++)
        FGPU_HIP(rocprim::exclusive_scan(pb + p_scan, scan_bytes, d_words + i * (n_calls + 1), d_word0 + i * (n_calls + 1), (uint64_t)0, n_calls + 1, rocprim::plus<uint64_t>(),
                                         ctx->stream));
    uint64_t tot[4] = {0, 0, 0, 0};
    uint32_t stop = S3B_NEVER;
    FGPU_HIP(hipMemcpyAsync(&tot[0], d_outat + n_calls, 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(&stop, d_stop, 4, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    // (the sums are over the calls that are output: entry tot[0] of each)
    for (int i = 0; i < 3; i++) FGPU_HIP(hipMemcpyAsync(&tot[1 + i], d_word0 + i * (n_calls + 1) + tot[0], 8, hipMemcpyDeviceToHost, ctx->stream));
    S3Res stopped;
    memset(&stopped, 0, sizeof(stopped));
    if (stop != S3B_NEVER) FGPU_HIP(hipMemcpyAsync(&stopped, d_res + stop, sizeof(S3Res), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    const S3bLayout lay = s3b_layout(tot);
    void* out = nullptr;
    if ((rc = s3c_alloc(ctx, &out, lay.bytes, "the results"))) return rc;
    ctx->s3b_out = out;                                    // (freed with the context from here on)
    char* ob = (char*)out;
    if (tot[0])
        FGPU_LAUNCH("s3b_chain", k_s3b_chain<true>, fgpu_blocks(n_calls, 256), 256, (const S3Call*)d_calls, n_calls, d_keys, nj, (const uint8_t*)d_made, d_res, 0u, ctx->fd,
                    (const uint32_t*)ctx->bloo2, tkeys, tdist, tcov, ctx->s3_mask, (const uint32_t*)d_dead, (int)max_read_length, d_text, stride, (S3Dep*)nullptr, d_ctr,
                    (uint64_t)0, (const uint64_t*)d_outat, (const uint64_t*)d_word0, (const uint64_t*)d_seg0, (const uint64_t*)d_cov0, (fgpu_contig*)(ob + lay.contigs),
                    (fgpu_build_call*)(ob + lay.calls), (uint64_t*)(ob + lay.text), (uint64_t*)(ob + lay.kmers), (uint8_t*)(ob + lay.dist), (uint8_t*)(ob + lay.cov));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    inf.status = stop == S3B_NEVER ? 0 : stopped.status;
    inf.stop_call = tot[0];
    inf.calls_possible = n_calls;
    for (int i = 0; i < 4; i++) totals[i] = ctx->s3b_totals[i] = tot[i];
    ctx->s3b_have = true;
    ctx->s3b_status = inf.status;
    if (info) *info = inf;
    return FGPU_OK;
}

extern "C" int fgpu_stage3_build_take(fgpu_ctx* ctx, fgpu_contig* contigs, fgpu_build_call* calls, uint64_t n_calls, uint64_t* text, uint64_t text_words,
                                      uint64_t* seg_kmers, uint8_t* seg_dist, uint64_t n_seg, uint8_t* cov, uint64_t n_cov) {
    if (!ctx) return FGPU_ERR_ARG;
    const uint64_t* tot = ctx->s3b_totals;
    if (n_calls < tot[0] || text_words < tot[1] || n_seg < tot[2] || n_cov < tot[3] || (tot[0] && (!contigs || !calls)) || (tot[1] && !text) ||
        (tot[2] && (!seg_kmers || !seg_dist)) || (tot[3] && !cov)) {
        ctx->err = "fgpu_stage3_build_take: an array is smaller than the totals fgpu_stage3_build gave";
        return FGPU_ERR_ARG;
    }
    if (!ctx->s3b_out) { ctx->s3b_have = false; return FGPU_OK; }
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const S3bLayout lay = s3b_layout(tot);
    const char* res = (const char*)ctx->s3b_out;
    if (tot[0]) FGPU_HIP(hipMemcpyAsync(contigs, res + lay.contigs, tot[0] * sizeof(fgpu_contig), hipMemcpyDeviceToHost, ctx->stream));
    if (tot[0]) FGPU_HIP(hipMemcpyAsync(calls, res + lay.calls, tot[0] * sizeof(fgpu_build_call), hipMemcpyDeviceToHost, ctx->stream));
    if (tot[1]) FGPU_HIP(hipMemcpyAsync(text, res + lay.text, tot[1] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tot[2]) FGPU_HIP(hipMemcpyAsync(seg_kmers, res + lay.kmers, tot[2] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tot[2]) FGPU_HIP(hipMemcpyAsync(seg_dist, res + lay.dist, tot[2], hipMemcpyDeviceToHost, ctx->stream));
    if (tot[3]) FGPU_HIP(hipMemcpyAsync(cov, res + lay.cov, tot[3], hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    s3b_drop(ctx);
    return FGPU_OK;
}
