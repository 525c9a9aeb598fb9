// stage3_join.hip — contigs that are joins of many contigs of a build: ContigJuncList::concatenate over piece lists, on the device
// (fgpu_stage3_join, fgpu_stage3_join_take; include/faucet_gpu.h).
//
// What the reference does per join, Contig::concatenate (src/Contig.cpp:83-109):
//   ContigJuncList::reverse                         utils/ContigJuncList.cpp:98-103    both lists reversed, the sequence reverse-complemented
//   ContigJuncList::concatenate                     utils/ContigJuncList.cpp:107-123   seq.substr(0, len - k) + other; distances appended; the
//                                                                                      last coverage and the other's first become their minimum
//   ContigJuncList::getAvgCoverage                  utils/ContigJuncList.cpp:166-176   sum / size, in double
// WHERE every piece's bases, distances and coverages land is arithmetic over the lists' sizes, which the host has in hand when it checks the
// lists (it must, so that no kernel reads behind an array): three running sums per piece.  MOVING them is the device's.  Three kernels,
// integer and bitwise only, every output element written by exactly one lane:
//   k_join_text   one lane per WORD of the joined strings: 32 bases cut out of as many pieces as it takes (a middle piece gives len - k
//                 bases, which may be none) at any base offset, by the funnel shifts and the 32-base reverse complement of stage3_bits.h
//   k_join_dist   one lane per distance: its piece by a search over the pieces' running sum, a flipped piece read backwards
//   k_join_cov    eight lanes per list, a lane per eighth coverage entry: the minimum over the pieces whose oriented list reaches the entry
//                 -- one inside a piece, two at a join, more where middle pieces hold a single entry -- and the list's sum by a reduction
//                 over the eight (shuffles; no atomics)
// And what a cleaning step reads of a contig's coverages before anything is joined (fgpu_stage3_cov_calls; cov_summary.h):
//   k_cov_calls   four lanes per contig record: sum, size, first and last entry of its list, one 16-byte record each
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "cov_summary.h"
#include "fgpu_ctx.h"
#include "stage3_bits.h"

namespace {

// Lanes that share a list in k_join_cov.  The contigs of a build hold two coverage entries on average and a cleaned graph's tens to hundreds:
// a wave per list (as k_emit_canon has it) spent 0.32 ms on the 9.1e5 lists of config 2's build, nearly all of it on waves with two busy
// lanes (profiles/stage3_join.txt).
constexpr uint32_t JOIN_COV_LANES = 8;

static_assert(sizeof(fgpu_join_piece) == 8 && sizeof(fgpu_joined) == 48, "the records as api.py lays them out");

// Per piece p, three running sums over ALL pieces in CSR order (entry n_pieces: the totals), each list's share following the last one's:
//   base[p]  joined bases in front of the piece's own (its own: len - k, all of len for a list's last piece)
//   dist[p]  joined distances in front of its own (n_seg)
//   cov[p]   the joined coverage entry its FIRST coverage goes into: a piece other than a list's last shares its last entry with the
//            next piece's first, so it moves the sum on by n_cov - 1, a list's last piece by n_cov
struct JoinIn {
    const uint64_t* list_first;                  // n + 1
    const fgpu_join_piece* pieces;
    const uint64_t *base, *dist, *cov;           // n_pieces + 1 each
    const uint64_t* word0;                       // n + 1: first word of each joined string
    const fgpu_contig* contigs;
    const uint64_t* text;
    const uint8_t *seg_dist, *covs;
};

__global__ void __launch_bounds__(256) k_join_text(JoinIn in, uint64_t n, int k, uint64_t n_words, uint64_t* __restrict__ joined) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_words) return;
    const uint64_t i = emit_find(in.word0, n, g);
    const uint64_t p0 = in.list_first[i], p1 = in.list_first[i + 1];
    const uint64_t first = in.base[p0] + (g - in.word0[i]) * 32, end = in.base[p1];      // the word's bases: first .. min(first + 32, end)
    uint64_t p = emit_find_in(in.base, p0, p1, first);                     // (the last piece that starts at or before `first`: it has bases of its own)
    uint64_t w = 0;
    uint32_t fill = 0;
    while (fill < 32 && first + fill < end) {                              // (first + fill < end: p < p1)
        const fgpu_join_piece pc = in.pieces[p];
        const fgpu_contig c = in.contigs[pc.call];
        const uint64_t own = in.base[p + 1] - in.base[p], off = first + fill - in.base[p];
        if (off < own) {
            const uint32_t take = (uint32_t)(own - off < 32 - fill ? own - off : 32 - fill);
            w |= (emit_oriented(in.text + c.text_word, c.len, pc.flip != 0, (uint32_t)off) & emit_low_fields(take)) << (2 * fill);
            fill += take;
        }
        p++;
    }
    joined[g] = w;                                                          // (the bits behind the string's last base were never set)
}

__global__ void __launch_bounds__(256) k_join_dist(JoinIn in, uint64_t n_pieces, uint64_t n_out, uint8_t* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_out) return;
    const uint64_t p = emit_find(in.dist, n_pieces, e);                    // (pieces without distances share a sum with the one behind them: the last of them has some)
    const fgpu_join_piece pc = in.pieces[p];
    const fgpu_contig c = in.contigs[pc.call];
    const uint64_t o = e - in.dist[p];
    out[e] = in.seg_dist[c.seg_first + (pc.flip ? c.n_seg - 1 - o : o)];
}

__global__ void __launch_bounds__(256) k_join_cov(JoinIn in, uint64_t n, uint8_t* __restrict__ out, uint64_t* __restrict__ sums) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / JOIN_COV_LANES;    // JOIN_COV_LANES lanes per list (uniform within the group)
    if (i >= n) return;
    const uint32_t lane = threadIdx.x % JOIN_COV_LANES;
    const uint64_t p0 = in.list_first[i], p1 = in.list_first[i + 1];
    uint64_t sum = 0;
    for (uint64_t j = in.cov[p0] + lane; j < in.cov[p1]; j += JOIN_COV_LANES) {
        // The last piece whose first coverage lands at or before j holds entry j; so does every piece in front of it whose list reaches
        // as far -- its last entry was merged into j -- and their ends only fall on the way down: stop at the first that does not.
        uint32_t v = 255;
        for (uint64_t p = emit_find_in(in.cov, p0, p1, j);; p--) {
            const fgpu_join_piece pc = in.pieces[p];
            const fgpu_contig c = in.contigs[pc.call];
            const uint64_t o = j - in.cov[p];
            if (o >= c.n_cov) break;
            const uint32_t x = in.covs[c.cov_first + (pc.flip ? c.n_cov - 1 - o : o)];
            v = x < v ? x : v;
            if (p == p0) break;
        }
        out[j] = (uint8_t)v;
        sum += v;
    }
    for (int d = JOIN_COV_LANES / 2; d; d >>= 1) sum += __shfl_down(sum, d, JOIN_COV_LANES);
    if (lane == 0) sums[i] = sum;
}

// Lanes that share a call in k_cov_calls: the same distribution as above before anything is joined -- two entries on average, a few lists of
// thousands -- so four lanes leave half of them busy on the common list and a long one costs a quarter of its entries per lane.
constexpr uint32_t COV_CALL_LANES = 4;

static_assert(sizeof(fgpu_cov_summary) == 16 && alignof(fgpu_cov_summary) == 8, "one record, one aligned 16-byte store");

// One summary per contig record, read from the coverage array where it lies: a lane per fourth entry for the sum (shuffles; no atomics), the
// group's first lane reads the two end entries and writes the record.  The host has checked that every record lies inside the array.
__global__ void __launch_bounds__(256) k_cov_calls(const fgpu_contig* __restrict__ contigs, uint64_t n, const uint8_t* __restrict__ covs,
                                                   fgpu_cov_summary* __restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / COV_CALL_LANES;    // (uniform within the group)
    if (i >= n) return;
    const uint32_t lane = threadIdx.x % COV_CALL_LANES;
    const uint64_t first = contigs[i].cov_first;
    const uint32_t n_cov = contigs[i].n_cov;
    uint64_t sum = 0;
    for (uint64_t j = lane; j < n_cov; j += COV_CALL_LANES) sum += covs[first + j];
    for (int d = COV_CALL_LANES / 2; d; d >>= 1) sum += __shfl_down(sum, d, COV_CALL_LANES);
    if (lane) return;
    fgpu_cov_summary s;
    s.sum = sum;
    s.n = n_cov;
    s.first = n_cov ? covs[first] : 0;
    s.last = n_cov ? covs[first + n_cov - 1] : 0;
    s.reserved[0] = s.reserved[1] = 0;
    out[i] = s;
}

struct JoinScratch {                             // device memory of one call, gone when it returns
    void* p = nullptr;
    ~JoinScratch() { if (p) (void)hipFree(p); }
};
inline uint64_t join_take(uint64_t& at, uint64_t bytes) {
    const uint64_t here = at;
    at += (bytes + 15) & ~15ULL;
    return here;
}
struct JoinLayout { uint64_t text, dist, cov, bytes; };
JoinLayout join_layout(const uint64_t tot[3]) {
    JoinLayout l;
    uint64_t at = 0;
    l.text = join_take(at, tot[0] * 8); l.dist = join_take(at, tot[1]); l.cov = join_take(at, tot[2]);
    l.bytes = at;
    return l;
}
void join_drop(fgpu_ctx* ctx) {                  // results nobody took
    if (ctx->s3j_out) { (void)hipFree(ctx->s3j_out); ctx->s3j_out = nullptr; }
    for (int i = 0; i < 3; i++) ctx->s3j_totals[i] = 0;
}
int join_bad(fgpu_ctx* ctx, const std::string& what) {
    ctx->err = "fgpu_stage3_join: " + what;
    return FGPU_ERR_ARG;
}

}  // namespace

int fgpu_s3j_text(fgpu_ctx* ctx, const uint64_t** text) {
    if (!ctx->s3j_out) return 0;
    *text = (const uint64_t*)((const char*)ctx->s3j_out + join_layout(ctx->s3j_totals).text);
    return 1;
}

extern "C" int fgpu_stage3_join(fgpu_ctx* ctx, const uint64_t* list_first, uint64_t n, const fgpu_join_piece* pieces, uint64_t n_pieces,
                                const fgpu_contig* contigs_host, uint64_t n_contigs, const uint64_t* text_host, uint64_t text_words,
                                const uint8_t* dist_host, uint64_t n_dist, const uint8_t* cov_host, uint64_t n_cov, fgpu_joined* out, uint64_t totals[3]) {
    if (!ctx || !totals || !list_first || (n && !out) || (n_pieces && !pieces)) return FGPU_ERR_ARG;
    totals[0] = totals[1] = totals[2] = 0;
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_join while a pass is open"; return FGPU_ERR_STATE; }
    const bool from_build = contigs_host == nullptr;
    if (from_build ? (n_contigs || text_host || text_words || dist_host || n_dist || cov_host || n_cov)
                   : ((text_words && !text_host) || (n_dist && !dist_host) || (n_cov && !cov_host)))
        return join_bad(ctx, from_build ? "without contigs the pieces index the build on the device: the other arrays must be NULL / 0" : "an array of some entries is NULL");
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const int k = ctx->prm.k;
    const fgpu_contig* d_contigs = nullptr;
    const uint64_t* d_text = nullptr;
    const uint8_t *d_dist = nullptr, *d_cov = nullptr;
    std::vector<fgpu_contig> of_build;
    if (from_build) {
        if (!fgpu_s3b_view(ctx, &d_contigs, nullptr, &d_text) || !fgpu_s3b_lists(ctx, &d_dist, &d_cov)) {
            ctx->err = "fgpu_stage3_join without contigs: no fgpu_stage3_build whose results are still on the device";
            return FGPU_ERR_STATE;
        }
        n_contigs = ctx->s3b_totals[0]; text_words = ctx->s3b_totals[1]; n_dist = ctx->s3b_totals[2]; n_cov = ctx->s3b_totals[3];
        of_build.resize(n_contigs);
        if (n_contigs) {
            FGPU_HIP(hipMemcpyAsync(of_build.data(), d_contigs, n_contigs * sizeof(fgpu_contig), hipMemcpyDeviceToHost, ctx->stream));
            FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
        }
        contigs_host = of_build.data();
    }
    // every entry the kernels will read lies in its array; where everything lands
    if (list_first[0] != 0 || list_first[n] != n_pieces) return join_bad(ctx, "list_first does not run from 0 to n_pieces");
    std::vector<uint64_t> sums(3 * (n_pieces + 1) + (n + 1));
    uint64_t *s_base = sums.data(), *s_dist = s_base + (n_pieces + 1), *s_cov = s_dist + (n_pieces + 1), *word0 = s_cov + (n_pieces + 1);
    uint64_t at_base = 0, at_dist = 0, at_cov = 0, at_word = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t p0 = list_first[i], p1 = list_first[i + 1];
        if (p0 >= p1 || p1 > n_pieces) return join_bad(ctx, "list " + std::to_string(i) + " is empty, or list_first does not ascend");
        const uint64_t base0 = at_base, dist0 = at_dist, cov0 = at_cov;
        for (uint64_t p = p0; p < p1; p++) {
            const fgpu_join_piece& pc = pieces[p];
            const bool last = p + 1 == p1;
            if (pc.call >= n_contigs || pc.flip > 1) return join_bad(ctx, "piece " + std::to_string(p) + " names a contig that is not there, or a flip other than 0 or 1");
            const fgpu_contig& c = contigs_host[pc.call];
            if (c.len < 1 || c.len >= (1u << 30) || c.text_word > text_words || ((uint64_t)c.len + 31) / 32 > text_words - c.text_word || c.seg_first > n_dist ||
                c.n_seg > n_dist - c.seg_first || c.n_cov < 1 || c.cov_first > n_cov || c.n_cov > n_cov - c.cov_first)
                return join_bad(ctx, "piece " + std::to_string(p) + " (contig " + std::to_string(pc.call) + ") reaches past the text, the distances or the coverages, has no bases or 2^30 and more, or no coverage entry");
            if (!last && c.len < (uint32_t)k) return join_bad(ctx, "piece " + std::to_string(p) + " is joined to the next one and is shorter than k");
            s_base[p] = at_base; s_dist[p] = at_dist; s_cov[p] = at_cov;
            at_base += last ? c.len : c.len - (uint32_t)k;
            at_dist += c.n_seg;
            at_cov += last ? c.n_cov : c.n_cov - 1;
        }
        if (at_base - base0 > 0xFFFFFFFFull || at_dist - dist0 > 0xFFFFFFFFull || at_cov - cov0 > 0xFFFFFFFFull)
            return join_bad(ctx, "list " + std::to_string(i) + " joins to 2^32 and more bases, distances or coverages");
        fgpu_joined& o = out[i];
        o.text_word = word0[i] = at_word; o.dist_first = dist0; o.cov_first = cov0; o.cov_sum = 0;
        o.len = (uint32_t)(at_base - base0); o.n_dist = (uint32_t)(at_dist - dist0); o.n_cov = (uint32_t)(at_cov - cov0); o.reserved = 0;
        at_word += ((uint64_t)o.len + 31) / 32;
    }
    s_base[n_pieces] = at_base; s_dist[n_pieces] = at_dist; s_cov[n_pieces] = at_cov; word0[n] = at_word;
    join_drop(ctx);
    if (!n) return FGPU_OK;
    const uint64_t tot[3] = {at_word, at_dist, at_cov};
    JoinScratch work;
    uint64_t at = 0;
    const uint64_t o_sums = join_take(at, sums.size() * 8), o_first = join_take(at, (n + 1) * 8), o_pieces = join_take(at, n_pieces * sizeof(fgpu_join_piece)),
                   o_res = join_take(at, n * 8), o_contigs = join_take(at, from_build ? 0 : n_contigs * sizeof(fgpu_contig)),
                   o_text = join_take(at, from_build ? 0 : text_words * 8), o_dist = join_take(at, from_build ? 0 : n_dist), o_cov = join_take(at, from_build ? 0 : n_cov);
    hipError_t e = hipMalloc(&work.p, at);
    const JoinLayout lay = join_layout(tot);
    void* res = nullptr;
    if (e == hipSuccess) e = hipMalloc(&res, lay.bytes ? lay.bytes : 16);
    if (e != hipSuccess) {
        ctx->err = std::string("fgpu_stage3_join: hipMalloc of ") + std::to_string(at) + " and " + std::to_string(lay.bytes) + " bytes failed: " + hipGetErrorString(e);
        return FGPU_ERR_NOMEM;
    }
    ctx->s3j_out = res;                          // (freed with the context from here on)
    char* wb = (char*)work.p;
    FGPU_HIP(hipMemcpyAsync(wb + o_sums, sums.data(), sums.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(wb + o_first, list_first, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    FGPU_HIP(hipMemcpyAsync(wb + o_pieces, pieces, n_pieces * sizeof(fgpu_join_piece), hipMemcpyHostToDevice, ctx->stream));
    if (!from_build) {
        if (n_contigs) FGPU_HIP(hipMemcpyAsync(wb + o_contigs, contigs_host, n_contigs * sizeof(fgpu_contig), hipMemcpyHostToDevice, ctx->stream));
        if (text_words) FGPU_HIP(hipMemcpyAsync(wb + o_text, text_host, text_words * 8, hipMemcpyHostToDevice, ctx->stream));
        if (n_dist) FGPU_HIP(hipMemcpyAsync(wb + o_dist, dist_host, n_dist, hipMemcpyHostToDevice, ctx->stream));
        if (n_cov) FGPU_HIP(hipMemcpyAsync(wb + o_cov, cov_host, n_cov, hipMemcpyHostToDevice, ctx->stream));
        d_contigs = (const fgpu_contig*)(wb + o_contigs); d_text = (const uint64_t*)(wb + o_text);
        d_dist = (const uint8_t*)(wb + o_dist); d_cov = (const uint8_t*)(wb + o_cov);
    }
    JoinIn in;
    in.list_first = (const uint64_t*)(wb + o_first);
    in.pieces = (const fgpu_join_piece*)(wb + o_pieces);
    in.base = (const uint64_t*)(wb + o_sums); in.dist = in.base + (n_pieces + 1); in.cov = in.dist + (n_pieces + 1); in.word0 = in.cov + (n_pieces + 1);
    in.contigs = d_contigs; in.text = d_text; in.seg_dist = d_dist; in.covs = d_cov;
    uint64_t* d_sums = (uint64_t*)(wb + o_res);
    if (tot[0]) FGPU_LAUNCH("s3j_text", k_join_text, fgpu_blocks(tot[0], 256), 256, in, n, k, tot[0], (uint64_t*)((char*)res + lay.text));
    if (tot[1]) FGPU_LAUNCH("s3j_dist", k_join_dist, fgpu_blocks(tot[1], 256), 256, in, n_pieces, tot[1], (uint8_t*)res + lay.dist);
    FGPU_LAUNCH("s3j_cov", k_join_cov, fgpu_blocks(n, 256 / JOIN_COV_LANES), 256, in, n, (uint8_t*)res + lay.cov, d_sums);
    std::vector<uint64_t> cov_sums(n);
    FGPU_HIP(hipMemcpyAsync(cov_sums.data(), d_sums, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    for (uint64_t i = 0; i < n; i++) out[i].cov_sum = cov_sums[i];
    for (int i = 0; i < 3; i++) totals[i] = ctx->s3j_totals[i] = tot[i];
    return FGPU_OK;
}

extern "C" int fgpu_stage3_cov_calls(fgpu_ctx* ctx, const fgpu_contig* contigs_host, uint64_t n_contigs, const uint8_t* cov_host, uint64_t n_cov,
                                     fgpu_cov_summary* out_host) {
    if (!ctx) return FGPU_ERR_ARG;
    auto bad = [&](const std::string& what) { ctx->err = "fgpu_stage3_cov_calls: " + what; return FGPU_ERR_ARG; };
    if (ctx->phase != 0) { ctx->err = "fgpu_stage3_cov_calls while a pass is open"; return FGPU_ERR_STATE; }
    const bool from_build = contigs_host == nullptr;
    if (from_build ? (n_contigs || cov_host || n_cov) : (n_cov && !cov_host))
        return bad(from_build ? "without contigs the calls are those of the build on the device: the other arrays must be NULL / 0" : "a coverage array of some entries is NULL");
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const fgpu_contig* d_contigs = nullptr;
    const uint8_t* d_cov = nullptr;
    if (from_build) {                            // (the build wrote these records and the array they index itself: nothing to check, nothing comes to the host)
        if (!fgpu_s3b_view(ctx, &d_contigs, nullptr, nullptr) || !fgpu_s3b_lists(ctx, nullptr, &d_cov)) {
            ctx->err = "fgpu_stage3_cov_calls without contigs: no fgpu_stage3_build whose results are still on the device";
            return FGPU_ERR_STATE;
        }
        n_contigs = ctx->s3b_totals[0]; n_cov = ctx->s3b_totals[3];
    }
    if (n_contigs && !out_host) return bad("no room for the summaries");
    for (uint64_t i = 0; !from_build && i < n_contigs; i++)     // every entry the kernel will read lies in the array
        if (contigs_host[i].cov_first > n_cov || contigs_host[i].n_cov > n_cov - contigs_host[i].cov_first)
            return bad("record " + std::to_string(i) + " reaches past the coverages");
    if (!n_contigs) return FGPU_OK;
    JoinScratch work;
    uint64_t at = 0;
    const uint64_t o_out = join_take(at, n_contigs * sizeof(fgpu_cov_summary)), o_contigs = join_take(at, from_build ? 0 : n_contigs * sizeof(fgpu_contig)),
                   o_cov = join_take(at, from_build ? 0 : n_cov);
    if (hipError_t e = hipMalloc(&work.p, at)) {
        ctx->err = std::string("fgpu_stage3_cov_calls: hipMalloc of ") + std::to_string(at) + " bytes failed: " + hipGetErrorString(e);
        return FGPU_ERR_NOMEM;
    }
    char* wb = (char*)work.p;
    if (!from_build) {
        FGPU_HIP(hipMemcpyAsync(wb + o_contigs, contigs_host, n_contigs * sizeof(fgpu_contig), hipMemcpyHostToDevice, ctx->stream));
        if (n_cov) FGPU_HIP(hipMemcpyAsync(wb + o_cov, cov_host, n_cov, hipMemcpyHostToDevice, ctx->stream));
        d_contigs = (const fgpu_contig*)(wb + o_contigs); d_cov = (const uint8_t*)(wb + o_cov);
    }
    FGPU_LAUNCH("s3j_cov_calls", k_cov_calls, fgpu_blocks(n_contigs, 256 / COV_CALL_LANES), 256, d_contigs, n_contigs, d_cov, (fgpu_cov_summary*)(wb + o_out));
    FGPU_HIP(hipMemcpyAsync(out_host, wb + o_out, n_contigs * sizeof(fgpu_cov_summary), hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    return FGPU_OK;
}

extern "C" int fgpu_stage3_join_take(fgpu_ctx* ctx, uint64_t* text, uint64_t text_words, uint8_t* dist, uint64_t n_dist, uint8_t* cov, uint64_t n_cov) {
    if (!ctx) return FGPU_ERR_ARG;
    const uint64_t* tot = ctx->s3j_totals;
    if (text_words < tot[0] || n_dist < tot[1] || n_cov < tot[2] || (tot[0] && !text) || (tot[1] && !dist) || (tot[2] && !cov)) {
        ctx->err = "fgpu_stage3_join_take: an array is smaller than the totals fgpu_stage3_join gave";
        return FGPU_ERR_ARG;
    }
    if (!ctx->s3j_out) return FGPU_OK;
    FGPU_HIP(hipSetDevice(ctx->prm.device));
    const JoinLayout lay = join_layout(tot);
    const char* res = (const char*)ctx->s3j_out;
    if (tot[0]) FGPU_HIP(hipMemcpyAsync(text, res + lay.text, tot[0] * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (tot[1]) FGPU_HIP(hipMemcpyAsync(dist, res + lay.dist, tot[1], hipMemcpyDeviceToHost, ctx->stream));
    if (tot[2]) FGPU_HIP(hipMemcpyAsync(cov, res + lay.cov, tot[2], hipMemcpyDeviceToHost, ctx->stream));
    FGPU_HIP(fgpu_sync_stream(ctx, ctx->stream));
    join_drop(ctx);
    return FGPU_OK;
}
