// faucet_main.cpp — the `faucet` command line on top of libfaucet_gpu.so (C ABI, include/faucet_gpu.h).
//
// Host side of the hot path in the reference's own language (C++11).  Same flags, same required arguments, same
// exit codes and the same output files as src/Faucet.cpp:57-182,248-300 for the part of the run this repository
// covers: the Bloom load pass (-> <prefix>.bloom) and the junction scan (-> <prefix>.junctions, and without
// --no_cleaning <prefix>.short_pair_filter / .long_pair_filter).  The contig-graph stage is not part of this build:
// the program stops after the last file the scan produces (exit code 3 when the reference would have gone on to the
// contig graph; the reference itself can be restarted from these files with -bloom_file / -junctions_file).
// No k-mer window, filter probe or junction is computed on the host: everything goes through fgpu_*; if the library
// finds no gfx950 device the program fails (there is no CPU path).  What stays on the host is what SURVEY.md 8(b)
// leaves there: the JunctionMap container that fixes the dump order, and the files.  Both pair filters are filled on the
// device from scanInputRead's per-read lists (fgpu_scan_short_pairs, fgpu_scan_long_pairs) and come back as bytes.
// Not in the reference: --estimate.  -estimated_kmers and -singletons, which the reference has its users find with a separate k-mer counter,
// may then be left out; a pass 0 over -read_load_file sketches the reads on the device (fgpu_estimate_*) and fills in whichever is absent;
// with -gpus N every rank sketches its read shard and the sketches are merged (ShardedRun::estimate).  Where -read_load_file can be read only
// once (a pipe) pass 0 keeps the batches it packs on the device and pass 1 loads from them (fgpu_estimate_keep, fgpu_load_batch_packed).
// Not in the reference either: --scan_kept.  Pass 1 keeps, beside the packed batches it keeps anyway, their read offsets (FGPU_LOAD_KEEP_READS),
// and pass 2 scans those batches (fgpu_scan_batch_kept) instead of reading, splitting and packing the input a second time: -read_scan_file may
// be left out, and one reading of the input -- with --estimate on a pipe: of a stream -- serves the whole run.  One device only.
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <math.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <atomic>
#include <fstream>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "faucet_gpu.h"
#include "junction_order.h"
#include "scan_pass.h"
#include "shard_host.h"
#include "text_source.h"

// The estimate pass' entry points are referred to WEAKLY, as shard_host.h refers to the sliced pass': linked against an implementation of the ABI
// without them they are null, and --estimate is refused before anything is read.
#pragma weak fgpu_estimate_begin
#pragma weak fgpu_estimate_batch
#pragma weak fgpu_estimate_end
// ... and so are the four that let pass 0 keep its packed reads for pass 1: without them --estimate needs a -read_load_file it can read twice
#pragma weak fgpu_estimate_keep
#pragma weak fgpu_estimate_keep_state
#pragma weak fgpu_estimate_take_kept
#pragma weak fgpu_load_batch_packed
// ... and the three through which pass 0's blocks carry their reads, for --scan_kept behind --estimate on a pipe (scan_pass.h refers to the two of
// the kept scan itself)
#pragma weak fgpu_estimate_keep_reads
#pragma weak fgpu_estimate_take_kept_reads
#pragma weak fgpu_load_batch_packed_reads
// ... and the four of --raw_contigs (Stage 3's graph build and the FASTA of its contigs): without them the flag is refused before anything is read
#pragma weak fgpu_stage3_set_junctions
#pragma weak fgpu_stage3_build
#pragma weak fgpu_stage3_raw_contigs
#pragma weak fgpu_stage3_fasta_take
// ... and the one more of --detipped_contigs (ContigGraph::deleteTipsAndClean on that build)
#pragma weak fgpu_stage3_detip
// ... and of --dechimered_contigs (ContigGraph::removeChimerasAndClean on the graph that step left)
#pragma weak fgpu_stage3_dechimera
// ... and the two of --raw_graph, --detipped_graph and --dechimered_graph (ContigGraph::printGraph on the build's graph and on the live one)
#pragma weak fgpu_stage3_raw_graph
#pragma weak fgpu_stage3_graph_fastg

using faucet_host::ReadSource;
using faucet_host::TextSource;
using faucet_host::pinned_slot;
using faucet_host::kTextPad;

namespace {

struct Options {   // globals of src/Faucet.h:14-53
    float fp_rate = .04f;
    int j = 1;
    std::string read_load_file, read_scan_file, bloom_input_file, junctions_prefix, file_prefix;
    int read_length = 0, k = 0;
    uint64_t estimated_kmers = 0, singletons = 0;
    bool load_file_flag = false, scan_file_flag = false, k_val_flag = false, max_len_flag = false, est_kmers_flag = false,
         est_sing_flag = false, pref_flag = false;
    bool two_hash = false, from_bloom = false, from_junctions = false, just_load = false, fastq = false, mercy = false,
         node_graph = false, paired_ends = false, no_cleaning = false, high_cov = false;
    int max_spacer_dist = 100;
    uint64_t batch_reads = 0;         // not a reference flag: > 0 = split records on the host, this many reads per device call
    uint64_t chunk_mb = 64;           // not a reference flag: file text handed to the device per call, records split there
    uint64_t chunk_bytes = 0;         // = chunk_mb << 20, less for regular files that are smaller (choose_chunk_bytes)
    uint64_t tai = 0;                 // bloo1 / bloo2: bits and hash functions, from the flags above (size_filters)
    int32_t n_hash = 0;
    int gpus = 1;                     // not a reference flag: read shards over this many GPUs, one host thread each (shard_host.h)
    std::string transport = "copy";   // not a reference flag: how the shards' bitmaps and tables travel: copy (device-to-device copies) | rccl
    bool estimate = false;            // not a reference flag: --estimate, -estimated_kmers / -singletons may be left out and are then estimated (pass 0)
    int estimate_bits = 0;            // not a reference flag: -estimate_bits r, 2^r cells per level of the sketch (0: the library's default, 30)
    bool scan_kept = false;           // not a reference flag: --scan_kept, pass 2 scans the batches pass 1 kept; -read_scan_file may be left out
    bool raw_contigs = false;         // not a reference flag: --raw_contigs, <prefix>.raw_contigs.fasta (the file src/Faucet.cpp:314 would write) behind the scan outputs
    bool detipped_contigs = false;    // not a reference flag: --detipped_contigs, <prefix>.detipped_contigs.fasta (what printContigs would write after the first deleteTipsAndClean of cleanGraph)
    bool raw_graph = false;           // not a reference flag: --raw_graph, <prefix>.raw_graph.fastg (the file src/Faucet.cpp:313 would write: ContigGraph::printGraph behind the build)
    bool detipped_graph = false;      // not a reference flag: --detipped_graph, <prefix>.detipped_graph.fastg (printGraph after the first deleteTipsAndClean)
    bool dechimered_graph = false;    // not a reference flag: --dechimered_graph, <prefix>.dechimered_graph.fastg (... after the removeChimerasAndClean behind it)
    bool dechimered_contigs = false;  // not a reference flag: --dechimered_contigs, <prefix>.dechimered_contigs.fasta (... after the removeChimerasAndClean behind it)
};

void argument_error() {   // src/Faucet.cpp:50-54
    fprintf(stderr, "Usage:\n");
    fprintf(stderr, "./faucet -read_load_file <filename> -read_scan_file <filename> -size_kmer <k> -max_read_length <length> "
                    "-estimated_kmers <num_kmers> -singletons <num_kmers> -file_prefix <prefix>");
    fprintf(stderr, "\nOptional arguments: --fastq --mercy --high_cov -max_spacer_dist <dist> -fp rate <rate> -j <int> --two_hash "
                    "-bloom_file <filename> -junctions_file <filename> --paired_ends --no_cleaning\n");
    fprintf(stderr, "Of this build: -gpus <n> -transport copy|rccl -batch_reads <n> -chunk_mb <n> --estimate -estimate_bits <r> "
                    "--scan_kept (pass 2 scans the reads pass 1 kept on the device: -read_scan_file may be left out) "
                    "--raw_contigs (writes <prefix>.raw_contigs.fasta, the contigs of the graph build before any cleaning)\n"
                    "--detipped_contigs (writes <prefix>.detipped_contigs.fasta, the contigs after the first cleaning step, ContigGraph::deleteTipsAndClean)\n"
                    "--dechimered_contigs (writes <prefix>.dechimered_contigs.fasta, the contigs after the second cleaning step, ContigGraph::removeChimerasAndClean)\n"
                    "--raw_graph (writes <prefix>.raw_graph.fastg, the graph build before any cleaning as ContigGraph::printGraph prints it: two strands per contig, headers that name the neighbours)\n"
                    "--detipped_graph (writes <prefix>.detipped_graph.fastg, the graph after the first cleaning step)\n"
                    "--dechimered_graph (writes <prefix>.dechimered_graph.fastg, the graph after the second cleaning step)\n");
}

// src/Faucet.cpp:57-182 (with the missing `return 0` supplied and a bounds check on flag values)
int handle_arguments(int argc, char** argv, Options& o) {
    if (argc == 1) { argument_error(); return 1; }
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char*& out) { if (i + 1 >= argc) return false; out = argv[++i]; return true; };
        const char* v = nullptr;
        if (a == "-read_load_file") { if (!val(v)) goto bad; o.read_load_file = v; o.load_file_flag = true; }
        else if (a == "-read_scan_file") { if (!val(v)) goto bad; o.read_scan_file = v; o.scan_file_flag = true; }
        else if (a == "-size_kmer") { if (!val(v)) goto bad; o.k = atoi(v); o.k_val_flag = true; }
        else if (a == "-max_read_length") { if (!val(v)) goto bad; o.read_length = atoi(v); o.max_len_flag = true; }
        else if (a == "-estimated_kmers") { if (!val(v)) goto bad; o.estimated_kmers = (uint64_t)atoll(v); o.est_kmers_flag = true; }
        else if (a == "-singletons") { if (!val(v)) goto bad; o.singletons = (uint64_t)atoll(v); o.est_sing_flag = true; }
        else if (a == "-fp") { if (!val(v)) goto bad; o.fp_rate = (float)atof(v); }
        else if (a == "-j") { if (!val(v)) goto bad; o.j = atoi(v); }
        else if (a == "-file_prefix") { if (!val(v)) goto bad; o.file_prefix = v; o.pref_flag = true; }
        else if (a == "--two_hash") o.two_hash = true;
        else if (a == "--just_load_bloom") o.just_load = true;
        else if (a == "--no_cleaning") o.no_cleaning = true;
        else if (a == "--fastq") o.fastq = true;
        else if (a == "--mercy") o.mercy = true;
        else if (a == "--high_cov") o.high_cov = true;
        else if (a == "--node_graph") o.node_graph = true;
        else if (a == "--paired_ends") o.paired_ends = true;
        else if (a == "-bloom_file") { if (!val(v)) goto bad; o.bloom_input_file = v; o.from_bloom = true; }
        else if (a == "-max_spacer_dist") { if (!val(v)) goto bad; o.max_spacer_dist = atoi(v); }
        else if (a == "-junctions_file") { if (!val(v)) goto bad; o.junctions_prefix = v; o.from_junctions = true; }
        else if (a == "-batch_reads") { if (!val(v)) goto bad; o.batch_reads = (uint64_t)atoll(v); }
        else if (a == "-chunk_mb") { if (!val(v)) goto bad; o.chunk_mb = (uint64_t)atoll(v); if (!o.chunk_mb) o.chunk_mb = 1; }
        else if (a == "-gpus") { if (!val(v)) goto bad; o.gpus = atoi(v); if (o.gpus < 1 || o.gpus > 64) { fprintf(stderr, "-gpus must be in 1..64\n"); return 1; } }
        else if (a == "-transport") { if (!val(v)) goto bad; o.transport = v; if (o.transport != "copy" && o.transport != "rccl") { fprintf(stderr, "-transport must be copy or rccl\n"); return 1; } }
        else if (a == "--estimate") o.estimate = true;
        else if (a == "--scan_kept") o.scan_kept = true;
        else if (a == "--raw_contigs") o.raw_contigs = true;
        else if (a == "--detipped_contigs") o.detipped_contigs = true;
        else if (a == "--dechimered_contigs") o.dechimered_contigs = true;
        else if (a == "--raw_graph") o.raw_graph = true;
        else if (a == "--detipped_graph") o.detipped_graph = true;
        else if (a == "--dechimered_graph") o.dechimered_graph = true;
        else if (a == "-estimate_bits") { if (!val(v)) goto bad; o.estimate_bits = atoi(v); if (o.estimate_bits < FGPU_EST_MIN_BITS || o.estimate_bits > FGPU_EST_MAX_BITS) { fprintf(stderr, "-estimate_bits must be in %d..%d\n", FGPU_EST_MIN_BITS, FGPU_EST_MAX_BITS); return 1; } }
        else if (a == "--help" || a == "-h") { argument_error(); return 1; }
        else { fprintf(stderr, "Cannot parse tag %s\n", argv[i]); argument_error(); return 1; }
        continue;
    bad:
        fprintf(stderr, "Missing value after %s\n", a.c_str());
        argument_error();
        return 1;
    }
    // (--estimate: the two counts may be left out, pass 0 fills them in; --scan_kept: the scan file may be, pass 2 reads no file)
    if (!(o.load_file_flag && (o.scan_file_flag || o.scan_kept) && o.k_val_flag && o.max_len_flag && (o.est_kmers_flag || o.estimate) && (o.est_sing_flag || o.estimate) && o.pref_flag)) {
        fprintf(stderr, "Some required argument is missing.\n");
        argument_error();
        return 1;
    }
    if (o.from_junctions && !o.from_bloom) {
        fprintf(stderr, "Cannot start from junctions without a bloom file.\n");
        argument_error();
        return 1;
    }
    return 0;
}

// ... and the lines it prints once the arguments stand (src/Faucet.cpp:136-181): apart, so that --estimate can fill in the two counts in between
void print_settings(const Options& o) {
    if (o.from_junctions) printf("Starting from after read scan based on bloom and junction files.\n");
    else if (o.from_bloom) printf("Starting from after bloom load based on bloom file.\n");
    else printf("Starting at the beginning: will load bloom and find junctions from the read set.\n");
    if (o.just_load) printf("Only loading bloom, dumping and termination.\n");
    printf(o.node_graph ? "Using node graph.\n" : "Using contig graph.\n");          // src/Faucet.cpp:146-149 (a switch of the stage this build stops before)
    printf("Read load file name: %s\n", o.read_load_file.c_str());
    printf("Read scan file name: %s\n", (o.scan_file_flag ? o.read_scan_file : o.read_load_file).c_str());      // (--scan_kept without one: the reads of the load file)
    printf("k: %d \n", o.k);
    printf("Maximal read length: %d\n", o.read_length);
    printf("Estimated number of distinct kmers, for sizing bloom filter: %llu.\n", (unsigned long long)o.estimated_kmers);
    printf("False positive rate: %f\n", o.fp_rate);
    printf("File prefix: %s\n", o.file_prefix.c_str());
    printf("Max spacer dist: %d\n", o.max_spacer_dist);
    printf(o.two_hash ? "Using 2 hash functions.\n" : "Using space-optimal hash settings.\n");
    printf("Paired ends: %d\n", (int)o.paired_ends);
    // src/Faucet.cpp:177-181 prints sizeof(Junction / ContigNode / Contig / int / long) of ITS build: the reference's values on x86-64 Linux,
    // so that what a caller greps or diffs in the log stays where it is
    printf("Size of junction: 14\nSize of contigNode: 48\nSize of contig: 104\nSize of int: 4\nSize of long: 8\n");
}

// one interface over both ways of cutting the input into batches: file text split on the device (TextSource), or -batch_reads records
// split here (ReadSource) -- text_source.h
class BatchSource {
public:
    BatchSource(const Options& o, const std::string& path)
        : host_(o.batch_reads ? new ReadSource(path, o.fastq) : nullptr),
          text_(o.batch_reads ? nullptr : new TextSource(path, o.fastq, o.chunk_bytes)), batch_reads_(o.batch_reads) {}
    ~BatchSource() { delete host_; delete text_; }
    BatchSource(const BatchSource&) = delete;
    BatchSource& operator=(const BatchSource&) = delete;
    bool is_open() const { return host_ ? host_->is_open() : text_->is_open(); }
    // 1 = a batch, 0 = input exhausted, < 0 = -status of a failed fgpu_text_split
    int next(fgpu_ctx* ctx, fgpu_reads* out) { return text_ ? text_->next(ctx, out) : host_->next(batch_reads_, out) ? 1 : 0; }
private:
    ReadSource* host_;
    TextSource* text_;
    uint64_t batch_reads_;
};

#define CHECK(call)                                                                   \
    do {                                                                              \
        int rc__ = (call);                                                            \
        if (rc__ != FGPU_OK) {                                                        \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, fgpu_last_error(ctx)); \
            return 2;                                                                 \
        }                                                                             \
    } while (0)

struct Junction {   // utils/Junction.h:10-18
    uint8_t cov[4], dist[5], linked[5];
};

const char kDecode[4] = {'A', 'C', 'T', 'G'};   // utils/Kmer.cpp:21

// ---- the pair filters: sized and written by the host, filled on the device ---------------------------------------
struct PairFilter {   // a Bloom used through addPair / containsPair only (utils/Bloom.cpp:127-154): here just its bytes, which the device fills
    uint64_t tai = 0;
    int n_hash = 0;
    std::vector<uint8_t> bits;
    void create(uint64_t elements, float fp) {   // create_bloom_filter_optimal, utils/Bloom.cpp:229-247
        int32_t bpk = 0, nh = 0;
        fgpu_size_optimal(elements, fp, &bpk, &tai, &nh);
        n_hash = nh;
        printf("Bits per kmer: %d \n", bpk);
        printf("BF memory: %f MB\n", (float)((elements * (uint64_t)bpk) / 8ULL / 1024ULL) / 1024);
        printf("Number of hash functions: %d \n", n_hash);
        bits.assign(tai / 8, 0);
    }
    float weight() const {   // Bloom::weight, utils/Bloom.cpp:191-203
        long w = 0;
        size_t i = 0;
        for (; i + 8 <= bits.size(); i += 8) {       // a word at a time (the filter of a --no_cleaning run is 8 MiB of zeros: 10 ms byte by byte)
            uint64_t x;
            memcpy(&x, &bits[i], 8);
            w += __builtin_popcountll(x);
        }
        for (; i < bits.size(); i++) w += __builtin_popcount(bits[i]);
        return (float)w / (float)tai;
    }
    int dump(const std::string& path) const {   // Bloom::dump, utils/Bloom.cpp:571-578
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
        const bool ok = fwrite(bits.data(), 1, bits.size(), f) == bits.size();
        if (fclose(f) != 0 || !ok) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
        return 0;
    }
};

// The junction container of the reference, for the paths that need a real one: -junctions_file (a later line with the same k-mer replaces the
// earlier one) and the dump order on a standard library whose container DumpOrder does not replay (junction_order.h).
typedef std::unordered_map<uint64_t, Junction> JunctionTable;

// JunctionMap::writeToFile (utils/JunctionMap.cpp:579-596), Junction::toString (utils/Junction.cpp:74-89):
//   "<kmer> d0 d1 d2 d3 d4  c0 c1 c2 c3 <sum>  l0 l1 l2 l3 l4 \n"
// in the order given (indices into keys / recs), formatted by hand: a million lines, a few threads, each its own stretch of the order.
int write_junctions(const std::string& path, const uint64_t* keys, const fgpu_junction* recs, const std::vector<uint32_t>& order, int k) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
    if (fd < 0) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
    const size_t kLine = (size_t)k + 1 + 5 * 4 + 1 + 4 * 4 + 5 + 1 + 5 * 2 + 1;   // longest line: three digits and a blank per byte field
    auto format = [&](size_t from, size_t to, std::vector<char>& buf) -> size_t {      // returns the bytes written into buf (sized once per thread, never re-zeroed)
        if (buf.size() < (to - from) * kLine) buf.resize((to - from) * kLine);
        char* w = buf.data();
        auto put_uint = [&](unsigned v) {
            if (v >= 1000) *w++ = (char)('0' + v / 1000);
            if (v >= 100) *w++ = (char)('0' + v / 100 % 10);
            if (v >= 10) *w++ = (char)('0' + v / 10 % 10);
            *w++ = (char)('0' + v % 10);
            *w++ = ' ';
        };
        for (size_t at = from; at < to; at++) {
            if (at + 8 < to) { __builtin_prefetch(&keys[order[at + 8]]); __builtin_prefetch(&recs[order[at + 8]]); }
            uint64_t x = keys[order[at]];
            for (int i = k - 1; i >= 0; i--) { w[i] = kDecode[x & 3]; x >>= 2; }
            w += k;
            *w++ = ' ';
            const fgpu_junction& j = recs[order[at]];
            for (int i = 0; i < 5; i++) put_uint(j.dist[i]);
            *w++ = ' ';
            for (int i = 0; i < 4; i++) put_uint(j.cov[i]);
            const unsigned sum = (unsigned)j.cov[0] + j.cov[1] + j.cov[2] + j.cov[3];
            put_uint(sum);   // at most 4 * 255
            *w++ = ' ';
            for (int i = 0; i < 5; i++) { *w++ = j.linked[i] ? '1' : '0'; *w++ = ' '; }
            *w++ = '\n';
        }
        return (size_t)(w - buf.data());
    };
    // Round 6 (profiles/r06_cli_large.txt: 1.25 s for config 5's 2.95e7 lines, formatting and writing in turn): the order is cut into chunks that
    // the threads take one after the other; a chunk's place in the file is known as soon as every chunk before it has been FORMATTED (its size), and
    // it is then written there (pwrite) while other chunks are still being formatted or written -- formatting and writing overlap, both in parallel.
    const size_t kChunk = getenv("FAUCET_DEBUG_DUMP_CHUNK") ? (size_t)std::max(1, atoi(getenv("FAUCET_DEBUG_DUMP_CHUNK"))) : (size_t)1 << 18;   // (tests: many small chunks)
    const size_t n_chunks = (order.size() + kChunk - 1) / kChunk;
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(8, std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 4), n_chunks));
    std::vector<uint64_t> offset(n_chunks + 1, 0);
    std::mutex m;
    std::condition_variable cv;
    size_t known = 0, next = 0;          // offset[0 .. known] are final; next chunk to hand out
    std::atomic<bool> failed(false);     // (set under the mutex, read outside it as well)
    auto worker = [&]() {
        std::vector<char> buf;
        for (;;) {
            size_t i;
            { std::lock_guard<std::mutex> g(m); if (next >= n_chunks || failed) return; i = next++; }
            const size_t bytes = format(i * kChunk, std::min(order.size(), (i + 1) * kChunk), buf);
            uint64_t at;
            {
                std::unique_lock<std::mutex> g(m);
                cv.wait(g, [&] { return known == i || failed; });      // (chunks are handed out in order: chunk i - 1 is being formatted or done)
                if (failed) return;
                at = offset[i];
                offset[i + 1] = at + bytes;
                known = i + 1;
            }
            cv.notify_all();
            size_t done = 0;
            while (done < bytes) {
                const ssize_t w = pwrite(fd, buf.data() + done, bytes - done, (off_t)(at + done));
                if (w <= 0) { std::lock_guard<std::mutex> g(m); failed = true; break; }
                done += (size_t)w;
            }
            if (failed) { cv.notify_all(); return; }
        }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < n_threads; t++) th.emplace_back(worker);
    worker();
    for (std::thread& t : th) t.join();
    const bool bad = failed || close(fd) != 0;
    if (bad) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
    return 0;
}

// JunctionMap::buildFromFile (utils/JunctionMap.cpp:619-639) with Junction's parsing constructor (utils/Junction.cpp:102-118): the k-mer as
// text (getFirstKmerFromRead: A0 C1 T2 G3), five distances, four coverages, their sum (skipped), five link flags; a later line with the same
// k-mer replaces the earlier one (junctionMap[kmer] = junc).  Returns -1 when the file cannot be opened or a line does not parse.
long read_junctions(const std::string& path, int k, JunctionTable& map) {
    std::ifstream in(path.c_str());
    if (!in.is_open()) return -1;
    std::string line;
    long n_lines = 0;
    while (std::getline(in, line)) {
        if ((int)line.size() < k + 1) return -1;
        uint64_t kmer = 0;
        for (int i = 0; i < k; i++) {
            const char c = line[(size_t)i];
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return -1;
            kmer = (kmer << 2) | (uint64_t)((c >> 1) & 3);
        }
        int v[15];
        const char* p = line.c_str() + k;
        for (int i = 0; i < 15; i++) {
            char* end = nullptr;
            const long x = strtol(p, &end, 10);
            if (end == p) return -1;
            v[i] = (int)x;
            p = end;
        }
        Junction j;
        for (int i = 0; i < 5; i++) j.dist[i] = (uint8_t)v[i];
        for (int i = 0; i < 4; i++) j.cov[i] = (uint8_t)v[5 + i];
        for (int i = 0; i < 5; i++) j.linked[i] = (uint8_t)(v[10 + i] != 0);
        map[kmer] = j;
        n_lines++;
    }
    return n_lines;
}

int load_pair_filter(PairFilter& pf, const std::string& path) {   // Bloom::load (utils/Bloom.cpp:580-587): what fits is taken, like -bloom_file
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 2; }
    printf("loading bloom filter from file, nelem %llu \n", (unsigned long long)pf.bits.size());
    const size_t got = fread(pf.bits.data(), 1, pf.bits.size(), f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != pf.bits.size() || more)
        fprintf(stderr, "note: %s is not of the %llu bytes this run's filter has: its head is taken, what it does not cover stays empty (as in the reference)\n",
                path.c_str(), (unsigned long long)pf.bits.size());
    printf("bloom loaded\n");
    return 0;
}

}  // namespace

// FGPU_CLI_TIMES=1: phase clock on stderr (measurement aid; stdout stays what the reference prints)
struct PhaseClock {
    bool on = getenv("FGPU_CLI_TIMES") != nullptr;
    double batch_ms = 0, take_ms = 0, pairs_ms = 0, scan_ms = 0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[cli] %-28s %9.2f ms  (at %9.2f ms)\n", what, std::chrono::duration<double, std::milli>(now - last).count(),
                std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// --raw_contigs: ContigGraph::printContigs on the graph JunctionMap::buildContigGraph returns (src/Faucet.cpp:305-314, the printContigs line
// commented out there), on the device that holds the map and bloo2.  The reference builds the graph on the map the scan left, iterated in
// its container's order -- the order `.junctions` is written in; set_junctions gets the records in that order.  0, or the exit code.
int write_raw_contigs(const Options& o, fgpu_ctx* ctx, const uint64_t* keys, const fgpu_junction* recs, const std::vector<uint32_t>& order, PhaseClock& clk) {
    std::vector<uint64_t> map_keys(order.size() ? order.size() : 1);
    std::vector<fgpu_junction> map_recs(order.size() ? order.size() : 1);
    for (size_t i = 0; i < order.size(); i++) { map_keys[i] = keys[order[i]]; map_recs[i] = recs[order[i]]; }
    CHECK(fgpu_stage3_set_junctions(ctx, map_keys.data(), map_recs.data(), order.size()));
    uint64_t totals[4] = {0, 0, 0, 0};
    fgpu_build_info bi;
    CHECK(fgpu_stage3_build(ctx, o.read_length, totals, &bi));
    clk.mark("  raw contigs: graph build");
    if (bi.status != 0) {      // the reference itself does not return from buildContigGraph on this map: no file
        const char* what = o.raw_graph ? "raw_graph" : o.raw_contigs ? "raw_contigs" : o.detipped_graph ? "detipped_graph" : o.detipped_contigs ? "detipped_contigs"
                           : o.dechimered_graph ? "dechimered_graph" : "dechimered_contigs";
        const char* kind = strstr(what, "graph") ? "fastg" : "fasta";
        fprintf(stderr, "--%s: getContig call %llu of JunctionMap::buildContigGraph %s: the reference does not get as far as printing on this map, no %s.%s.%s is written\n",
                what, (unsigned long long)bi.stop_call, bi.status == 1 ? "trips an assert of the reference" : "never returns in the reference", o.file_prefix.c_str(), what, kind);
        return 2;
    }
    // a file leaves the device right behind the call that made it: the next Stage-3 call drops what was not taken
    auto take_file = [&](std::vector<char>& text, uint64_t bytes) -> int {
        text.assign(bytes ? bytes : 1, 0);
        CHECK(fgpu_stage3_fasta_take(ctx, text.data(), bytes));
        return 0;
    };
    auto put_file = [&](const std::string& path, const std::vector<char>& text, uint64_t bytes) -> int {
        FILE* f = fopen(path.c_str(), "wb");
        if (!f || fwrite(text.data(), 1, bytes, f) != bytes || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 2; }
        return 0;
    };
    auto write_file = [&](const std::string& path, uint64_t bytes) -> int {
        std::vector<char> text;
        if (int rc = take_file(text, bytes)) return rc;
        return put_file(path, text, bytes);
    };
    // ContigGraph::printGraph (src/ContigGraph.cpp:1470-1503) and its four lines, ahead of printContigs as src/Faucet.cpp:313-314 and :325-326 have them
    auto write_graph = [&](const char* what, int call_rc, uint64_t bytes, const fgpu_fastg_info& gi) -> int {
        if (call_rc != FGPU_OK) {
            fprintf(stderr, "--%s: %s: no %s.%s.fastg is written\n", what, fgpu_last_error(ctx), o.file_prefix.c_str(), what);
            return 2;
        }
        printf("Printing unitig FASTG.\n");
        if (int rc = write_file(o.file_prefix + "." + what + ".fastg", bytes)) return rc;
        printf("printed %d node-connected unitigs\n", (int)gi.node_records);
        printf("printed %d isolated contigs\n", (int)gi.isolated_listed);       // (the whole list, as the reference counts)
        printf("Done printing graph.\n");
        return 0;
    };
    if (o.raw_graph) {
        uint64_t bytes = 0;
        fgpu_fastg_info gi;
        const int call_rc = fgpu_stage3_raw_graph(ctx, o.read_length, &bytes, &gi);
        if (int rc = write_graph("raw_graph", call_rc, bytes, gi)) return rc;
        clk.mark("  raw graph: summaries, plan, join, emission, file");
    }
    if (o.raw_contigs) {
        uint64_t bytes = 0;
        fgpu_raw_info ri;
        CHECK(fgpu_stage3_raw_contigs(ctx, o.read_length, &bytes, &ri));
        if (int rc = write_file(o.file_prefix + ".raw_contigs.fasta", bytes)) return rc;
        printf("Raw contigs: %llu records (%llu bubble, %llu off nodes, %llu isolated; %llu isolated below the read length left out) from %llu nodes, %llu bytes\n",
               (unsigned long long)ri.records, (unsigned long long)ri.bubble_records, (unsigned long long)ri.node_contigs, (unsigned long long)ri.isolated_kept,
               (unsigned long long)ri.isolated_dropped, (unsigned long long)ri.nodes, (unsigned long long)bytes);
        clk.mark("  raw contigs: plan, emission, file");
    }
    if (o.detipped_contigs || o.dechimered_contigs || o.detipped_graph || o.dechimered_graph) {  // the first step of ContigGraph::cleanGraph (src/ContigGraph.cpp:211-215) on the same build, which is still on the device
        uint64_t bytes = 0;
        fgpu_tips_info ti;
        if (fgpu_stage3_detip(ctx, o.read_length, &bytes, &ti) != FGPU_OK) {      // (a plan status other than OK among them: no file)
            const char* what = o.detipped_graph ? "detipped_graph" : o.detipped_contigs ? "detipped_contigs" : o.dechimered_graph ? "dechimered_graph" : "dechimered_contigs";
            fprintf(stderr, "--%s: %s: no %s.%s.%s is written\n", what, fgpu_last_error(ctx), o.file_prefix.c_str(), what, strstr(what, "graph") ? "fastg" : "fasta");
            return 2;
        }
        std::vector<char> contigs_text;          // (the step runs for the next one whether or not its own file is asked for)
        if (o.detipped_contigs) {
            if (int rc = take_file(contigs_text, bytes)) return rc;
        }
        if (o.detipped_graph) {                  // the live graph the step left, printed before its contigs are; the graph stays as it is
            uint64_t graph_bytes = 0;
            fgpu_fastg_info gi;
            const int call_rc = fgpu_stage3_graph_fastg(ctx, &graph_bytes, &gi);
            if (int rc = write_graph("detipped_graph", call_rc, graph_bytes, gi)) return rc;
            clk.mark("  detipped graph: summaries, plan, join, emission, file");
        }
        if (o.detipped_contigs) {
            if (int rc = put_file(o.file_prefix + ".detipped_contigs.fasta", contigs_text, bytes)) return rc;
            printf("Detipped contigs: %llu tips deleted (and %llu back tips), %llu of %llu nodes left, %llu records (%llu bubble, %llu off nodes, %llu isolated; %llu isolated below "
                   "the read length left out), %llu bytes\n",
                   (unsigned long long)ti.tips, (unsigned long long)ti.back_tips, (unsigned long long)ti.print.nodes, (unsigned long long)ti.nodes_before,
                   (unsigned long long)ti.print.records, (unsigned long long)ti.print.bubble_records, (unsigned long long)ti.print.node_contigs,
                   (unsigned long long)ti.print.isolated_kept, (unsigned long long)ti.print.isolated_dropped, (unsigned long long)bytes);
            clk.mark("  detipped contigs: plan, join, emission, file");
        }
    }
    if (o.dechimered_contigs || o.dechimered_graph) {  // the second step (src/ContigGraph.cpp:218-220) on the graph the first one left, which the context kept alive
        uint64_t bytes = 0;
        fgpu_chimera_info ci;
        if (fgpu_stage3_dechimera(ctx, &bytes, &ci) != FGPU_OK) {
            const char* what = o.dechimered_graph ? "dechimered_graph" : "dechimered_contigs";
            fprintf(stderr, "--%s: %s: no %s.%s.%s is written\n", what, fgpu_last_error(ctx), o.file_prefix.c_str(), what, o.dechimered_graph ? "fastg" : "fasta");
            return 2;
        }
        std::vector<char> contigs_text;
        if (o.dechimered_contigs) {
            if (int rc = take_file(contigs_text, bytes)) return rc;
        }
        if (o.dechimered_graph) {
            uint64_t graph_bytes = 0;
            fgpu_fastg_info gi;
            const int call_rc = fgpu_stage3_graph_fastg(ctx, &graph_bytes, &gi);
            if (int rc = write_graph("dechimered_graph", call_rc, graph_bytes, gi)) return rc;
            clk.mark("  dechimered graph: plan, join, emission, file");
        }
        if (o.dechimered_contigs) {
            if (int rc = put_file(o.file_prefix + ".dechimered_contigs.fasta", contigs_text, bytes)) return rc;
            printf("Dechimered contigs: %d chimeric extensions removed, %d of %d nodes left, %d records\n", (int)ci.removed, (int)ci.print.nodes, (int)ci.nodes_before,
                   (int)ci.print.records);
            clk.mark("  dechimered contigs: summaries, plan step, join, emission, file");
        }
    }
    return 0;
}

// What both kinds of run -- one device, or read shards over several -- do once the scan has ended: the lines ReadScanner::scanReads and
// printScanSummary print (src/ReadScanner.cpp:19-27,352-358), the junction map (held by `ctx`: the only context, or the last shard's) into
// <prefix>.junctions in the reference's dump order, and the pair filter files (src/Faucet.cpp:296-300).  0, or the exit code of a failure.
int write_scan_outputs(const Options& o, fgpu_ctx* ctx, const fgpu_scan_stats& ss, uint64_t empty_count, uint64_t not_empty_count, double seconds,
                       const PairFilter& short_pf, const PairFilter& long_pf, PhaseClock& clk) {
    printf("Empty count: %d, not empty count: %d\n", (int)empty_count, (int)not_empty_count);
    printf("Reads processed: %llu\n", (unsigned long long)ss.reads_processed);
    printf("Unambiguous reads: %llu\n", (unsigned long long)ss.unambiguous_reads);
    printf("Time in seconds for read scan: %f \n", seconds);
    printf("\nDistinct junctions: %llu \n", (unsigned long long)ss.n_junctions);
    printf("Number of kmers that we j-checked: %llu \n", (unsigned long long)ss.nb_jcheck_kmer);
    printf("Number of reads with no junctions: %llu \n", (unsigned long long)ss.nb_no_juncs);
    printf("Number of processed kmers: %llu \n", (unsigned long long)ss.nb_processed);
    printf("Number of skipped kmers: %llu \n", (unsigned long long)ss.nb_skipped);
    printf("Reads without errors: %llu\n", (unsigned long long)ss.reads_no_errors);

    // junction records come back in creation order; the reference's container gives the reference's dump order
    uint64_t n = 0;
    CHECK(fgpu_scan_junction_count(ctx, &n));
    std::vector<uint64_t> keys(n ? n : 1);
    std::vector<fgpu_junction> recs(n ? n : 1);
    CHECK(fgpu_scan_download_junctions(ctx, keys.data(), recs.data(), keys.size(), &n));
    clk.mark("  junction download");
    // the reference's dump order = the iteration order of its container after these insertions (junction_order.h).  Round 6: computed on the DEVICE
    // from the closed form of what the container does to its node list (fgpu_scan_dump_order: one radix sort per stretch between rehashes; the host
    // replay was 5.7 s of a 9.5 s run at config 5's 2.95e7 junctions) -- after the device has shown, on a prefix of these very keys, that it agrees
    // with the host's replay, which has shown that it agrees with a real container.  Anything else falls back to the replay, or to the container.
    std::vector<uint32_t> order;
    const size_t prefix = (size_t)std::min<uint64_t>(n, 50000);
    const bool replay_ok = DumpOrder::agrees_with_the_container(keys.data(), prefix);
    bool on_device = false;
    if (replay_ok && n) {
        auto device_order = [&](size_t m, std::vector<uint32_t>* out) -> bool {
            const std::vector<DumpOrder::Rehash> sch = DumpOrder::schedule(m);
            std::vector<uint64_t> counts, buckets;
            for (const DumpOrder::Rehash& r : sch) { counts.push_back(r.count); buckets.push_back(r.buckets); }
            out->assign(m, 0);
            return fgpu_scan_dump_order(ctx, counts.data(), buckets.data(), counts.size(), m, out->data()) == FGPU_OK;
        };
        std::vector<uint32_t> head;
        if (device_order(prefix, &head) && head == DumpOrder::of(keys.data(), prefix) && device_order((size_t)n, &order)) on_device = true;
        if (on_device && getenv("FAUCET_DEBUG_DUMP_ORDER_CHECK")) {     // (tests, measurements: the whole order against the host replay)
            const bool same = order == DumpOrder::of(keys.data(), (size_t)n);
            fprintf(stderr, "[cli] dump order of %llu junctions on the device %s the host replay's\n", (unsigned long long)n, same ? "equals" : "DIFFERS FROM");
            if (!same) return 2;
        }
    }
    if (!on_device) {
        if (replay_ok) {
            order = DumpOrder::of(keys.data(), (size_t)n);
        } else {   // a standard library that links its nodes another way: ask the container itself
            order.clear();
            std::unordered_map<uint64_t, uint32_t> container;
            for (uint64_t i = 0; i < n; i++) container.insert(std::pair<uint64_t, uint32_t>(keys[i], (uint32_t)i));
            for (const auto& kv : container) order.push_back(kv.second);
        }
    }
    if (clk.on) fprintf(stderr, "[cli]   dump order %s\n", on_device ? "on the device (fgpu_scan_dump_order)" : replay_ok ? "by the host replay" : "by the container");
    clk.mark("  dump order");
    // JunctionMap::writeToFile (utils/JunctionMap.cpp:579-596) first counts the junctions that are solid at thresholds 0..4
    // (Junction::isSolid, utils/Junction.cpp:38-46: more than one of the four extensions with that much coverage)
    for (int thr = 0; thr < 5; thr++) {
        long solid = 0;
        for (uint64_t i = 0; i < n; i++) {
            int paths = 0;
            for (int e = 0; e < 4; e++) paths += recs[i].cov[e] >= thr ? 1 : 0;
            solid += paths > 1 ? 1 : 0;
        }
        printf("There are %ld junctions with solidity at least %d.\n", solid, thr);
    }
    printf("Writing to junction file\n");
    if (int rc = write_junctions(o.file_prefix + ".junctions", keys.data(), recs.data(), order, o.k)) return rc;
    printf("Done writing to junction file\n");
    clk.mark("junction download + dump");
    if (!o.no_cleaning) {   // src/Faucet.cpp:297-300
        if (int rc = short_pf.dump(o.file_prefix + ".short_pair_filter")) return rc;
        printf("bloom dumped \n");                                   // (Bloom::dump's line, utils/Bloom.cpp:571-578: once per filter written)
        if (o.paired_ends) {
            if (int rc = long_pf.dump(o.file_prefix + ".long_pair_filter")) return rc;
            printf("bloom dumped \n");
        }
    }
    printf("Weight of short pair filter: %f\n", short_pf.weight());
    if (o.paired_ends) printf("Weight of long pair filter: %f\n", long_pf.weight());
    printf("Number of junctions: %llu\n", (unsigned long long)order.size());
    if (o.raw_contigs || o.detipped_contigs || o.dechimered_contigs || o.raw_graph || o.detipped_graph || o.dechimered_graph) return write_raw_contigs(o, ctx, keys.data(), recs.data(), order, clk);
    return 0;
}

namespace {

using faucet_host::ShardedRun;

// The device side of a run: one context, or -- `-gpus N` -- read shards over N GPUs, one host thread per device (shard_host.h): shard r = the
// r-th file-order share of the records, on device r (with fewer devices than shards several shards share a device: what a one-GPU box can
// test).  Same files, same log, same exit codes either way; what differs is who does the two passes.
// fgpu_create returns while a thread of the library is still creating the walk's streams and loading code objects: every way out of main
// goes through fgpu_destroy (here, or in ~ShardedRun), which joins it, before the HIP runtime is torn down.  The one exception is
// the _exit at the very end, after both passes -- the first scan call has joined the thread by then.
struct Run {
    fgpu_ctx* one = nullptr;
    std::unique_ptr<ShardedRun> shards;
    ~Run() { close(); }
    void close() {
        shards.reset();
        if (one) { fgpu_destroy(one); one = nullptr; }
    }
    std::vector<fgpu_ctx*> contexts() const {
        if (!shards) return std::vector<fgpu_ctx*>(1, one);
        std::vector<fgpu_ctx*> all;
        for (int r = 0; r < shards->n_ranks(); r++) all.push_back(shards->ctx(r));
        return all;
    }
    fgpu_ctx* first() const { return shards ? shards->first_ctx() : one; }
    fgpu_ctx* last() const { return shards ? shards->last_ctx() : one; }      // holds the run's junction map and pair filters after pass 2
};

// bloo2's bytes and the thread that writes them to <prefix>.bloom (Bloom::dump, utils/Bloom.cpp:571-578) beside pass 2: every way out of main
// waits for the file to be complete (the destructor), and every SUCCESSFUL way out looks at how the write went (complete(): a short write
// of --just_load_bloom's only output is not exit code 0)
class BloomFile {
public:
    BloomFile(const std::string& prefix, uint64_t tai) : bytes((size_t)(tai / 8)), path_(prefix + ".bloom") {}
    ~BloomFile() { if (writer_.joinable()) writer_.join(); }
    std::vector<uint8_t> bytes;
    // the bytes are in host memory; writing them out (64 MiB - 1 GiB) is waited for before the process ends
    int start_writing() {
        FILE* f = fopen(path_.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", path_.c_str()); return 2; }
        writer_ = std::thread([this, f] {
            if (fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) failed_ = true;
            if (fclose(f) != 0) failed_ = true;
        });
        return 0;
    }
    bool complete() {
        if (writer_.joinable()) writer_.join();
        if (failed_) fprintf(stderr, "cannot write %s\n", path_.c_str());
        return !failed_;
    }
private:
    const std::string path_;
    std::thread writer_;
    bool failed_ = false;      // (written by the writer, read behind its join)
};

// ---- filter sizing: getBloomFilterFromReads / getBloomFilterFromFile (src/Faucet.cpp:185-219).  0, or exit code 1
int size_filters(Options& o) {
    int32_t bits = 0;
    if (o.from_bloom) {
        if (o.two_hash) fgpu_size_two_hash(o.estimated_kmers, o.fp_rate, &bits, &o.tai, &o.n_hash);
        else fgpu_size_optimal(o.estimated_kmers, o.fp_rate, &bits, &o.tai, &o.n_hash);
        printf("Bits per kmer: %d \n", bits);                       // create_bloom_filter_2_hash / _optimal, utils/Bloom.cpp:204-247
        if (o.two_hash) {
            printf("Estimated items: %llu \n", (unsigned long long)o.estimated_kmers);
            printf("Estimated bloom size: %llu .\n", (unsigned long long)(o.estimated_kmers * (uint64_t)bits));
        }
        printf("BF memory: %f MB\n", (float)((o.estimated_kmers * (uint64_t)bits) / 8ULL / 1024ULL) / 1024);
        printf("Number of hash functions: %d \n", o.n_hash);
        return 0;
    }
    int32_t iters = 0;
    const double p1 = fgpu_solve_p1(o.estimated_kmers, o.singletons, o.fp_rate, &iters);
    if (p1 < 0) {   // the reference prints a message and goes on with nonsense sizes; we refuse
        fprintf(stderr, "Signs of f(lower_bound) and f(upper_bound) must be opposites: check -singletons (must be > 0)\n");
        return 1;
    }
    printf("After %d iterations the root is: %g\n", iters, p1);
    printf("p2 is %g p1 estimated as %g\n", (double)o.fp_rate, p1);
    fgpu_size_optimal(o.estimated_kmers, (float)p1, &bits, &o.tai, &o.n_hash);
    for (int i = 0; i < 2; i++) {   // printed once per filter, utils/Bloom.cpp:234-243
        printf("Bits per kmer: %d \n", bits);
        printf("BF memory: %f MB\n", (float)((o.estimated_kmers * (uint64_t)bits) / 8ULL / 1024ULL) / 1024);
        printf("Number of hash functions: %d \n", o.n_hash);
    }
    return 0;
}

fgpu_params context_params(const Options& o) {
    fgpu_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.k = o.k;
    prm.j = o.j;
    prm.max_spacer_dist = o.max_spacer_dist;
    prm.n_hash = o.n_hash;
    prm.tai = o.tai;
    // scanInputRead's lists feed the pair filters and the pair counts, all on the device (scan_pass.h); with --no_cleaning only the paired-end
    // loop's two counts are left of them
    if (!o.no_cleaning || o.paired_ends) prm.flags |= FGPU_FLAG_RECORD_STOPS;
    prm.flags |= FGPU_FLAG_KEY_ORDER_FROM_START;   // real genomes have repeats: a few launches per window against a first batch walked by cluster
    if (o.mercy) prm.flags |= FGPU_FLAG_MERCY;
    return prm;
}

// the size of the larger of the inputs that are regular files; false if one of them is something else (a pipe)
bool largest_input(const Options& o, uint64_t* largest) {
    bool all_regular = true;
    *largest = 0;
    for (const std::string* f : {&o.read_load_file, &o.read_scan_file}) {
        struct stat st;
        if (f->empty()) continue;
        if (stat(f->c_str(), &st) == 0 && S_ISREG(st.st_mode)) *largest = std::max<uint64_t>(*largest, (uint64_t)st.st_size);
        else all_regular = false;
    }
    return all_regular;
}

// The text buffers are page-locked, and pinning costs time in proportion (2 x 80 MB: ~40 ms beside the context's creation, on the same
// driver): input files that are smaller than a chunk -- the reference's own test case is 100 KB -- get buffers of their size.
void choose_chunk_bytes(Options& o) {
    o.chunk_bytes = o.chunk_mb << 20;
    uint64_t largest = 0;
    if (largest_input(o, &largest) && largest + (1u << 20) < o.chunk_bytes) o.chunk_bytes = ((largest >> 20) + 1) << 20;
}

// the options of the run's read shards (and of pass 0's, which runs on the same devices over the same transport)
faucet_host::ShardOptions shard_options_of(const Options& o, const fgpu_params& prm) {
    // every shard reads its share through buffers of its own: chunks no larger than a share needs
    uint64_t chunk_bytes = o.chunk_bytes, largest = 0;
    largest_input(o, &largest);
    const bool all_regular = largest_input(o, &largest);
    const uint64_t share = largest / (uint64_t)o.gpus + (4u << 20);
    if (all_regular && share < chunk_bytes) chunk_bytes = ((share >> 20) + 1) << 20;      // (a pipe's size is not known: the chunks -chunk_mb asks for)
    faucet_host::ShardOptions so = faucet_host::shard_options(o.gpus, o.transport == "rccl" ? FGPU_TRANSPORT_RCCL : FGPU_TRANSPORT_COPY, prm, o.fastq, o.mercy,
                                                              o.paired_ends, o.no_cleaning, chunk_bytes);
    so.scan_kept = o.scan_kept && ShardedRun::slices_asked();
    return so;
}

// ---- the run's contexts.  0, or the exit code of a failure
int open_shards(const Options& o, const fgpu_params& prm, bool verbose, Run* run) {
    if (o.batch_reads) { fprintf(stderr, "-batch_reads (records split on the host) cannot be combined with -gpus: the shards split their records on their devices\n"); return 1; }
    const bool slices = ShardedRun::slices_asked();
    for (const std::string* f : {&o.read_load_file, &o.read_scan_file}) {      // (before any device is touched)
        struct stat st;
        if (o.from_bloom && f == &o.read_load_file) continue;
        // --scan_kept under filter slices: -read_load_file is read once and may be a pipe; a scan file, where one was given, is only looked
        // at if pass 2 has to fall back to it
        if (slices && o.scan_kept && f == &o.read_scan_file) continue;
        if (stat(f->c_str(), &st) != 0) { fprintf(stderr, "cannot open %s\n", f->c_str()); return 2; }
        if (slices && o.scan_kept && f == &o.read_load_file) continue;
        if (!S_ISREG(st.st_mode)) {
            if (slices)
                fprintf(stderr, "%s is not a regular file: under FAUCET_SHARD_PROTOCOL=slices a pipe can be the run's only input with --scan_kept (pass 2 then scans "
                                "the reads pass 1 kept); without it there is no second stream to shard\n", f->c_str());
            else
                fprintf(stderr, "%s is not a regular file: with -gpus the read shards are byte ranges of their input (pipes need -gpus 1)\n", f->c_str());
            return 2;
        }
    }
    const int ndev = fgpu_device_count();
    if (ndev < 1) { fprintf(stderr, "fgpu_create failed (%d): no gfx950 device\n", FGPU_ERR_HIP); return 2; }
    if (ndev < o.gpus) fprintf(stderr, "note: %d read shards on %d device%s: shards share devices\n", o.gpus, ndev, ndev == 1 ? "" : "s");
    faucet_host::ShardOptions so = shard_options_of(o, prm);
    so.verbose = verbose;
    run->shards.reset(new ShardedRun(so));
    if (int rc = run->shards->create()) { fprintf(stderr, "fgpu_create failed (%d): %s\n", rc, run->shards->error().c_str()); return 2; }
    return 0;
}

int open_one_device(const Options& o, const fgpu_params& prm, Run* run) {
    std::thread pin;   // the two text buffers, pinned beside the context's creation; joined before anything else can fail or read
    if (!o.batch_reads && !o.from_junctions)
        pin = std::thread([&o] { for (int i = 0; i < 2; i++) pinned_slot(i, kTextPad + o.chunk_bytes); });
    const int rc = fgpu_create(&prm, &run->one);
    if (pin.joinable()) pin.join();
    if (rc != FGPU_OK) { fprintf(stderr, "fgpu_create failed (%d): %s\n", rc, fgpu_last_error(nullptr)); return 2; }
    return 0;
}

// ---- -bloom_file (Bloom::load, utils/Bloom.cpp:580-587): the filter into every context
int load_bloom_file(const Options& o, const Run& run, BloomFile& bloom) {
    FILE* f = fopen(o.bloom_input_file.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", o.bloom_input_file.c_str()); return 2; }
    printf("loading bloom filter from file, nelem %llu \n", (unsigned long long)(o.tai / 8));
    const size_t got = fread(bloom.bytes.data(), 1, bloom.bytes.size(), f);
    fclose(f);
    // Bloom::load reads as many bytes as the filter it has just sized holds and does not look at fread's count: a longer file gives its
    // head, a shorter one leaves the rest of the (zeroed) filter empty -- e.g. the .bloom of a run that loaded from reads (sized with p1)
    // restarted with the sizes -fp implies.  Same here; a note on stderr is all that is added.
    if (got != bloom.bytes.size())
        fprintf(stderr, "note: %s holds %llu of the %llu bytes this run's filter has: the rest stays empty (as in the reference)\n",
                o.bloom_input_file.c_str(), (unsigned long long)got, (unsigned long long)(o.tai / 8));
    for (fgpu_ctx* ctx : run.contexts()) CHECK(fgpu_bloom_upload(ctx, FGPU_BLOO2, bloom.bytes.data(), bloom.bytes.size()));
    printf("bloom loaded\n");
    return 0;
}

// ---- the reading loop of every pass on one device: the batches of `src` in file order, each handed to `each` (a status); the time spent in
// `each` is added to *each_ms, `progress` (or null) is the line rewritten on stdout.  FGPU_OK, or the status that ended it with *failed = who
template <class Each>
int feed_batches(fgpu_ctx* ctx, BatchSource& src, const char* progress, double* each_ms, const char** failed, const Each& each) {
    uint64_t reads = 0;
    fgpu_reads r;
    for (int more; (more = src.next(ctx, &r)) != 0;) {
        if (more < 0) { *failed = "fgpu_text_split"; return -more; }
        const auto t_batch = std::chrono::steady_clock::now();
        if (int rc = each(&r)) return rc;
        *each_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_batch).count();
        reads += r.n_reads;
        if (progress) {
            fprintf(stdout, "\r%s: %lld", progress, (long long)reads);
            fflush(stdout);
        }
    }
    return FGPU_OK;
}

// ---- pass 0 (--estimate): whichever of -estimated_kmers / -singletons the command line left out, from a sketch of -read_load_file.  The sizes
// of the run's contexts follow from these numbers, so the pass has placeholder contexts of its own (tai = 128, one hash function: the pass
// reads neither), destroyed before the run's contexts are made.  With -gpus N every rank sketches its read shard and the sketches are merged
// (ShardedRun::estimate): the same counts, hence the same two lines and the same run, as from the first device alone -- which is what
// FAUCET_ESTIMATE_SHARDS=0 (A/B timing, tests), a library without fgpu_group_estimate_end and -batch_reads (refused by open_shards, behind
// pass 0) still get.  0, or the exit code of a failure
// The packed reads pass 0 kept for pass 1 (fgpu_estimate_take_kept): device blocks that belong to this program until a context adopts them
// (fgpu_load_batch_packed).  What is left when a run ends early goes back through whichever context is at hand.
struct KeptReads {
    bool asked = false;               // pass 0 is to keep its batches ...
    bool must = false;                // ... and the run cannot go on without them: -read_load_file cannot be read again
    bool have = false;                // it did, and `blocks` are all of -read_load_file
    uint64_t budget = 0, bytes = 0;   // the budget the pass had, what its blocks are charged
    std::vector<fgpu_packed> blocks;
    bool with_reads = false;          // --scan_kept: every block came with its read offsets (fgpu_estimate_keep_reads), adopted with it
    std::vector<fgpu_kept_reads> reads;
    size_t next = 0;                  // blocks before this one have been adopted
    void release(fgpu_ctx* ctx) {
        for (; ctx && next < blocks.size(); next++) {
            (void)fgpu_device_free(ctx, blocks[next].block_dev);
            if (next < reads.size()) (void)fgpu_device_free(ctx, reads[next].offsets_dev);
        }
        blocks.clear();
        reads.clear();
        next = 0;
        have = false;
    }
};

const int kStoppedKeeping = 1000;     // estimate_one_device's batch callback: not a status of the library

int estimate_one_device(const Options& o, const fgpu_params& prm, PhaseClock& clk, fgpu_estimate* est, KeptReads* kept) {
    Run placeholder;
    if (int rc = open_one_device(o, prm, &placeholder)) return rc;
    fgpu_ctx* ctx = placeholder.one;
    clk.mark("arguments, placeholder context");
    BatchSource src(o, o.read_load_file);
    if (!src.is_open()) { fprintf(stderr, "cannot open %s\n", o.read_load_file.c_str()); return 2; }
    CHECK(fgpu_estimate_begin(ctx, o.estimate_bits));
    bool keeping = false;
    if (kept->asked) {      // what a context sets aside for resident batches: what pass 0 keeps, the run's context can hold
        CHECK(fgpu_load_fixup_state(ctx, nullptr, &kept->budget));
        if (const char* cap = getenv("FAUCET_ESTIMATE_KEEP_BYTES")) kept->budget = std::min<uint64_t>(kept->budget, strtoull(cap, nullptr, 10));   // (tests)
        CHECK(fgpu_estimate_keep(ctx, kept->budget));
        if (kept->with_reads) CHECK(fgpu_estimate_keep_reads(ctx));
        keeping = true;
    }
    double batch_ms = 0;
    const char* failed = "fgpu_estimate_batch";
    const int frc = feed_batches(ctx, src, nullptr, &batch_ms, &failed, [&](const fgpu_reads* r) -> int {
        if (int rc = fgpu_estimate_batch(ctx, r)) return rc;
        if (!keeping) return FGPU_OK;
        int still = 0;
        uint64_t bytes = 0;
        if (int rc = fgpu_estimate_keep_state(ctx, &still, nullptr, &bytes)) { failed = "fgpu_estimate_keep_state"; return rc; }
        if (still) { kept->bytes = bytes; return FGPU_OK; }
        keeping = false;
        if (kept->must) return kStoppedKeeping;
        fprintf(stderr, "note: --estimate: pass 0 stopped keeping its packed reads (%llu bytes kept, budget %llu bytes): pass 1 reads %s again\n",
                (unsigned long long)kept->bytes, (unsigned long long)kept->budget, o.read_load_file.c_str());
        return FGPU_OK;
    });
    if (frc == kStoppedKeeping) {      // (the source and the placeholder go on the way out: a writer at the other end of a pipe is not left waiting)
        fprintf(stderr, "--estimate: the packed reads of %s do not fit the device memory set aside for them (%llu bytes kept, budget %llu bytes) and a pipe "
                        "cannot be read again for pass 1: give -estimated_kmers and -singletons\n",
                o.read_load_file.c_str(), (unsigned long long)kept->bytes, (unsigned long long)kept->budget);
        return 2;
    }
    if (frc) {
        fprintf(stderr, "%s failed (%d): %s\n", failed, frc, fgpu_last_error(ctx));
        return 2;
    }
    const int rc = fgpu_estimate_end(ctx, est);
    if (rc == FGPU_ERR_CAPACITY) { fprintf(stderr, "--estimate: the sketch of 2^%d cells per level is too full for these reads: raise -estimate_bits\n", (int)est->r_bits); return 2; }
    if (rc != FGPU_OK) { fprintf(stderr, "fgpu_estimate_end failed (%d): %s\n", rc, fgpu_last_error(ctx)); return 2; }
    if (keeping) {
        uint64_t n = 0;
        CHECK(fgpu_estimate_keep_state(ctx, nullptr, &n, &kept->bytes));
        kept->blocks.resize((size_t)n);
        CHECK(fgpu_estimate_take_kept(ctx, kept->blocks.data(), n, &n));
        kept->have = true;
        if (kept->with_reads) {
            kept->reads.resize((size_t)n);
            CHECK(fgpu_estimate_take_kept_reads(ctx, kept->reads.data(), n, &n));
        }
    }
    if (clk.on) fprintf(stderr, "[cli]   %.2f ms in fgpu_estimate_batch calls; %llu k-mers sketched, 2^%d cells per level, estimates from level %d on\n", batch_ms,
                        (unsigned long long)est->kmers, (int)est->r_bits, (int)est->level);
    if (clk.on && kept->have) fprintf(stderr, "[cli]   %llu bytes of packed reads kept in %llu blocks (budget %llu bytes)\n", (unsigned long long)kept->bytes,
                                      (unsigned long long)kept->blocks.size(), (unsigned long long)kept->budget);
    clk.mark(kept->have ? "pass 0 (read + estimate, reads kept)" : "pass 0 (read + estimate)");
    return 0;
}

int estimate_shards(const Options& o, const fgpu_params& prm, PhaseClock& clk, fgpu_estimate* est) {
    if (fgpu_device_count() < 1) { fprintf(stderr, "fgpu_create failed (%d): no gfx950 device\n", FGPU_ERR_HIP); return 2; }
    faucet_host::ShardOptions so = shard_options_of(o, prm);
    so.verbose = clk.on;
    ShardedRun placeholder(so);
    if (int rc = placeholder.create()) { fprintf(stderr, "fgpu_create failed (%d): %s\n", rc, placeholder.error().c_str()); return 2; }
    clk.mark("arguments, placeholder contexts");
    std::vector<uint64_t> kmers;
    const int rc = placeholder.estimate(o.read_load_file, o.estimate_bits, est, &kmers);
    if (rc == FGPU_ERR_CAPACITY) { fprintf(stderr, "--estimate: the sketch of 2^%d cells per level is too full for these reads: raise -estimate_bits\n", (int)est->r_bits); return 2; }
    if (rc != FGPU_OK) { fprintf(stderr, "estimate pass failed (%d): %s\n", rc, placeholder.error().c_str()); return 2; }
    if (clk.on) {
        for (size_t r = 0; r < kmers.size(); r++) fprintf(stderr, "[cli]   rank %d: %llu k-mers sketched\n", (int)r, (unsigned long long)kmers[r]);
        fprintf(stderr, "[cli]   %llu k-mers sketched over %d read shards, 2^%d cells per level, estimates from level %d on\n", (unsigned long long)est->kmers, o.gpus,
                (int)est->r_bits, (int)est->level);
    }
    clk.mark("pass 0 (shards)");      // (the placeholder contexts go as the one-device pass' does: behind the mark)
    return 0;
}

int estimate_missing(Options& o, PhaseClock& clk, KeptReads* kept) {
    // decided before any device call: the file is read once more by pass 1 -- unless pass 0 can keep what it packs --, and the library has to have the pass
    struct stat st;
    const bool can_keep = fgpu_estimate_keep && fgpu_estimate_keep_state && fgpu_estimate_take_kept && fgpu_load_batch_packed;
    const bool found = stat(o.read_load_file.c_str(), &st) == 0, regular = found && S_ISREG(st.st_mode);
    if (!found || (!regular && !can_keep)) {
        fprintf(stderr, "--estimate: %s is not a regular file: pass 0 reads -read_load_file once more than the run does (give -estimated_kmers and -singletons for a pipe)\n",
                o.read_load_file.c_str());
        return 1;
    }
    if (!regular && o.gpus > 1 && !o.from_bloom) {      // open_shards would say so with pass 0 behind it and the pipe consumed
        fprintf(stderr, "%s is not a regular file: with -gpus the read shards are byte ranges of their input (pipes need -gpus 1)\n", o.read_load_file.c_str());
        return 2;
    }
    // Pass 1 from what pass 0 packed: where the input cannot be read twice, and on request (FAUCET_ESTIMATE_KEEP=1: measurements) for files.
    // One device only; with -bloom_file no pass 1 follows and a pipe is simply sketched once.
    const char* keep_env = getenv("FAUCET_ESTIMATE_KEEP");
    kept->must = !regular && !o.from_bloom;
    kept->asked = can_keep && !o.from_bloom && o.gpus == 1 && (!regular || (keep_env && keep_env[0] == '1'));
    kept->with_reads = kept->asked && o.scan_kept;      // (main has seen to it that the library has the entry points)
    if (!fgpu_estimate_begin || !fgpu_estimate_batch || !fgpu_estimate_end) {
        fprintf(stderr, "--estimate: the library this program is linked against lacks the entry points of the estimate pass "
                        "(fgpu_estimate_begin, fgpu_estimate_batch, fgpu_estimate_end)\n");
        return 2;
    }
    fgpu_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.k = o.k;
    prm.j = 1;
    prm.max_spacer_dist = 100;
    prm.n_hash = 1;
    prm.tai = 128;
    const char* by_shards_env = getenv("FAUCET_ESTIMATE_SHARDS");
    const bool by_shards = o.gpus > 1 && regular && !o.from_junctions && !o.batch_reads && ShardedRun::estimate_linked() && !(by_shards_env && by_shards_env[0] == '0');
    fgpu_estimate est;
    memset(&est, 0, sizeof(est));
    if (int rc = by_shards ? estimate_shards(o, prm, clk, &est) : estimate_one_device(o, prm, clk, &est, kept)) return rc;
    const long long f0 = llround(est.f0), f1 = std::max(llround(est.f1), 1LL);
    printf("Estimated distinct k-mers (F0): %lld\n", f0);
    printf("Estimated singletons (f1): %lld\n", f1);
    if (!o.est_kmers_flag) o.estimated_kmers = (uint64_t)f0;
    if (!o.est_sing_flag) o.singletons = (uint64_t)f1;
    return 0;
}

// (both ways of pass 1 answer with a ShardLoadResult: the run's counters and the weights of bloo1 / bloo2)
int load_one_device(fgpu_ctx* ctx, BatchSource& src, PhaseClock& clk, faucet_host::ShardLoadResult* out, bool keep_reads) {
    CHECK(fgpu_load_begin(ctx, keep_reads ? FGPU_LOAD_KEEP_READS : 0));
    const char* failed = "fgpu_load_batch";
    if (int rc = feed_batches(ctx, src, "reads consumed", &clk.batch_ms, &failed, [&](const fgpu_reads* r) { return fgpu_load_batch(ctx, r); })) {
        fprintf(stderr, "%s failed (%d): %s\n", failed, rc, fgpu_last_error(ctx));
        return 2;
    }
    const auto t_end = std::chrono::steady_clock::now();
    CHECK(fgpu_load_end(ctx, &out->stats));
    if (clk.on) fprintf(stderr, "[cli]   %.2f ms in fgpu_load_batch calls, %.2f ms in fgpu_load_end\n", clk.batch_ms,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_end).count());
    clk.mark(keep_reads ? "pass 1 (read + load, reads kept)" : "pass 1 (read + load)");
    CHECK(fgpu_bloom_weight(ctx, FGPU_BLOO1, &out->w1));
    CHECK(fgpu_bloom_weight(ctx, FGPU_BLOO2, &out->w2));
    return 0;
}

// ... from the blocks pass 0 kept: the same pass, a block where load_one_device has a batch of the file.  Blocks the context has not adopted
// when the pass fails are still the caller's (KeptReads::release)
int load_kept(fgpu_ctx* ctx, KeptReads& kept, PhaseClock& clk, faucet_host::ShardLoadResult* out) {
    CHECK(fgpu_load_begin(ctx, kept.with_reads ? FGPU_LOAD_KEEP_READS : 0));
    uint64_t reads = 0;
    for (; kept.next < kept.blocks.size(); kept.next++) {
        const auto t_batch = std::chrono::steady_clock::now();
        if (kept.with_reads) CHECK(fgpu_load_batch_packed_reads(ctx, &kept.blocks[kept.next], &kept.reads[kept.next]));
        else CHECK(fgpu_load_batch_packed(ctx, &kept.blocks[kept.next]));
        clk.batch_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_batch).count();
        reads += kept.blocks[kept.next].n_reads;
        fprintf(stdout, "\rreads consumed: %lld", (long long)reads);
        fflush(stdout);
    }
    const auto t_end = std::chrono::steady_clock::now();
    CHECK(fgpu_load_end(ctx, &out->stats));
    if (clk.on) fprintf(stderr, "[cli]   %.2f ms in fgpu_load_batch_packed calls, %.2f ms in fgpu_load_end\n", clk.batch_ms,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_end).count());
    clk.mark(kept.with_reads ? "pass 1 (load from kept reads, reads kept)" : "pass 1 (load from kept reads)");
    CHECK(fgpu_bloom_weight(ctx, FGPU_BLOO1, &out->w1));
    CHECK(fgpu_bloom_weight(ctx, FGPU_BLOO2, &out->w2));
    return 0;
}

int load_shards(const Options& o, ShardedRun& run, PhaseClock& clk, faucet_host::ShardLoadResult* out) {
    if (int rc = run.load(o.read_load_file, out)) { fprintf(stderr, "load pass failed (%d): %s\n", rc, run.error().c_str()); return 2; }
    clk.mark(out->slices && run.reads_kept() ? "pass 1 (shards, filter slices, reads kept)" : out->slices ? "pass 1 (shards, filter slices)" : out->fixup ? "pass 1 (shards, fix-up protocol)" : "pass 1 (shards, presence protocol)");
    fprintf(stdout, "\rreads consumed: %lld", (long long)out->stats.reads_processed);
    return 0;
}

// ---- pass 1 (load_two_filters, utils/Bloom.cpp:267-350), and bloo2 on its way into <prefix>.bloom
int load_from_reads(const Options& o, const Run& run, PhaseClock& clk, BloomFile& bloom, KeptReads& kept) {
    std::unique_ptr<BatchSource> src;      // (one device; the shards open their byte ranges themselves; kept reads need no source)
    if (!run.shards && !kept.have) {
        src.reset(new BatchSource(o, o.read_load_file));
        if (!src->is_open()) { fprintf(stderr, "cannot open %s\n", o.read_load_file.c_str()); return 2; }   // the reference silently reads nothing
    }
    time_t start, stop;
    time(&start);
    printf("Weights before load: %f, %f \n", 0.0f, 0.0f);
    faucet_host::ShardLoadResult lo;
    if (int rc = run.shards ? load_shards(o, *run.shards, clk, &lo) : kept.have ? load_kept(run.one, kept, clk, &lo) : load_one_device(run.one, *src, clk, &lo, o.scan_kept)) return rc;
    printf("\n");
    printf("Weights after load: %f, %f \n", lo.w1, lo.w2);
    printf("Reads processed: %llu\n", (unsigned long long)lo.stats.reads_processed);
    printf("Unambiguous reads: %llu\n", (unsigned long long)lo.stats.unambiguous_reads);
    time(&stop);
    printf("Time to load: %f \n", difftime(stop, start));
    fgpu_ctx* ctx = run.first();           // (every context holds the run's bloo2)
    CHECK(fgpu_bloom_download(ctx, FGPU_BLOO2, bloom.bytes.data(), bloom.bytes.size()));
    if (int rc = bloom.start_writing()) return rc;
    printf("bloom dumped \n");
    clk.mark("bloom download (dump beside pass 2)");
    return 0;
}

// ---- pair filters (src/Faucet.cpp:266-283): created, and their sizes printed, before --just_load_bloom returns
void create_pair_filters(const Options& o, PairFilter* short_pf, PairFilter* long_pf) {
    const uint64_t E = o.estimated_kmers;
    // mercy k-mers lead to more junctions: the reference doubles both filters (src/Faucet.cpp:268-271)
    short_pf->create(o.high_cov ? E / 2 : o.mercy ? E / 10 : E / 20, 0.01f);
    if (o.paired_ends) long_pf->create(o.high_cov ? E / 2 : o.mercy ? E / 5 : E / 10, 0.01f);
}

// ---- -junctions_file <prefix> (src/Faucet.cpp:104-109,289-293): the scan's three files are reloaded instead of being made.  What the
// reference does next is its contig graph, which is not part of this build: the files are parsed and checked (sizes as the flags imply),
// the lines the reference prints after reloading are printed, and the program stops where every run of this build stops (exit code 3).
int reload_scan_files(const Options& o, PairFilter& short_pf, PairFilter& long_pf) {
    JunctionTable junction_map;
    printf("Reading from Junction file to build junction map.\n");
    const long n_lines = read_junctions(o.junctions_prefix + ".junctions", o.k, junction_map);
    if (n_lines < 0) { fprintf(stderr, "cannot read %s.junctions (missing, or not in the .junctions format for k = %d)\n", o.junctions_prefix.c_str(), o.k); return 2; }
    if (int rc = load_pair_filter(short_pf, o.junctions_prefix + ".short_pair_filter")) return rc;
    if (o.paired_ends)
        if (int rc = load_pair_filter(long_pf, o.junctions_prefix + ".long_pair_filter")) return rc;
    printf("Weight of short pair filter: %f\n", short_pf.weight());
    if (o.paired_ends) printf("Weight of long pair filter: %f\n", long_pf.weight());
    printf("Number of junctions: %llu\n", (unsigned long long)junction_map.size());
    fprintf(stderr, "The contig-graph stage is not part of this build: -bloom_file / -junctions_file inputs have been read and checked; the\n"
                    "reference continues from them.\n");
    return 0;
}

// FGPU_CLI_TIMES: what the library counted during pass 2
void tell_scan_diagnostics(const Options& o, fgpu_ctx* ctx) {
    uint64_t waits = 0;
    double wait_ms = 0;
    if (fgpu_diag_host_waits(ctx, &waits, &wait_ms) == FGPU_OK)
        fprintf(stderr, "[cli]   pass 2: the host waited for the device %llu times, %.2f ms in all\n", (unsigned long long)waits, wait_ms);
    uint64_t d[6] = {0, 0, 0, 0, 0, 0}, form[4] = {0, 0, 0, 0};
    if (o.paired_ends && !o.no_cleaning && fgpu_diag_long_pairs(ctx, d) == FGPU_OK) {
        if (fgpu_diag_long_pairs_state) (void)fgpu_diag_long_pairs_state(ctx, form);
        fprintf(stderr, "[cli]   long pair filter on the device: %llu first-end k-mers checked, %llu paired by the filter as their batch found it, %llu inserted; "
                        "%llu evaluation rounds over %llu batches (at most %llu in one); first-set times %s, at most %llu table slots in a batch\n",
                (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2], (unsigned long long)d[3], (unsigned long long)d[5], (unsigned long long)d[4],
                form[0] == 2 ? "sparse" : form[0] == 1 ? "dense" : "unknown", (unsigned long long)form[2]);
    }
    memset(d, 0, sizeof(d));
    if (fgpu_diag_ovw(ctx, d) == FGPU_OK && (d[2] || d[3] || d[5]))
        fprintf(stderr, "[cli]   large clusters, walked optimistically: %llu pieces, %llu rounds over %llu windows (%llu piece-rounds kept their log); "
                        "%llu windows left to the key-ordered walk, %llu to the walk by cluster\n",
                (unsigned long long)d[0], (unsigned long long)d[1], (unsigned long long)d[2], (unsigned long long)d[4], (unsigned long long)d[3],
                (unsigned long long)d[5]);
}

// pass 2 on the one device: scan_pass.h over this program's batches; the progress line and the phase clock are this side's
int scan_one_device(const Options& o, fgpu_ctx* ctx, PairFilter& short_pf, PairFilter& long_pf, PhaseClock& clk, faucet_host::ScanPassResult* res) {
    BatchSource src(o, o.read_scan_file);
    if (!src.is_open()) { fprintf(stderr, "cannot open %s\n", o.read_scan_file.c_str()); return 2; }
    const faucet_host::PairTarget none = {nullptr, 0, 0};
    const faucet_host::PairTarget short_target = {short_pf.bits.data(), short_pf.tai, short_pf.n_hash}, long_target = {long_pf.bits.data(), long_pf.tai, long_pf.n_hash};
    const auto t_pass = std::chrono::steady_clock::now();
    auto t_fed = t_pass;
    const int rc = faucet_host::scan_pass(ctx, o.k, o.no_cleaning ? none : short_target, o.no_cleaning || !o.paired_ends ? none : long_target, o.paired_ends,
        [&](const faucet_host::EachBatch& each) -> int {
            if (int frc = feed_batches(ctx, src, "reads scanned", &clk.scan_ms, &res->failed, each)) return frc;
            t_fed = std::chrono::steady_clock::now();
            return FGPU_OK;
        }, res);
    if (rc != FGPU_OK) { fprintf(stderr, "%s failed (%d): %s\n", res->failed, rc, fgpu_last_error(ctx)); return 2; }
    clk.take_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fed).count();
    if (clk.on) {
        fprintf(stderr, "[cli]   %.2f ms in fgpu_scan_batch calls, %.2f ms in fgpu_scan_end (the last walks, the last lists, the pair filters' last batches)\n",
                clk.scan_ms, clk.take_ms);
        tell_scan_diagnostics(o, ctx);
    }
    return 0;
}

// ... over the batches pass 1 kept (--scan_kept): no file is opened, a batch is fgpu_scan_batch_kept(i)
int scan_kept_one_device(const Options& o, fgpu_ctx* ctx, uint64_t n_batches, PairFilter& short_pf, PairFilter& long_pf, PhaseClock& clk, faucet_host::ScanPassResult* res) {
    const faucet_host::PairTarget none = {nullptr, 0, 0};
    const faucet_host::PairTarget short_target = {short_pf.bits.data(), short_pf.tai, short_pf.n_hash}, long_target = {long_pf.bits.data(), long_pf.tai, long_pf.n_hash};
    const auto t_pass = std::chrono::steady_clock::now();
    auto t_fed = t_pass;
    const int rc = faucet_host::scan_pass_kept(ctx, o.k, o.no_cleaning ? none : short_target, o.no_cleaning || !o.paired_ends ? none : long_target, o.paired_ends,
        n_batches, [&](uint64_t reads) {
            fprintf(stdout, "\rreads scanned: %lld", (long long)reads);
            fflush(stdout);
            t_fed = std::chrono::steady_clock::now();
        }, res);
    if (rc != FGPU_OK) { fprintf(stderr, "%s failed (%d): %s\n", res->failed, rc, fgpu_last_error(ctx)); return 2; }
    clk.scan_ms += std::chrono::duration<double, std::milli>(t_fed - t_pass).count();
    clk.take_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fed).count();
    if (clk.on) {
        fprintf(stderr, "[cli]   %.2f ms in fgpu_scan_batch_kept calls (%llu kept batches), %.2f ms in fgpu_scan_end (the last walks, the last lists, the pair filters' last batches)\n",
                clk.scan_ms, (unsigned long long)n_batches, clk.take_ms);
        tell_scan_diagnostics(o, ctx);
    }
    return 0;
}

// --scan_kept, after pass 1: did it keep every batch with its reads?  *from_kept: pass 2 scans them.  If not, pass 2 can still read
// -read_scan_file where one was given and the input is a file that can be read again (one note); otherwise the run ends here, exit code 2,
// with <prefix>.bloom written -- the restart that exists.  FAUCET_DEBUG_SCAN_KEPT_BUDGET=<bytes> (tests): "the device keeps this many bytes"
int decide_scan_kept(const Options& o, fgpu_ctx* ctx, BloomFile& bloom, const PhaseClock& clk, bool* from_kept, uint64_t* n_batches) {
    int complete = 0;
    uint64_t bytes = 0, budget = 0;
    CHECK(fgpu_scan_kept_state(ctx, &complete, n_batches, nullptr, &bytes));
    CHECK(fgpu_load_fixup_state(ctx, nullptr, &budget));
    if (const char* e = getenv("FAUCET_DEBUG_SCAN_KEPT_BUDGET")) {
        budget = std::min<uint64_t>(budget, strtoull(e, nullptr, 10));
        if (bytes > budget) { complete = 0; bytes = 0; }      // (as if the first batch had not fitted)
    }
    *from_kept = complete != 0;
    if (clk.on) fprintf(stderr, "[cli]   %llu bytes kept on the device in %llu batches (budget %llu bytes)%s\n", (unsigned long long)bytes, (unsigned long long)*n_batches,
                        (unsigned long long)budget, complete ? "" : ": not all of pass 1");
    if (complete) return 0;
    struct stat st;
    const bool regular = stat(o.read_load_file.c_str(), &st) == 0 && S_ISREG(st.st_mode);
    if (o.scan_file_flag && regular) {
        fprintf(stderr, "note: --scan_kept: pass 1 could not keep all of its reads on the device (%llu bytes kept, budget %llu bytes): pass 2 reads %s\n",
                (unsigned long long)bytes, (unsigned long long)budget, o.read_scan_file.c_str());
        return 0;
    }
    fprintf(stderr, "--scan_kept: pass 1 could not keep all of its reads on the device (%llu bytes kept, budget %llu bytes) and there is no input pass 2 could "
                    "read instead.  %s.bloom has been written: -bloom_file %s.bloom -read_scan_file <the reads> finishes the job\n",
            (unsigned long long)bytes, (unsigned long long)budget, o.file_prefix.c_str(), o.file_prefix.c_str());
    (void)bloom.complete();
    return 2;
}

// --scan_kept over filter slices, after pass 1: does every rank hold the reads of its range?  As decide_scan_kept: if not, a regular file that
// came with a -read_scan_file is scanned from the text (one note); otherwise the run ends here, exit code 2, with <prefix>.bloom written
int decide_scan_kept_shards(const Options& o, ShardedRun& run, BloomFile& bloom, bool* from_kept) {
    *from_kept = run.reads_kept();
    if (*from_kept) return 0;
    struct stat st;
    const bool regular = stat(o.read_load_file.c_str(), &st) == 0 && S_ISREG(st.st_mode);
    const bool scan_regular = o.scan_file_flag && stat(o.read_scan_file.c_str(), &st) == 0 && S_ISREG(st.st_mode);
    if (regular && scan_regular) {
        fprintf(stderr, "note: --scan_kept: the ranks could not keep all of their reads on the device (%llu bytes kept, budget %llu bytes): pass 2 reads %s\n",
                (unsigned long long)run.kept_bytes(), (unsigned long long)run.kept_budget(), o.read_scan_file.c_str());
        return 0;
    }
    fprintf(stderr, "--scan_kept: the ranks could not keep all of their reads on the device (%llu bytes kept, budget %llu bytes) and there is no input pass 2 could "
                    "read instead.  %s.bloom has been written: -bloom_file %s.bloom -read_scan_file <the reads> finishes the job\n",
            (unsigned long long)run.kept_bytes(), (unsigned long long)run.kept_budget(), o.file_prefix.c_str(), o.file_prefix.c_str());
    (void)bloom.complete();
    return 2;
}

// pass 2 over the read shards: the last shard ends with the run's junction map and pair filters, the counts are the sum over the shards
int scan_shards(const Options& o, ShardedRun& run, PairFilter& short_pf, PairFilter& long_pf, faucet_host::ScanPassResult* res, bool from_kept) {
    fgpu_ctx* ctx = run.last_ctx();
    run.set_pair_filters(o.no_cleaning ? 0 : short_pf.tai, short_pf.n_hash, o.paired_ends && !o.no_cleaning ? long_pf.tai : 0, long_pf.n_hash);
    faucet_host::ShardScanResult sr;
    if (int rc = run.scan(o.read_scan_file, &sr, from_kept)) { fprintf(stderr, "junction scan failed (%d): %s\n", rc, run.error().c_str()); return 2; }
    fprintf(stdout, "\rreads scanned: %lld", (long long)sr.stats.reads_processed);
    if (!o.no_cleaning) CHECK(fgpu_scan_short_pairs_download(ctx, short_pf.bits.data(), short_pf.bits.size()));
    if (o.paired_ends && !o.no_cleaning) {
        uint64_t e = 0, ne = 0;      // (this shard's counts)
        CHECK(fgpu_scan_long_pairs_download(ctx, long_pf.bits.data(), long_pf.bits.size(), &e, &ne));
    }
    res->stats = sr.stats;
    res->empty_count = sr.empty_count;
    res->not_empty_count = sr.not_empty_count;
    return 0;
}

// ---- pass 2 (ReadScanner::scanReads, src/ReadScanner.cpp:284-359; printScanSummary :19-27) and the files it makes
int scan_and_write(const Options& o, const Run& run, PairFilter& short_pf, PairFilter& long_pf, PhaseClock& clk, bool from_kept, uint64_t kept_batches) {
    time_t start, stop;
    time(&start);
    float w2 = 0;
    fgpu_ctx* ctx = run.last();
    CHECK(fgpu_bloom_weight(ctx, FGPU_BLOO2, &w2));
    printf("Weight before read scan: %f \n", w2);
    faucet_host::ScanPassResult res;
    if (int rc = run.shards ? scan_shards(o, *run.shards, short_pf, long_pf, &res, from_kept) : from_kept ? scan_kept_one_device(o, ctx, kept_batches, short_pf, long_pf, clk, &res)
                                                                                               : scan_one_device(o, ctx, short_pf, long_pf, clk, &res)) return rc;
    time(&stop);
    clk.mark(run.shards && from_kept ? "pass 2 (shards, scan of kept reads)" : run.shards ? "pass 2 (shards)" : from_kept ? "pass 2 (scan of kept reads)" : "pass 2 (read + scan)");
    return write_scan_outputs(o, ctx, res.stats, res.empty_count, res.not_empty_count, difftime(stop, start), short_pf, long_pf, clk);
}

}  // namespace

int main(int argc, char** argv) {
    PhaseClock clk;
    Options o;
    KeptReads kept;
    if (handle_arguments(argc, argv, o) == 1) return 1;
    if (o.scan_kept) {      // refused before any input is opened and before anything is printed or written
        const bool slices = o.gpus > 1 && ShardedRun::slices_asked();      // (filter slices: every rank ends pass 1 holding the whole stream)
        if (o.gpus > 1 && !slices) { fprintf(stderr, "--scan_kept needs -gpus 1: read shards and filter slices keep batches of their own\n"); return 2; }
        if (slices && o.batch_reads) {
            fprintf(stderr, "--scan_kept with -gpus %d cannot be combined with -batch_reads: the ranks split their records on their devices (leave -batch_reads out)\n", o.gpus);
            return 2;
        }
        if (o.from_bloom) { fprintf(stderr, "--scan_kept cannot be combined with -bloom_file: without pass 1 no reads are kept (give -read_scan_file and leave --scan_kept out)\n"); return 2; }
        if (slices && !ShardedRun::scan_kept_linked()) {
            fprintf(stderr, "--scan_kept with -gpus %d: the library this program is linked against lacks the entry points of the sliced pass that keeps its reads "
                            "(fgpu_load_slice_keep_reads, fgpu_load_slice_packed_reads, fgpu_load_slice_expect_reads, fgpu_load_slice_adopt_reads, "
                            "fgpu_scan_kept_range, fgpu_scan_batch_kept, fgpu_scan_prepare_kept): run with -gpus 1, or give -read_scan_file and leave --scan_kept out\n", o.gpus);
            return 2;
        }
        if (!faucet_host::scan_kept_linked() || !fgpu_estimate_keep_reads || !fgpu_estimate_take_kept_reads || !fgpu_load_batch_packed_reads) {
            fprintf(stderr, "--scan_kept: the library this program is linked against lacks the entry points of the scan of kept reads "
                            "(fgpu_scan_kept_state, fgpu_scan_batch_kept, fgpu_estimate_keep_reads, fgpu_estimate_take_kept_reads, fgpu_load_batch_packed_reads)\n");
            return 2;
        }
    }
    if (o.raw_contigs) {    // refused before any input is opened and before anything is printed or written
        if (!fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_raw_contigs || !fgpu_stage3_fasta_take) {
            fprintf(stderr, "--raw_contigs: the library this program is linked against lacks the entry points of the graph build and its contigs "
                            "(fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_raw_contigs, fgpu_stage3_fasta_take)\n");
            return 2;
        }
        if (o.just_load || o.from_junctions) { fprintf(stderr, "--raw_contigs needs the junction scan of this run: leave out --just_load_bloom and -junctions_file\n"); return 2; }
    }
    if (o.detipped_contigs) {    // ... likewise
        if (!fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_detip || !fgpu_stage3_fasta_take) {
            fprintf(stderr, "--detipped_contigs: the library this program is linked against lacks the entry points of the graph build and its first cleaning step "
                            "(fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_detip, fgpu_stage3_fasta_take)\n");
            return 2;
        }
        if (o.just_load || o.from_junctions) { fprintf(stderr, "--detipped_contigs needs the junction scan of this run: leave out --just_load_bloom and -junctions_file\n"); return 2; }
    }
    if (o.dechimered_contigs) {  // ... likewise
        if (!fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_detip || !fgpu_stage3_dechimera || !fgpu_stage3_fasta_take) {
            fprintf(stderr, "--dechimered_contigs: the library this program is linked against lacks the entry points of the graph build and its first two cleaning steps "
                            "(fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_detip, fgpu_stage3_dechimera, fgpu_stage3_fasta_take)\n");
            return 2;
        }
        if (o.just_load || o.from_junctions) { fprintf(stderr, "--dechimered_contigs needs the junction scan of this run: leave out --just_load_bloom and -junctions_file\n"); return 2; }
    }
    struct { bool on; const char* flag; bool missing; const char* entries; } graph_flags[] = {   // ... likewise
        {o.raw_graph, "--raw_graph", !fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_raw_graph || !fgpu_stage3_fasta_take,
         "fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_raw_graph, fgpu_stage3_fasta_take"},
        {o.detipped_graph, "--detipped_graph", !fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_detip || !fgpu_stage3_graph_fastg || !fgpu_stage3_fasta_take,
         "fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_detip, fgpu_stage3_graph_fastg, fgpu_stage3_fasta_take"},
        {o.dechimered_graph, "--dechimered_graph",
         !fgpu_stage3_set_junctions || !fgpu_stage3_build || !fgpu_stage3_detip || !fgpu_stage3_dechimera || !fgpu_stage3_graph_fastg || !fgpu_stage3_fasta_take,
         "fgpu_stage3_set_junctions, fgpu_stage3_build, fgpu_stage3_detip, fgpu_stage3_dechimera, fgpu_stage3_graph_fastg, fgpu_stage3_fasta_take"}};
    for (const auto& g : graph_flags) {
        if (!g.on) continue;
        if (g.missing) {
            fprintf(stderr, "%s: the library this program is linked against lacks the entry points of the graph build, its cleaning steps and the graph's FASTG (%s)\n", g.flag, g.entries);
            return 2;
        }
        if (o.just_load || o.from_junctions) { fprintf(stderr, "%s needs the junction scan of this run: leave out --just_load_bloom and -junctions_file\n", g.flag); return 2; }
    }
    if (o.estimate && !(o.est_kmers_flag && o.est_sing_flag)) {     // pass 0, ahead of everything the two numbers decide (and of the lines that print them)
        if (o.k < 1 || o.k > 31) { fprintf(stderr, "k must be in 1..31 on this build\n"); return 1; }
        choose_chunk_bytes(o);
        if (int rc = estimate_missing(o, clk, &kept)) return rc;
    }
    print_settings(o);
    if (o.k < 1 || o.k > 31) { fprintf(stderr, "k must be in 1..31 on this build\n"); return 1; }
    if (int rc = size_filters(o)) return rc;
    const fgpu_params prm = context_params(o);
    choose_chunk_bytes(o);
    const bool sharded = o.gpus > 1 && !o.from_junctions;
    Run run;                    // (declared before the .bloom writer: the file is complete before the contexts go)
    if (int rc = sharded ? open_shards(o, prm, clk.on, &run) : open_one_device(o, prm, &run)) return rc;
    clk.mark(sharded ? "arguments, sizing, contexts" : "arguments, sizing, fgpu_create");
    BloomFile bloom(o.file_prefix, o.tai);
    if (int rc = o.from_bloom ? load_bloom_file(o, run, bloom) : load_from_reads(o, run, clk, bloom, kept)) {
        kept.release(run.first());
        return rc;
    }
    bool from_kept = false;
    uint64_t kept_batches = 0;
    if (o.scan_kept && !o.just_load)
        if (int rc = run.shards ? decide_scan_kept_shards(o, *run.shards, bloom, &from_kept) : decide_scan_kept(o, run.one, bloom, clk, &from_kept, &kept_batches)) return rc;
    PairFilter short_pf, long_pf;
    create_pair_filters(o, &short_pf, &long_pf);
    if (o.just_load) return bloom.complete() ? 0 : 2;
    if (o.from_junctions) {
        if (int rc = reload_scan_files(o, short_pf, long_pf)) return rc;
        return bloom.complete() ? 3 : 2;
    }
    if (int rc = scan_and_write(o, run, short_pf, long_pf, clk, from_kept, kept_batches)) return rc;
    clk.mark("pair filter weights");
    if (!o.no_cleaning)
        fprintf(stderr, "The contig-graph stage is not part of this build: the load and scan outputs have been written; the reference\n"
                        "continues from the same calls through integration/faucet_binding.cpp (INTEGRATION.md).\n");
    if (!bloom.complete()) return 2;                  // (_exit below skips destructors)
    const int code = o.no_cleaning ? 0 : 3;
    // Every output file is closed and both passes have ended with a synchronised device.  Returning several hundred HBM buffers one by
    // one, unpinning the text buffers and unloading the HIP runtime took 0.15 s of a 0.9 s run and changes nothing the caller can see:
    // the driver releases what the process held.  FGPU_CLI_TIDY=1 takes the long way (profilers that write their output at exit need it).
    if (!getenv("FGPU_CLI_TIDY")) {
        fflush(stdout);
        fflush(stderr);
        _exit(code);
    }
    run.close();
    clk.mark("fgpu_destroy");
    return code;
}
