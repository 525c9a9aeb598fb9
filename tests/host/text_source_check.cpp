// text_source_check.cpp — faucet_amd/host/text_source.h alone, linked with the tests' CPU stand-in of the C ABI (tests/stub/faucet_gpu_stub.cpp):
// TextSource (the chunked feed with its reader thread and the tail it carries from chunk to chunk, over a whole file and over the byte
// ranges of read shards), record_cuts and ReadSource on one input file.  It judges nothing itself: it prints the reads every feed hands
// out and the cuts, and tests/test_input_side_cpu.py compares them with the restatement of the reference's reading loop
// (tests/getline_ref.py).  Built plain, with -fsanitize=address,undefined and with -fsanitize=thread, and run directly.
//
//   text_source_check <file> <fastq: 0 | 1>
//
// Output, one item per line (reads in hex, "-" for an empty one):
//   cuts <group> <n> <n + 1 offsets>
//   source <chunk> <begin> <end>          a TextSource over [begin, end) ("all" "all": the whole file), then its reads, then
//   batches <batches handed out> <bytes handed out>
//   getline <batch size>                  a ReadSource, then its reads, then
//   batches <batches handed out> 0
//   read <hex>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "text_source.h"

using faucet_host::ReadSource;
using faucet_host::TextSource;
using faucet_host::kTextPad;
using faucet_host::record_cuts;

namespace {

void print_reads(const fgpu_reads& r) {
    for (uint64_t i = 0; i < r.n_reads; i++) {
        const uint64_t len = r.offsets[i + 1] - r.offsets[i];
        const char* p = r.bases + (r.starts ? r.starts[i] : r.offsets[i]);
        fputs("read ", stdout);
        if (!len) fputs("-", stdout);
        for (uint64_t b = 0; b < len; b++) printf("%02x", (unsigned)(unsigned char)p[b]);
        fputs("\n", stdout);
    }
}

// false: a call failed
bool feed(fgpu_ctx* ctx, const std::string& path, bool fastq, uint64_t chunk, bool whole, uint64_t begin, uint64_t end, char* const* bufs) {
    if (whole) printf("source %llu all all\n", (unsigned long long)chunk);
    else printf("source %llu %llu %llu\n", (unsigned long long)chunk, (unsigned long long)begin, (unsigned long long)end);
    TextSource src(path, fastq, chunk, whole ? 0 : begin, whole ? ~0ULL : end, bufs);
    if (!src.is_open()) return false;
    uint64_t batches = 0;
    for (;;) {
        fgpu_reads r;
        const int rc = src.next(ctx, &r);
        if (rc < 0) { fprintf(stderr, "TextSource::next: %d\n", rc); return false; }
        if (rc == 0) break;
        batches++;
        print_reads(r);
    }
    printf("batches %llu %llu\n", (unsigned long long)batches, (unsigned long long)src.bytes_handed_out());
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: text_source_check <file> <fastq: 0 | 1>\n"); return 2; }
    const std::string path = argv[1];
    const bool fastq = atoi(argv[2]) != 0;
    fgpu_params prm = fgpu_params();
    prm.k = 21;
    prm.j = 1;
    prm.max_spacer_dist = 100;
    prm.n_hash = 2;
    prm.tai = 1 << 12;
    fgpu_ctx* ctx = nullptr;
    if (fgpu_create(&prm, &ctx) != FGPU_OK) { fprintf(stderr, "fgpu_create failed\n"); return 1; }
    const uint64_t chunks[] = {1, 2, 3, 7, 23, 64, 4096};
    char* bufs[2];
    for (int i = 0; i < 2; i++) {
        bufs[i] = (char*)malloc(kTextPad + 4096);  // caller-owned: kTextPad + the largest chunk (not cleared: only what a chunk wrote may be read)
        if (!bufs[i]) return 1;
    }
    bool ok = true;
    for (uint64_t chunk : chunks) ok = ok && feed(ctx, path, fastq, chunk, true, 0, 0, bufs);
    for (int group = 1; group <= 2 && ok; group++)
        for (int n = 1; n <= 9 && ok; n++) {
            std::vector<uint64_t> cuts;
            if (!record_cuts(path, fastq ? 4 : 2, group, n, &cuts) || cuts.size() != (size_t)n + 1) { fprintf(stderr, "record_cuts failed\n"); ok = false; break; }
            printf("cuts %d %d", group, n);
            for (uint64_t c : cuts) printf(" %llu", (unsigned long long)c);
            printf("\n");
            for (uint64_t chunk : {(uint64_t)7, (uint64_t)4096})
                for (int r = 0; r < n && ok; r++) ok = feed(ctx, path, fastq, chunk, false, cuts[(size_t)r], cuts[(size_t)r + 1], bufs);
        }
    for (uint64_t batch : {(uint64_t)1, (uint64_t)3, (uint64_t)1000}) {
        if (!ok) break;
        printf("getline %llu\n", (unsigned long long)batch);
        ReadSource src(path, fastq);
        if (!src.is_open()) { ok = false; break; }
        uint64_t batches = 0;
        fgpu_reads r;
        while (src.next(batch, &r)) {
            batches++;
            print_reads(r);
        }
        printf("batches %llu 0\n", (unsigned long long)batches);
    }
    fgpu_destroy(ctx);
    for (int i = 0; i < 2; i++) free(bufs[i]);
    if (!ok) return 1;
    printf("ok\n");
    return 0;
}
