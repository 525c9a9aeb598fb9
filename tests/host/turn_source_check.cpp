// turn_source_check.cpp — the turn-taking reader (faucet_amd/host/text_source.h, TurnSource) and the board walked in the stream's order
// (batch_board.h, StreamCursor) the way the sliced pass 1 of shard_host.h uses them on a pipe: N threads, one context each of the tests' CPU
// stand-in of the C ABI (tests/stub/faucet_gpu_stub.cpp), ONE TextSource.  Every thread first takes its turns -- chunk g is read and split
// by thread g mod N and posted as its batch g / N --, then walks the board.  It judges the threads against each other and prints the reads
// in the order the first thread consumed them; tests/test_multi_scan_kept_cpu.py compares those with the restatement of the reference's
// reading loop (tests/getline_ref.py).  Built plain, with -fsanitize=thread and with -fsanitize=address,undefined, and run directly.
//
//   turn_source_check <input: a file or a FIFO> <fastq: 0 | 1> <threads> <chunk bytes> [<g>: the thread that is handed chunk g aborts instead]
//
// Output: "read <hex>" per read ("-" for an empty one), "batches <n>", then "ok"; with an abort: "aborted <threads that were told>" and "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "batch_board.h"
#include "text_source.h"

using namespace faucet_host;

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const std::string path = argv[1];
    const bool fastq = atoi(argv[2]) != 0;
    const int n = atoi(argv[3]);
    const uint64_t chunk = strtoull(argv[4], nullptr, 10);
    const long long abort_at = argc > 5 ? atoll(argv[5]) : -1;
    fgpu_params prm;
    memset(&prm, 0, sizeof(prm));
    prm.k = 21; prm.j = 1; prm.max_spacer_dist = 100; prm.n_hash = 1; prm.tai = 128;
    std::vector<fgpu_ctx*> ctx((size_t)n, nullptr);
    for (int r = 0; r < n; r++)
        if (fgpu_create(&prm, &ctx[(size_t)r]) != FGPU_OK) { fprintf(stderr, "fgpu_create failed\n"); return 2; }
    char* bufs[2] = {(char*)malloc(kTextPad + chunk), (char*)malloc(kTextPad + chunk)};
    int status = 0;
    {
        TextSource src(path, fastq, chunk, 0, ~0ULL, bufs);
        if (!src.is_open()) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 2; }
        TurnSource turns(&src, n);
        BatchBoard board(n);
        std::mutex store_m;
        std::map<uint64_t, std::vector<std::string>> store;      // chunk g -> its reads, put there before the batch is posted
        std::vector<std::vector<std::string>> seen((size_t)n);
        std::vector<int> told((size_t)n, 0), failed((size_t)n, 0);
        std::vector<std::thread> th;
        for (int r = 0; r < n; r++)
            th.emplace_back([&, r] {
                fgpu_reads b;
                uint64_t g = 0, mine = 0;
                for (int more; (more = turns.next(r, ctx[(size_t)r], &b, &g)) != 0;) {
                    if (more == TurnSource::ABORTED) { told[(size_t)r] = 1; break; }
                    if (more < 0) { failed[(size_t)r] = 1; board.abort(); turns.abort(); return; }
                    if (g % (uint64_t)n != (uint64_t)r || g / (uint64_t)n != mine) { failed[(size_t)r] = 1; board.abort(); turns.abort(); return; }
                    if ((long long)g == abort_at) { board.abort(); turns.abort(); told[(size_t)r] = 1; break; }
                    std::vector<std::string> reads;
                    uint64_t bases = 0;
                    for (uint64_t i = 0; i < b.n_reads; i++) {
                        const uint64_t len = b.offsets[i + 1] - b.offsets[i];
                        reads.push_back(std::string(b.bases + (b.starts ? b.starts[i] : b.offsets[i]), (size_t)len));
                        bases += len;
                    }
                    {
                        std::lock_guard<std::mutex> lk(store_m);
                        store[g].swap(reads);
                    }
                    BoardBatch bb;
                    bb.T = bases + b.n_reads;
                    bb.n_reads = b.n_reads;
                    if (!board.post(r, bb)) { told[(size_t)r] = 1; break; }
                    mine++;
                }
                board.close(r);
                StreamCursor cursor(&board, true);
                for (;;) {
                    BoardBatch bb;
                    int owner = 0;
                    uint64_t j = 0;
                    const BatchBoard::Wait w = cursor.next(&owner, &j, &bb);
                    if (w == BatchBoard::ABORTED) { told[(size_t)r] = 1; return; }
                    if (w == BatchBoard::CLOSED) break;
                    std::lock_guard<std::mutex> lk(store_m);
                    const std::vector<std::string>& reads = store[j * (uint64_t)n + (uint64_t)owner];
                    uint64_t T = 0;
                    for (const std::string& s : reads) { seen[(size_t)r].push_back(s); T += s.size() + 1; }
                    if (T != bb.T || reads.size() != bb.n_reads) failed[(size_t)r] = 1;
                }
            });
        for (std::thread& t : th) t.join();
        for (int r = 0; r < n; r++) {
            if (failed[(size_t)r]) { fprintf(stderr, "thread %d failed\n", r); status = 1; }
            if (abort_at < 0 && (told[(size_t)r] || seen[(size_t)r] != seen[0])) { fprintf(stderr, "thread %d saw another stream\n", r); status = 1; }
        }
        if (abort_at >= 0) {
            int all = 0;
            for (int t : told) all += t;
            printf("aborted %d\n", all);
        } else {
            for (const std::string& s : seen[0]) {
                fputs("read ", stdout);
                if (s.empty()) fputs("-", stdout);
                for (unsigned char c : s) printf("%02x", (unsigned)c);
                fputs("\n", stdout);
            }
            printf("batches %llu\n", (unsigned long long)store.size());
        }
    }
    for (fgpu_ctx* c : ctx) fgpu_destroy(c);
    free(bufs[0]);
    free(bufs[1]);
    if (status == 0) printf("ok\n");
    return status;
}
