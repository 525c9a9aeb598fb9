// batch_board_check.cpp — faucet_amd/host/batch_board.h alone, the way the sliced pass 1 of shard_host.h uses it: every rank's thread first
// publishes the batches of its own shard, then walks the board in file order.  Built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_slices_host_cpu.py and run directly; exit status 0 and "ok" iff every consumer saw the same
// file-order list and the abort case woke every waiter.
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <thread>
#include <vector>

#include "batch_board.h"

using faucet_host::BatchBoard;
using faucet_host::BoardBatch;

namespace {

struct Seen {
    int shard;
    uint64_t index, T, n_reads;
    bool operator==(const Seen& o) const { return shard == o.shard && index == o.index && T == o.T && n_reads == o.n_reads; }
};

uint64_t stream_positions(int shard, uint64_t j) { return (uint64_t)(shard + 1) * 1000003ULL + j * 7919ULL + (j % 5 == 0 ? 0 : 1); }

// publisher and consumer in one thread per rank, as in ShardedRun::slice_rank; `pause_every`: the publisher yields now and then, so that
// consumers of other ranks meet shards in every state -- empty, growing, closed
int run(const std::vector<uint64_t>& per_shard, int pause_every) {
    const int n = (int)per_shard.size();
    BatchBoard board(n);
    std::vector<std::vector<Seen>> seen((size_t)n);
    std::vector<int> failed((size_t)n, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < n; r++)
        th.emplace_back([&, r] {
            for (uint64_t j = 0; j < per_shard[(size_t)r]; j++) {
                BoardBatch b;
                b.T = stream_positions(r, j);
                b.n_reads = j % 5 == 0 ? 0 : j + 1;
                if (j % 5 == 0) b.T = 0;                       // an empty batch: posted all the same, it keeps its place in the list
                if (!board.post(r, b)) failed[(size_t)r] = 1;
                if (pause_every && j % (uint64_t)pause_every == 0) std::this_thread::yield();
            }
            board.close(r);
            if (board.post(r, BoardBatch())) failed[(size_t)r] = 1;      // nothing is posted to a closed shard
            for (int s = 0; s < n; s++)
                for (uint64_t j = 0;; j++) {
                    BoardBatch b;
                    const BatchBoard::Wait w = board.wait(s, j, &b);
                    if (w == BatchBoard::ABORTED) { failed[(size_t)r] = 1; return; }
                    if (w == BatchBoard::CLOSED) break;
                    seen[(size_t)r].push_back(Seen{s, j, b.T, b.n_reads});
                }
        });
    for (std::thread& t : th) t.join();
    std::vector<Seen> want;
    for (int s = 0; s < n; s++)
        for (uint64_t j = 0; j < per_shard[(size_t)s]; j++)
            want.push_back(Seen{s, j, j % 5 == 0 ? 0 : stream_positions(s, j), j % 5 == 0 ? 0 : j + 1});
    for (int r = 0; r < n; r++) {
        if (failed[(size_t)r]) { fprintf(stderr, "rank %d: a post or a wait failed\n", r); return 1; }
        if (!(seen[(size_t)r] == want)) { fprintf(stderr, "rank %d saw %zu batches, not the file-order list of %zu\n", r, seen[(size_t)r].size(), want.size()); return 1; }
        if (board.count(r) != per_shard[(size_t)r]) { fprintf(stderr, "count of shard %d\n", r); return 1; }
    }
    return 0;
}

// three consumers wait for a batch of shard 1 that never comes; its owner aborts instead: all wake with ABORTED, batches posted before
// the abort are not handed out any more, nothing can be posted afterwards
int run_abort() {
    BatchBoard board(4);
    BoardBatch one;
    one.T = 64;
    one.n_reads = 1;
    if (!board.post(0, one)) return 1;
    board.close(0);
    if (board.count(0) != 1 || board.count(1) != ~0ULL) return 1;
    std::atomic<int> arrived{0}, aborted{0}, wrong{0};
    std::vector<std::thread> th;
    for (int r = 0; r < 3; r++)
        th.emplace_back([&] {
            BoardBatch b;
            if (board.wait(0, 0, &b) != BatchBoard::BATCH || b.T != 64) wrong++;
            if (board.wait(0, 1, &b) != BatchBoard::CLOSED) wrong++;
            arrived++;
            if (board.wait(1, 0, &b) == BatchBoard::ABORTED) aborted++; else wrong++;
        });
    while (arrived.load() < 3) std::this_thread::yield();
    board.abort();
    for (std::thread& t : th) t.join();
    BoardBatch b;
    if (board.wait(0, 0, &b) != BatchBoard::ABORTED || board.post(2, one)) wrong++;
    if (aborted.load() != 3 || wrong.load() != 0) { fprintf(stderr, "abort: %d of 3 waiters woke aborted, %d wrong answers\n", aborted.load(), wrong.load()); return 1; }
    return 0;
}

}  // namespace

int main() {
    // uneven shards, one of them empty, a few hundred batches in all; once as fast as the threads go, once with the publishers yielding
    const std::vector<uint64_t> shards = {150, 0, 37, 260};
    for (int pause_every : {0, 3})
        if (int rc = run(shards, pause_every)) return rc;
    if (int rc = run({0, 0, 0, 0}, 0)) return rc;              // nobody has anything
    if (int rc = run({1}, 0)) return rc;                       // one rank
    if (int rc = run_abort()) return rc;
    printf("ok\n");
    return 0;
}
