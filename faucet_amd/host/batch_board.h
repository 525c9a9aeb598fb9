// batch_board.h — who has packed which batch: the host-side board of the sliced pass 1 (shard_host.h, FAUCET_SHARD_PROTOCOL=slices).
//
// Under filter slices every rank loads every batch of the stream, in file order, but each batch is read, split and packed by one rank only:
// the owner of its read shard.  The owner POSTS the batch's description here -- (shard, index within the shard, stream positions, reads) --
// and sends the packed bytes device to device; every rank walks the board in file order (shard 0's batches, then shard 1's, ...) and so
// learns what to expect from whom, and how many batches a shard has once its owner has CLOSED it.  Every rank therefore sees the same list,
// which is what lets them make the same sequence of collective calls.
//
// The stream's batches come onto the board in one of two ways, and StreamCursor walks either in the stream's order:
//   by shards  (a regular file)  rank r posts the batches of its own file-order share; global order = shard 0's batches, shard 1's, ...
//   by turns   (a pipe)          the ranks take turns at ONE reader: chunk g is posted by rank g mod N as its batch g / N; global order = g
// "Global batch g is (owner, j) on the board" is all the consumers need to know.
//
// Nothing here knows about devices: the standard library only, so it can be tested alone (tests/host/batch_board_check.cpp).
#pragma once
#include <stdint.h>

#include <condition_variable>
#include <mutex>
#include <vector>

namespace faucet_host {

struct BoardBatch {
    uint64_t T = 0;         // stream positions of the packed batch (0: no reads, no block)
    uint64_t n_reads = 0;
};

class BatchBoard {
public:
    explicit BatchBoard(int n_shards) : shards_((size_t)(n_shards > 0 ? n_shards : 0)) {}
    BatchBoard(const BatchBoard&) = delete;
    BatchBoard& operator=(const BatchBoard&) = delete;

    int n_shards() const { return (int)shards_.size(); }

    // the owner of `shard`: its next batch (index = the number of batches it has posted before).  False after close(shard) or abort().
    bool post(int shard, const BoardBatch& b) {
        {
            std::lock_guard<std::mutex> g(m_);
            Shard& s = shards_[(size_t)shard];
            if (s.closed || aborted_) return false;
            s.batches.push_back(b);
        }
        cv_.notify_all();
        return true;
    }
    // the owner of `shard`: no more batches
    void close(int shard) {
        {
            std::lock_guard<std::mutex> g(m_);
            shards_[(size_t)shard].closed = true;
        }
        cv_.notify_all();
    }
    // wakes every waiter; all further waits answer ABORTED
    void abort() {
        {
            std::lock_guard<std::mutex> g(m_);
            aborted_ = true;
        }
        cv_.notify_all();
    }

    enum Wait { BATCH = 0, CLOSED = 1, ABORTED = 2 };
    // Blocks until batch `index` of `shard` is posted (BATCH, *out filled), the shard is closed with no more than `index` batches (CLOSED),
    // or the board is aborted (which wins over both: an aborted run hands out nothing more).
    Wait wait(int shard, uint64_t index, BoardBatch* out) {
        std::unique_lock<std::mutex> g(m_);
        Shard& s = shards_[(size_t)shard];
        cv_.wait(g, [&] { return aborted_ || s.batches.size() > index || s.closed; });
        if (aborted_) return ABORTED;
        if (s.batches.size() > index) {
            if (out) *out = s.batches[(size_t)index];
            return BATCH;
        }
        return CLOSED;
    }
    // batches of a closed shard (what pass 2 needs to find its own batches among the resident ones); ~0 while the shard is open
    uint64_t count(int shard) {
        std::lock_guard<std::mutex> g(m_);
        const Shard& s = shards_[(size_t)shard];
        return s.closed ? (uint64_t)s.batches.size() : ~0ULL;
    }

private:
    struct Shard {
        std::vector<BoardBatch> batches;
        bool closed = false;
    };
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<Shard> shards_;
    bool aborted_ = false;
};

// The board's batches in the order of the stream, one consumer's view (every consumer has a cursor of its own)
class StreamCursor {
public:
    StreamCursor(BatchBoard* board, bool by_turns) : board_(board), by_turns_(by_turns) {}
    // Blocks like BatchBoard::wait.  BATCH: the stream's next batch is batch *j of *owner; CLOSED: the stream has ended; ABORTED.
    BatchBoard::Wait next(int* owner, uint64_t* j, BoardBatch* out) {
        const int n = board_->n_shards();
        if (n <= 0) return BatchBoard::CLOSED;
        if (by_turns_) {      // chunk g belongs to rank g mod n: the first turn that finds its owner closed is the end of the stream
            *owner = (int)(g_ % (uint64_t)n);
            *j = g_ / (uint64_t)n;
            const BatchBoard::Wait w = board_->wait(*owner, *j, out);
            if (w == BatchBoard::BATCH) g_++;
            return w;
        }
        while (shard_ < n) {
            const BatchBoard::Wait w = board_->wait(shard_, j_, out);
            if (w == BatchBoard::CLOSED) { shard_++; j_ = 0; continue; }
            if (w == BatchBoard::BATCH) { *owner = shard_; *j = j_++; g_++; }
            return w;
        }
        return BatchBoard::CLOSED;
    }
    uint64_t taken() const { return g_; }      // batches handed out so far = the global number of the next one

private:
    BatchBoard* board_;
    bool by_turns_;
    uint64_t g_ = 0, j_ = 0;
    int shard_ = 0;
};

}  // namespace faucet_host
