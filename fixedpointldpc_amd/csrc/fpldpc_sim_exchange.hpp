// fpldpc_sim_exchange.hpp -- what a simulation's rank threads exchange through host memory (fpldpc_sim.cpp): a
// reusable barrier that a failed rank can break, and on it the all-gather and all-reduce of the ranks' counters.
// Decoders sharing a device exchange this way, and so does an FPLDPC_COLL_AUTO run whose RCCL start failed; the
// RCCL transport (fpldpc_sim.cpp) keeps one for the frame-order barrier.  No HIP, no RCCL: tests/cpp/sim_exchange_test.cpp
// runs it under the address and thread sanitizers.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

namespace fpldpc {

// Host barrier for the rank threads (generation count, reusable).  abort() releases every waiter
// for good: wait() then returns false, so a failed rank cannot leave the others blocked.
class Barrier {
  public:
    explicit Barrier(int n) : n_(n) {}
    bool wait() {
        std::unique_lock<std::mutex> l(m_);
        if (aborted_) return false;
        const uint64_t g = gen_;
        if (++count_ == n_) {
            count_ = 0;
            ++gen_;
            cv_.notify_all();
        } else {
            cv_.wait(l, [&] { return gen_ != g || aborted_; });
            return gen_ != g;  // completed, even if a rank that left it first has aborted since
        }
        return true;
    }
    void abort() {
        std::lock_guard<std::mutex> l(m_);
        aborted_ = true;
        cv_.notify_all();
    }

  private:
    std::mutex m_;
    std::condition_variable cv_;
    int n_, count_ = 0;
    uint64_t gen_ = 0;
    bool aborted_ = false;
};

// The exchange of `words` int64 per rank through host memory.  Every rank makes the same sequence of calls, each
// from its own thread; a call returns false once any rank has called abort() ("another rank of the simulation
// failed", says the caller).  Double-buffered slots, indexed by call parity: a barrier separates the calls, so a
// rank that is already writing call k + 1 does not touch what a slower rank still reads of call k.
class HostExchange {
  public:
    HostExchange(int ranks, int words)
        : bar(ranks), n_(ranks), w_(words), slots_(2 * (size_t)ranks * words), calls_(ranks, 0) {}
    Barrier bar;  // also the frame-order barrier of rank_loop
    void abort() {
        aborted_ = true;
        bar.abort();
    }
    bool aborted() const { return aborted_; }
    // all[ranks][words] = every rank's `mine`, in rank order
    bool allgather(int rank, const int64_t *mine, int64_t *all) {
        if (aborted_) return false;
        int64_t *buf = &slots_[(size_t)(calls_[rank]++ & 1) * n_ * w_];
        memcpy(buf + (size_t)rank * w_, mine, sizeof(int64_t) * w_);
        if (!bar.wait()) return false;
        memcpy(all, buf, sizeof(int64_t) * w_ * n_);
        return true;
    }
    // sum over ranks of `mine` (words): the gather plus a sum
    bool allreduce(int rank, const int64_t *mine, int64_t *sum) {
        std::vector<int64_t> all((size_t)n_ * w_);
        if (!allgather(rank, mine, all.data())) return false;
        for (int w = 0; w < w_; ++w) {
            sum[w] = 0;
            for (int i = 0; i < n_; ++i) sum[w] += all[(size_t)i * w_ + w];
        }
        return true;
    }

  private:
    int n_, w_;
    std::atomic<bool> aborted_{false};
    std::vector<int64_t> slots_;
    std::vector<int> calls_;
};

}  // namespace fpldpc
