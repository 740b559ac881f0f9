// sim_exchange_test.cpp -- CPU check of what a simulation's rank threads share through host memory
// (fixedpointldpc_amd/csrc/fpldpc_sim_exchange.hpp) and of the weighted sums' frame step (bias_sums_add,
// fpldpc_bias.hpp).  tests/test_sim_exchange.py builds it plain, with the address and undefined-behaviour sanitizers
// and with the thread sanitizer.
//
// Barrier: 2, 3 and 8 threads through 3000 generations; a thread counts itself in before each wait and, once
// released, must find every thread counted in.  abort() while others wait or are about to: every wait returns
// false, and so does every later one.  abort() by a thread just released from a completed generation, 2000 times
// with 2 and with 3 threads: the other threads of that generation still return true, slow to wake or not, and
// their next wait returns false.
// HostExchange: 1, 2, 3 and 8 ranks, 300 alternating allgather / allreduce calls of 5 words: every rank receives
// every rank's words in rank order, and the exact sums.  Failure: a rank calls abort() in place of its call k --
// every other rank's calls before k succeed and its call k fails -- or right after its call k returned: then call k
// succeeds everywhere and call k + 1 fails.  No thread may block: one that has not ended after 120 s ends the
// program with exit code 2.
// bias_sums_add: 300 runs of 1 to 400 random (logw, blk) pairs, blk = 0 in about half the frames, against the sums
// written out from include/fpldpc.h's definition: integers equal, doubles bit for bit.
// Exit 0 = all trials agree.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <random>
#include <thread>
#include <vector>

#include "fpldpc_bias.hpp"
#include "fpldpc_sim_exchange.hpp"

using fpldpc::Barrier;
using fpldpc::HostExchange;

namespace {

// fn(t) on n threads; the sum of what they return.  A thread that does not end is a deadlock: exit 2.
int run_threads(int n, const std::function<int(int)> &fn) {
    std::vector<std::future<int>> done;
    std::vector<std::thread> th;
    for (int t = 0; t < n; ++t) {
        std::packaged_task<int(int)> task(fn);
        done.push_back(task.get_future());
        th.emplace_back(std::move(task), t);
    }
    int bad = 0;
    for (auto &d : done) {
        if (d.wait_for(std::chrono::seconds(120)) != std::future_status::ready) {
            printf("sim_exchange_test: a thread is still blocked after 120 s\n");
            fflush(stdout);
            std::_Exit(2);
        }
        bad += d.get();
    }
    for (auto &x : th) x.join();
    return bad;
}

int barrier_generations(int n) {
    const int G = 3000;
    Barrier bar(n);
    std::vector<std::atomic<int>> in(G);
    for (auto &x : in) x = 0;
    return run_threads(n, [&](int) {
        int bad = 0;
        for (int g = 0; g < G; ++g) {
            ++in[g];
            bad += !bar.wait();
            bad += in[g].load() != n;
        }
        return bad;
    });
}

int barrier_abort_while_waiting(int n) {
    Barrier bar(n + 1);  // one thread never comes
    std::atomic<int> near{0};
    std::thread aborter([&] {
        while (near.load() != n) std::this_thread::yield();
        for (int i = 0; i < 100; ++i) std::this_thread::yield();  // most are inside wait() by now; either way is tested
        bar.abort();
    });
    const int bad = run_threads(n, [&](int) {
        ++near;
        int b = bar.wait();  // must be false
        for (int i = 0; i < 3; ++i) b += bar.wait();
        return b;
    });
    aborter.join();
    return bad + bar.wait();
}

int barrier_abort_after_completion(int n) {
    int bad = 0;
    for (int trial = 0; trial < 2000; ++trial) {
        Barrier bar(n);
        bad += run_threads(n, [&](int t) {
            int b = !bar.wait();      // the generation completes: true for all, whoever wakes last
            if (t == 0) bar.abort();  // at once, while the others may not have woken yet
            if (t != 0) {
                // their next wait cannot complete (thread 0 never comes): false, now or once the abort lands
                b += bar.wait();
            }
            return b;
        });
        bad += bar.wait();
    }
    return bad;
}

constexpr int kWords = 5;
int64_t word(int rank, int call, int w) { return (int64_t)(rank + 1) * 1000003 + (int64_t)call * 8191 + w * 17 - 40000; }

// One rank's `calls` alternating calls; the index of its first failing call, or `calls`; *bad counts wrong contents.
int exchange_calls(HostExchange &ex, int ranks, int rank, int calls, int *bad) {
    std::vector<int64_t> all((size_t)ranks * kWords);
    int64_t mine[kWords], sum[kWords];
    for (int c = 0; c < calls; ++c) {
        for (int w = 0; w < kWords; ++w) mine[w] = word(rank, c, w);
        if (c & 1) {
            if (!ex.allreduce(rank, mine, sum)) return c;
            for (int w = 0; w < kWords; ++w) {
                int64_t want = 0;
                for (int i = 0; i < ranks; ++i) want += word(i, c, w);
                *bad += sum[w] != want;
            }
        } else {
            if (!ex.allgather(rank, mine, all.data())) return c;
            for (int i = 0; i < ranks; ++i)
                for (int w = 0; w < kWords; ++w) *bad += all[(size_t)i * kWords + w] != word(i, c, w);
        }
    }
    return calls;
}

int exchange_all(int ranks) {
    HostExchange ex(ranks, kWords);
    return run_threads(ranks, [&](int r) {
        int bad = 0;
        const int first = exchange_calls(ex, ranks, r, 300, &bad);
        return bad + (first != 300);
    });
}

// Rank `failing` aborts in place of its call k (after = false) or right after its call k (after = true)
int exchange_failure(int ranks, int failing, int k, bool after) {
    HostExchange ex(ranks, kWords);
    return run_threads(ranks, [&](int r) {
        int bad = 0;
        if (r == failing) {
            const int own = after ? k + 1 : k;
            const int first = exchange_calls(ex, ranks, r, own, &bad);
            ex.abort();
            return bad + (first != own);
        }
        const int first = exchange_calls(ex, ranks, r, k + 6, &bad);
        bad += first != (after ? k + 1 : k);
        int64_t mine[kWords] = {0}, out[8 * kWords];
        bad += ex.allgather(r, mine, out) || ex.allreduce(r, mine, out);  // and every later call fails at once
        return bad;
    });
}

int bias_sums(std::mt19937_64 &rng, int frames) {
    std::vector<double> lw(frames);
    std::vector<int64_t> blk(frames);
    std::normal_distribution<double> nd(-3.0, 4.0);
    for (int f = 0; f < frames; ++f) {
        lw[f] = nd(rng);
        blk[f] = rng() % 2 ? 0 : (int64_t)(rng() % 2000);
    }
    fpldpc_bias_sums got = fpldpc::bias_sums_start();
    for (int f = 0; f < frames; ++f) fpldpc::bias_sums_add(got, lw[f], blk[f]);
    // include/fpldpc.h: added in frame order with w = exp(logw[f]), fe = (blk > 0)
    fpldpc_bias_sums want{};
    want.min_logw = INFINITY;
    want.max_logw = -INFINITY;
    for (int f = 0; f < frames; ++f) {
        const double w = exp(lw[f]), fe = blk[f] > 0 ? 1.0 : 0.0;
        want.frames += 1;
        want.frame_errors += blk[f] > 0 ? 1 : 0;
        want.bit_errors += blk[f];
        want.sum_w = want.sum_w + w;
        want.sum_w2 = want.sum_w2 + w * w;
        want.sum_w_fe = want.sum_w_fe + w * fe;
        want.sum_w2_fe = want.sum_w2_fe + w * w * fe;
        want.sum_w_be = want.sum_w_be + w * (double)blk[f];
        if (lw[f] < want.min_logw) want.min_logw = lw[f];
        if (lw[f] > want.max_logw) want.max_logw = lw[f];
    }
    int bad = got.frames != want.frames || got.frame_errors != want.frame_errors || got.bit_errors != want.bit_errors;
    const double g[7] = {got.sum_w, got.sum_w2, got.sum_w_fe, got.sum_w2_fe, got.sum_w_be, got.min_logw, got.max_logw};
    const double w[7] = {want.sum_w, want.sum_w2, want.sum_w_fe, want.sum_w2_fe, want.sum_w_be, want.min_logw, want.max_logw};
    return bad + (memcmp(g, w, sizeof(g)) != 0);
}

}  // namespace

int main() {
    int bad = 0, trials = 0;
    auto tally = [&](const char *what, int b) {
        ++trials;
        if (b) printf("  %s: %d mismatches\n", what, b);
        bad += b;
    };
    for (int n : {2, 3, 8}) tally("barrier generations", barrier_generations(n));
    for (int n : {1, 2, 7}) tally("barrier abort while waiting", barrier_abort_while_waiting(n));
    for (int n : {2, 3}) tally("barrier abort after completion", barrier_abort_after_completion(n));
    for (int n : {1, 2, 3, 8}) tally("exchange", exchange_all(n));
    for (int n : {2, 3, 8})
        for (int k : {0, 1, 6, 7})
            for (int after = 0; after < 2; ++after) tally("exchange failure", exchange_failure(n, (k + after) % n, k, after != 0));
    std::mt19937_64 rng(20240611);
    tally("bias sums, one frame", bias_sums(rng, 1));
    for (int t = 0; t < 300; ++t) tally("bias sums", bias_sums(rng, 1 + (int)(rng() % 400)));
    printf("sim_exchange_test: %d trials, %d mismatches\n", trials, bad);
    return bad ? 1 : 0;
}
