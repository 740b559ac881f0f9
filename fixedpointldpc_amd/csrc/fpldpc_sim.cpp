// fpldpc_sim.cpp -- ordered BER/FER simulation around one or several GPU decoders
// (fpldpc_ber_sim, fpldpc_ber_sim_multi, and the same pair for the layered and the flooding min-sum decoder).
//
// The reference harness decodes one frame at a time and stops at the frame whose decode brings the frame-error count to
// 100 (PerfTest.cpp:97-135, 275-311, 385-426, 485-511, 574-600).  Here frames are decoded in chunks by ranks (one decoder,
// one device, one host thread each: fpldpc_sim_rank.hpp).  Rounds, ranges and the stop rule are fpldpc_sim_plan.hpp's:
// per round the ranks exchange their chunk sums (an all-gather), the rank holding the stop frame scans its chunk for it,
// and one all-reduce adds the contributions -- so every counter equals the serial loop's for any number of ranks.  With
// decoders on distinct devices the exchange is RCCL (ncclCommInitAll in this process, collectives on each decoder's
// stream, over xGMI on an MI355X node); decoders sharing a device exchange through host memory
// (fpldpc_sim_exchange.hpp).  Frames of the last round past the stop frame are decoded but not counted.
//
// Two chunks in flight per rank leave the counters unchanged: chunks are still counted in round order, and a chunk
// decoded past the stop frame is drained, not counted.  FPLDPC_SIM_OVERLAP=0 submits each chunk after the previous
// round's exchange, on one decoder.
//
// Frame order (frame_order): for on_frame, a harvest (the *_ber_sim_harvest entry points) and a bias (the
// *_ber_sim_biased entry points), after the stop decision rank 0's thread walks the ranks' chunks in frame order.  It
// appends them to the harvest up to the stop frame, where on_frame is called, and adds the weighted sums
// (include/fpldpc.h, fpldpc_bias_sums) up to and including the stop frame: they depend on neither the chunk size nor
// the number of ranks.  The *_ber_sim_source and float entry points run the same loop; every entry point without a
// source passes the Lehmer stream.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "fpldpc_sim_exchange.hpp"
#include "fpldpc_sim_rank.hpp"
#include "fpldpc_testing.h"

using namespace fpldpc;

namespace {

constexpr int kWords = 5;  // exchanged per rank: 4 counters + a status / frames-decoded word

int other_rank_failed() { return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed"); }

// The exchange between ranks.  Every rank makes the same sequence of calls.  A rank that fails
// anywhere calls abort(): host-mode waiters leave the barrier, and RCCL-mode ranks, which wait for
// their collectives by polling their own stream, abort their own communicator (from their own
// thread, so no communicator is freed under another thread) and return an error.
struct Exchange {
    int ndev = 1;
    HostExchange host;  // the host mode, and the frame-order barrier of both
    // RCCL mode
    std::vector<ncclComm_t> comms;
    std::vector<int64_t *> dbuf;  // per rank: [kWords] send + [ndev * kWords] receive
    bool rccl = false;
    Exchange(int n, bool use_rccl) : ndev(n), host(n, kWords), rccl(use_rccl) {}
    ~Exchange() { release(); }
    void release() {
        for (auto *p : dbuf) (void)hipFree(p);
        dbuf.clear();
        for (auto c : comms)  // after a failure, peers may never join a collective: abort, don't destroy
            if (c) (void)(host.aborted() ? ncclCommAbort(c) : ncclCommDestroy(c));
        comms.clear();
    }
    void abort() { host.abort(); }
    int init(const std::vector<Dec> &decs, bool injected_failure) {
        if (!rccl) return FPLDPC_OK;
        if (injected_failure) return fail(FPLDPC_ERR_HIP, "ncclCommInitAll: injected failure (fpldpc_testing_sim_inject)");
        std::vector<int> devs(ndev);
        for (int i = 0; i < ndev; ++i) devs[i] = decs[i].device();
        comms.assign(ndev, nullptr);
        ncclResult_t r = ncclCommInitAll(comms.data(), ndev, devs.data());
        if (r != ncclSuccess) {
            comms.clear();
            return fail(FPLDPC_ERR_HIP, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
        }
        dbuf.assign(ndev, nullptr);
        for (int i = 0; i < ndev; ++i) {
            if (hipSetDevice(devs[i]) != hipSuccess) return fail(FPLDPC_ERR_HIP, "hipSetDevice");
            HIP_TRY(hipMalloc((void **)&dbuf[i], sizeof(int64_t) * kWords * (ndev + 1)));
        }
        return FPLDPC_OK;
    }
    // Wait for this rank's collective (RCCL mode) while watching for another rank's failure.
    int sync(int rank, hipStream_t st) {
        for (;;) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) return FPLDPC_OK;
            if (q != hipErrorNotReady) return fail_hip((int)q, "hipStreamQuery (collective)");
            if (host.aborted()) {
                (void)ncclCommAbort(comms[rank]);
                comms[rank] = nullptr;
                return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed (collective aborted)");
            }
            std::this_thread::yield();
        }
    }
    // all[ndev][kWords] = every rank's `mine`, in rank order
    int allgather(int rank, hipStream_t st, const int64_t *mine, int64_t *all) {
        if (!rccl) return host.allgather(rank, mine, all) ? FPLDPC_OK : other_rank_failed();
        if (host.aborted()) return other_rank_failed();
        int64_t *send = dbuf[rank], *recv = dbuf[rank] + kWords;
        HIP_TRY(hipMemcpyAsync(send, mine, sizeof(int64_t) * kWords, hipMemcpyHostToDevice, st));
        ncclResult_t r = ncclAllGather(send, recv, kWords, ncclInt64, comms[rank], st);
        if (r != ncclSuccess) return fail(FPLDPC_ERR_HIP, std::string("ncclAllGather: ") + ncclGetErrorString(r));
        HIP_TRY(hipMemcpyAsync(all, recv, sizeof(int64_t) * kWords * ndev, hipMemcpyDeviceToHost, st));
        return sync(rank, st);
    }
    // sum over ranks of `mine` (kWords)
    int allreduce(int rank, hipStream_t st, const int64_t *mine, int64_t *sum) {
        if (!rccl) return host.allreduce(rank, mine, sum) ? FPLDPC_OK : other_rank_failed();
        if (host.aborted()) return other_rank_failed();
        int64_t *buf = dbuf[rank];
        HIP_TRY(hipMemcpyAsync(buf, mine, sizeof(int64_t) * kWords, hipMemcpyHostToDevice, st));
        ncclResult_t r = ncclAllReduce(buf, buf, kWords, ncclInt64, ncclSum, comms[rank], st);
        if (r != ncclSuccess) return fail(FPLDPC_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
        HIP_TRY(hipMemcpyAsync(sum, buf, sizeof(int64_t) * kWords, hipMemcpyDeviceToHost, st));
        return sync(rank, st);
    }
};

struct Shared {
    const fpldpc_sim_params *sp = nullptr;
    int ndev = 1, chunk = 0;
    int64_t frame_end = 0;
    Exchange *ex = nullptr;
    std::vector<Rank *> ranks;  // on_frame, harvest: rank 0's thread reads every rank's slot in frame order
    fpldpc_harvest *hv = nullptr;
    bool biased = false;       // a bias: rank 0's thread adds the weighted sums in frame order
    fpldpc_bias_sums wsums = bias_sums_start();
    // per rank outcome
    std::vector<int> status;
    std::vector<std::string> message;
    plan::Sums result;
    int64_t decoded = 0;
    int fail_rank = -1;  // fpldpc_testing_sim_inject (include/fpldpc_testing.h)
    int64_t fail_round = 0;
    bool fail_abrupt = false;
};

// Test-only fault injection (include/fpldpc_testing.h), set by an explicit call, never from the
// environment.
struct Inject {
    std::atomic<int> fail_rank{-1};
    std::atomic<int64_t> fail_round{0};
    std::atomic<bool> abrupt{false};
    std::atomic<int> comm_init{0};  // 1: ncclCommInitAll fails; 2: also AUTO attempts RCCL on one device
};
Inject g_inject;

void pack(const plan::Sums &s, int64_t w4, int64_t *out) {
    out[0] = s.bit_errors;
    out[1] = s.frame_errors;
    out[2] = s.frames;
    out[3] = s.iter_sum;
    out[4] = w4;
}
plan::Sums unpack(const int64_t *w) {
    plan::Sums s;
    s.bit_errors = w[0];
    s.frame_errors = w[1];
    s.frames = w[2];
    s.iter_sum = w[3];
    return s;
}

// The round's frames in frame order, on rank 0's thread between two barriers: slot `cur` of the ranks up to the one
// holding the stop frame (sr; every rank if sr < 0), each frame to on_frame, to the harvest and to the weighted
// sums, up to and including the stop frame.  run: the counted frames before this round.
void frame_order(Shared &sh, int cur, int sr, plan::Sums run) {
    const fpldpc_sim_params *sp = sh.sp;
    for (int i = 0; i <= (sr < 0 ? sh.ndev - 1 : sr); ++i) {
        const Rank &Ri = *sh.ranks[i];
        const Slot &xi = Ri.s[cur];
        int64_t rec = 0;  // the chunk's codeword-error frames so far: the next record of its buffer
        for (int64_t f = 0; f < xi.frames; ++f) {
            if (sp->on_frame) sp->on_frame(sp->on_frame_ctx, xi.first + f, Ri.its(xi)[f], Ri.blk(xi)[f]);
            if (sh.hv) {
                const int32_t w = xi.h_hv[f];
                const bool keep = w > 0 && rec < Ri.cap;  // add_frame reads the row of a record only
                const uint32_t *recs = (const uint32_t *)(xi.h_hv + 2 * xi.frames);
                sh.hv->add_frame(xi.first + f, Ri.its(xi)[f], Ri.blk(xi)[f], w, xi.h_hv[xi.frames + f],
                                 keep ? recs + (size_t)rec * Ri.row_words : nullptr);
                rec += w > 0;
            }
            if (sh.biased) bias_sums_add(sh.wsums, xi.h_logw[f], Ri.blk(xi)[f]);
            run.add_frame(Ri.blk(xi)[f], Ri.its(xi)[f]);
            if (i == sr && sp->max_frame_errors > 0 && run.frame_errors >= sp->max_frame_errors) return;
        }
    }
}

// One rank's frame loop.  Every rank runs the same rounds and the same collective calls; a rank
// that fails reports its status through the round's all-gather so that all stop together.
int rank_loop(Shared &sh, int rank) {
    Rank &R = *sh.ranks[rank];
    const fpldpc_sim_params *sp = sh.sp;
    const int ndev = sh.ndev;
    hipStream_t st = R.exchange_stream();
    const int64_t need = sp->max_frame_errors;
    auto range = [&](int64_t round, int rk) {
        return plan::rank_range(sp->first_frame, sh.frame_end, sh.chunk, ndev, round, rk);
    };
    plan::Sums total;  // the counted frames before the current round (identical on every rank)
    int err = FPLDPC_OK;
    std::string own;  // this rank's first error message
    int cur = 0;
    int64_t round = 0;
    err = R.generate(R.s[0], range(0, rank));
    if (!err) err = R.submit(R.s[0]);
    std::vector<int64_t> all((size_t)ndev * kWords);
    int64_t mine[kWords], red[kWords];
    for (;;) {
        Slot &x = R.s[cur], &y = R.s[cur ^ 1];
        const bool more = plan::round_has_frames(sp->first_frame, sh.frame_end, sh.chunk, ndev, round + 1);
        y.frames = 0;
        if (!err && rank == sh.fail_rank && round == sh.fail_round) {
            err = fail(FPLDPC_ERR_HIP, "injected failure (fpldpc_testing_sim_inject)");
            own = fpldpc_last_error();
            if (sh.fail_abrupt) {
                for (const Slot &z : R.s) (void)hipStreamSynchronize(z.dec.stream());
                return err;
            }
        }
        // overlap: the next round's host channel while the GPU decodes this one, and with two
        // decoders the next round's decode as well
        if (!err && more) err = R.generate(y, range(round + 1, rank));
        if (!err && more && R.overlap) err = R.submit(y);
        if (!err) err = R.wait(x);
        if (err && own.empty()) own = fpldpc_last_error();
        plan::Sums loc;
        if (!err)
            for (int64_t f = 0; f < x.frames; ++f) loc.add_frame(R.blk(x)[f], R.its(x)[f]);
        pack(loc, err, mine);
        int e2 = sh.ex->allgather(rank, st, mine, all.data());
        if (e2 && err) return fail(err, own);  // this rank's own error, not the abort it caused
        if (e2) return e2;
        int first_err = FPLDPC_OK;
        for (int i = 0; i < ndev && !first_err; ++i) first_err = (int)all[(size_t)i * kWords + 4];
        if (first_err) return err ? err : fail(first_err, "another rank of the simulation failed");
        std::vector<plan::Sums> sums(ndev);
        for (int i = 0; i < ndev; ++i) sums[i] = unpack(&all[(size_t)i * kWords]);
        const int sr = plan::stop_rank(sums.data(), ndev, total.frame_errors, need);
        if (sp->on_frame || sh.hv || sh.biased) {  // frame order across ranks: rank 0's thread serves everyone
            if (!sh.ex->host.bar.wait()) return other_rank_failed();
            if (rank == 0) frame_order(sh, cur, sr, total);
            if (!sh.ex->host.bar.wait()) return other_rank_failed();
        }
        if (sr < 0) {
            for (int i = 0; i < ndev; ++i) total.add(sums[i]);
            if (!more) {
                pack(plan::Sums(), R.decoded, mine);
                break;
            }
            if (!R.overlap) err = R.submit(y);
            cur ^= 1;
            ++round;
            continue;
        }
        // the stop frame lies in rank sr's chunk: ranks before it count whole chunks, rank sr up
        // to the stop frame, ranks after it nothing
        plan::Sums contrib;
        if (rank < sr) contrib = loc;
        if (rank == sr) {
            int64_t prior = total.frame_errors;
            for (int i = 0; i < sr; ++i) prior += sums[i].frame_errors;
            plan::scan_chunk(R.blk(x), R.its(x), x.frames, prior, need, &contrib);
        }
        pack(contrib, R.decoded, mine);
        break;
    }
    int e3 = sh.ex->allreduce(rank, st, mine, red);
    if (e3) return e3;
    total.add(unpack(red));
    // drain: a generated-but-not-submitted slot holds nothing on the device; a submitted one (two
    // chunks in flight, decoded past the stop frame) is waited for, not counted
    for (const Slot &z : R.s) HIP_TRY(hipStreamSynchronize(z.dec.stream()));
    HIP_TRY(hipStreamSynchronize(st));
    if (rank == 0) {
        sh.result = total;
        sh.decoded = red[4];
    }
    return FPLDPC_OK;
}

int validate(const Dec &dec, const fpldpc_sim_params *sp) {
    const int n = dec.code().n;
    if (sp->max_frame_errors <= 0 && sp->max_frames <= 0)
        return fail(FPLDPC_ERR_ARG, "ber_sim needs max_frame_errors or max_frames");
    if (sp->count_mode != FPLDPC_COUNT_BITS && sp->count_mode != FPLDPC_COUNT_ITERS)
        return fail(FPLDPC_ERR_ARG, "bad count_mode");
    if (sp->random_info) {
        if (sp->random_info != 1) return fail(FPLDPC_ERR_ARG, "random_info must be 0 or 1");
        if (!sp->device_channel)
            return fail(FPLDPC_ERR_ARG, "random_info needs device_channel = 1 (the host channel takes one codeword only)");
        if (sp->codeword || sp->info_index || sp->info_bits)
            return fail(FPLDPC_ERR_ARG,
                        "random_info: codeword, info_index and info_bits must be NULL (the simulation owns them)");
        if (sp->n_forced > 0)
            return fail(FPLDPC_ERR_ARG, "random_info: no forced positions (shortening fixes information bits)");
        if (sp->info_seed < 1 || sp->info_seed > 2147483646)
            return fail(FPLDPC_ERR_ARG, "random_info: info_seed must be in 1 .. 2^31 - 2");
    } else if (sp->count_mode == FPLDPC_COUNT_BITS && (sp->k <= 0 || !sp->info_index || !sp->info_bits)) {
        return fail(FPLDPC_ERR_ARG, "FPLDPC_COUNT_BITS needs info_index / info_bits");
    }
    if (sp->n_forced < 0 || (sp->n_forced > 0 && !sp->forced_index)) return fail(FPLDPC_ERR_ARG, "bad forced list");
    for (int i = 0; i < sp->n_forced; i++)
        if (sp->forced_index[i] < 0 || sp->forced_index[i] >= n) return fail(FPLDPC_ERR_ARG, "forced index out of range");
    if (sp->forced_llr < -32768 || sp->forced_llr > 32767) return fail(FPLDPC_ERR_ARG, "forced_llr must fit int16");
    return FPLDPC_OK;
}

// The rules a bias adds to a simulation's (include/fpldpc.h, fpldpc_ber_sim_biased)
int validate_bias(const Dec &dec, const fpldpc_sim_params *sp, const fpldpc_bias &b) {
    if (sp->device_channel != 1)
        return fail(FPLDPC_ERR_ARG, "a bias needs device_channel = 1 (the host channel's path is not biased)");
    if (sp->count_mode != FPLDPC_COUNT_BITS) return fail(FPLDPC_ERR_ARG, "a bias needs count_mode = FPLDPC_COUNT_BITS");
    if (b.n != dec.code().n) return fail(FPLDPC_ERR_ARG, "the bias was made for another n than the decoders' code");
    for (int i = 0; i < sp->n_forced; i++)
        if (std::binary_search(b.pos.begin(), b.pos.end(), sp->forced_index[i]))
            return fail(FPLDPC_ERR_ARG, "a forced position is also a biased one (bias and shortening must not overlap)");
    return FPLDPC_OK;
}

// The float decoder's envelope (float_setup, fpldpc_float.hip, which would otherwise refuse at a slot's first decode,
// after frames have been generated) and its messages.  create_decoder bounds n and the check degree more tightly; the variable degree it does not.
int validate_float(const Dec &dec) {
    const fpldpc_code &c = dec.code();
    if (c.n > 16384) return fail(FPLDPC_ERR_UNSUPPORTED, "float decoder: n > 16384");
    if (c.dc_max > 255) return fail(FPLDPC_ERR_UNSUPPORTED, "float decoder: check degree > 255");
    if (c.dv_max > 255) return fail(FPLDPC_ERR_UNSUPPORTED, "float decoder: variable degree > 255");
    return FPLDPC_OK;
}

// What an entry point adds to a simulation
struct SimOptions {
    fpldpc_harvest *hv = nullptr;      // the harvest to fill, or null
    fpldpc_bias *bias = nullptr;       // the shift of the channel, or null
    int source = FPLDPC_NOISE_LEHMER;  // the noise source (include/fpldpc.h)
    bool harvest_required = false;     // a *_ber_sim_harvest call: one without a harvest is an error
    bool bias_required = false;        // a *_ber_sim_biased call: one without a bias is an error
    SimOptions &require_harvest() { return harvest_required = true, *this; }
    SimOptions &require_bias() { return bias_required = true, *this; }
};

int run_sim(const std::vector<Dec> &dv, const fpldpc_sim_params *sp, int collective, fpldpc_sim_result *out, int32_t *used,
            const SimOptions &opt) {
    fpldpc_harvest *const hv = opt.hv;
    fpldpc_bias *const bias = opt.bias;
    const int source = opt.source;
    const int ndev = (int)dv.size();
    if (ndev < 1 || !sp || !out) return fail(FPLDPC_ERR_ARG, "null argument");
    if (source != FPLDPC_NOISE_LEHMER && source != FPLDPC_NOISE_PHILOX)
        return fail(FPLDPC_ERR_ARG, "bad noise source (FPLDPC_NOISE_LEHMER or FPLDPC_NOISE_PHILOX)");
    if (source == FPLDPC_NOISE_PHILOX &&
        (sp->seed < 0 || sp->first_frame < 0 || (sp->max_frames > 0 && sp->first_frame > INT64_MAX - sp->max_frames)))
        return fail(FPLDPC_ERR_ARG, "philox: 0 <= seed and first_frame + max_frames < 2^63");
    if (opt.harvest_required && !hv) return fail(FPLDPC_ERR_ARG, "null harvest");
    if (opt.bias_required && !bias) return fail(FPLDPC_ERR_ARG, "null bias");
    if (hv && sp->count_mode != FPLDPC_COUNT_BITS)
        return fail(FPLDPC_ERR_ARG, "a harvest needs count_mode = FPLDPC_COUNT_BITS");
    if (collective < FPLDPC_COLL_AUTO || collective > FPLDPC_COLL_HOST) return fail(FPLDPC_ERR_ARG, "bad collective");
    bool distinct = true;
    for (int i = 0; i < ndev; ++i) {
        if (!dv[i]) return fail(FPLDPC_ERR_ARG, "null decoder");
        if (dv[i].code().n != dv[0].code().n || dv[i].code().m != dv[0].code().m)
            return fail(FPLDPC_ERR_ARG, "decoders of different codes");
        for (int j = 0; j < i; ++j) {
            if (dv[j] == dv[i]) return fail(FPLDPC_ERR_ARG, "the same decoder twice (a decoder is single-stream)");
            distinct = distinct && dv[j].device() != dv[i].device();
        }
        int st = validate(dv[i], sp);
        if (st) return st;
        if (bias && (st = validate_bias(dv[i], sp, *bias))) return st;
        if (dv[i].fl && (st = validate_float(dv[i]))) return st;
        const fpldpc_code &c = dv[i].code();
        if (hv && (hv->n != c.n || hv->m != c.m || hv->dc != c.dc_max || hv->clist != c.clist))
            return fail(FPLDPC_ERR_ARG, "the harvest was made from another code than the decoders'");
    }
    if (hv) hv->clear();
    if (bias) bias->sums = fpldpc_bias_sums{};
    static_assert(FPLDPC_COLL_AUTO == plan::kCollAuto && FPLDPC_COLL_RCCL == plan::kCollRccl &&
                  FPLDPC_COLL_HOST == plan::kCollHost, "collective codes");
    // (test hook: comm_init == 2 makes AUTO attempt RCCL with a single decoder, so that its fallback
    // runs on a one-GPU box)
    const bool rccl = plan::try_rccl(collective, distinct, ndev) ||
                      (collective == FPLDPC_COLL_AUTO && ndev == 1 && g_inject.comm_init.load() == 2);
    if (rccl && !distinct) return fail(FPLDPC_ERR_ARG, "RCCL needs the decoders on distinct devices");
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGuard restore(-1);  // the ranks below set their own devices: the caller gets its own back
    const char *ov = getenv("FPLDPC_SIM_OVERLAP");
    const bool overlap = !(ov && *ov == '0');

    Shared sh;
    sh.sp = sp;
    sh.hv = hv;
    sh.biased = bias != nullptr;
    sh.ndev = ndev;
    sh.chunk = sp->chunk > 0 ? sp->chunk : 16384;
    if (sp->max_frames > 0) sh.chunk = (int)std::min<int64_t>(sh.chunk, sp->max_frames);
    sh.frame_end = sp->max_frames > 0 ? sp->first_frame + sp->max_frames : INT64_MAX;
    Exchange ex(ndev, rccl);
    sh.ex = &ex;
    std::vector<std::unique_ptr<Rank>> ranks(ndev);
    for (int i = 0; i < ndev; ++i) {
        ranks[i].reset(new Rank);
        ranks[i]->dec = dv[i];
        ranks[i]->sp = sp;
        ranks[i]->chunk = sh.chunk;
        ranks[i]->n = dv[i].code().n;
        ranks[i]->overlap = overlap;
        ranks[i]->hv = hv;
        ranks[i]->bias = bias;
        ranks[i]->source = source;
        ranks[i]->fl = dv[i].fl;
        if (hipSetDevice(dv[i].device()) != hipSuccess) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
        if (const int st = ranks[i]->setup()) return st;
        sh.ranks.push_back(ranks[i].get());
    }
    int st = ex.init(dv, g_inject.comm_init.load() != 0);
    const int coll_used = plan::exchange_after_init(collective, rccl, st == FPLDPC_OK);
    if (coll_used < 0) return st;
    if (st) {  // AUTO: identical counters without RCCL, through host memory
        fprintf(stderr, "fpldpc_ber_sim_multi: %s; exchanging the counters through host memory instead\n",
                fpldpc_last_error());
        ex.release();
        ex.rccl = false;
        st = FPLDPC_OK;
    }
    sh.fail_rank = g_inject.fail_rank.load();
    sh.fail_round = g_inject.fail_round.load();
    sh.fail_abrupt = g_inject.abrupt.load();
    sh.status.assign(ndev, FPLDPC_OK);
    sh.message.assign(ndev, std::string());
    if (ndev == 1) {  // in the calling thread (its device and error state)
        if (hipSetDevice(dv[0].device()) != hipSuccess) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
        st = rank_loop(sh, 0);
        if (st) return st;
    } else {
        std::vector<std::thread> th;
        for (int i = 0; i < ndev; ++i)
            th.emplace_back([&, i] {
                if (hipSetDevice(dv[i].device()) != hipSuccess) {
                    sh.status[i] = fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
                } else {
                    sh.status[i] = rank_loop(sh, i);
                }
                if (sh.status[i]) {
                    sh.message[i] = fpldpc_last_error();
                    ex.abort();  // every failure ends the others' waits (barrier, polled collectives)
                }
            });
        for (auto &t : th) t.join();
        // report the rank that failed first-hand, not one that only saw the abort
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < ndev; ++i)
                if (sh.status[i] && (pass == 1 || sh.message[i].find("another rank") == std::string::npos))
                    return fail(sh.status[i], "rank " + std::to_string(i) + ": " + sh.message[i]);
    }
    fpldpc_sim_result r{};
    r.bit_errors = sh.result.bit_errors;
    r.frame_errors = sh.result.frame_errors;
    r.frames = sh.result.frames;
    r.iter_sum = sh.result.iter_sum;
    r.frames_decoded = sh.decoded;
    r.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out = r;
    if (bias) bias->sums = sh.wsums;
    if (used) *used = coll_used;  // what ran, after any AUTO fallback
    return FPLDPC_OK;
}

// The entry points' handles as Dec (a null handle stays a null Dec; no list at all is an empty one); fl: the float
// decoder of a fpldpc_decoder_t
Dec from(fpldpc_decoder_t d, bool fl) { return {d, nullptr, fl}; }
Dec from(fpldpc_layered_t d, bool) { return {nullptr, d, false}; }
Dec from(fpldpc_minsum_t d, bool) { return from(d ? d->lay : nullptr, false); }

// The single form of an entry point, and the form over a list of decoders
template <typename T>
int sim_one(T dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out, bool fl = false) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return run_sim({from(dec, fl)}, sp, FPLDPC_COLL_HOST, out, nullptr, SimOptions());
}
template <typename T>
int sim_multi(const T *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective, fpldpc_sim_result *out,
              int32_t *collective_used, const SimOptions &opt, bool fl = false) {
    std::vector<Dec> v;
    for (int i = 0; decs && i < ndev; ++i) v.push_back(from(decs[i], fl));
    return run_sim(v, sp, collective, out, collective_used, opt);
}

}  // namespace

extern "C" {

void fpldpc_sim_params_default(fpldpc_sim_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->seed = 123456789;  // rngs.cpp:45
    p->frac_bits = 4;     // ArrayLDPCMacro.h:36
    p->max_frame_errors = 100;  // PerfTest.cpp:97
    p->count_mode = FPLDPC_COUNT_BITS;
    p->info_seed = 987654321;
}

int fpldpc_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) { return sim_one(dec, sp, out); }
int fpldpc_layered_ber_sim(fpldpc_layered_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    return sim_one(dec, sp, out);
}
int fpldpc_minsum_ber_sim(fpldpc_minsum_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    return sim_one(dec, sp, out);
}
int fpldpc_float_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    return sim_one(dec, sp, out, true);
}

int fpldpc_ber_sim_multi(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                         fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions());
}
int fpldpc_layered_ber_sim_multi(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions());
}
int fpldpc_minsum_ber_sim_multi(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                                fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions());
}

int fpldpc_ber_sim_harvest(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                           fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h}.require_harvest());
}
int fpldpc_layered_ber_sim_harvest(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                   int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                   int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h}.require_harvest());
}
int fpldpc_minsum_ber_sim_harvest(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h}.require_harvest());
}

int fpldpc_ber_sim_biased(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b}.require_bias());
}
int fpldpc_layered_ber_sim_biased(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b}.require_bias());
}
int fpldpc_minsum_ber_sim_biased(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                 int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b}.require_bias());
}

int fpldpc_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                          int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b, source});
}
int fpldpc_layered_ber_sim_source(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                  fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b, source});
}
int fpldpc_minsum_ber_sim_source(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                 fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b, source});
}
int fpldpc_float_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                fpldpc_sim_result *out, int32_t *collective_used) {
    return sim_multi(decs, ndev, sp, collective, out, collective_used, SimOptions{h, b, source}, true);
}

void fpldpc_testing_sim_inject(int32_t fail_rank, int64_t fail_round, int32_t abrupt, int32_t fail_comm_init) {
    g_inject.fail_rank = fail_rank;
    g_inject.fail_round = fail_round;
    g_inject.abrupt = abrupt != 0;
    g_inject.comm_init = fail_comm_init;
}

}  // extern "C"
