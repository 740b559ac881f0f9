// fpldpc_sim.cpp -- ordered BER/FER simulation around one or several GPU decoders
// (fpldpc_ber_sim, fpldpc_ber_sim_multi, and the same pair for the layered and the flooding min-sum decoder).
//
// The reference harness decodes one frame at a time and stops at the frame whose decode brings the
// frame-error count to 100 (PerfTest.cpp:97-135, 275-311, 385-426, 485-511, 574-600).  Here frames
// are decoded in chunks: each rank (one decoder, one device, one host thread) holds two pinned /
// device buffer pairs on its decoder's stream, so that the host generates the next chunk's LLRs
// while the GPU decodes this one (or, with device_channel, the LLRs are generated on the device in
// the same stream, fpldpc_gen.hip).  Rounds, ranges and the stop rule are fpldpc_sim_plan.hpp's:
// per round the ranks exchange their chunk sums (an all-gather), the rank holding the stop frame
// scans its chunk for it, and one all-reduce adds the contributions -- so every counter equals the
// serial loop's for any number of ranks.  With decoders on distinct devices the exchange is RCCL
// (ncclCommInitAll in this process, collectives on each decoder's stream, over xGMI on an MI355X
// node); decoders sharing a device exchange through host memory.  Frames of the last round past the
// stop frame are decoded but not counted.
//
// Two chunks in flight per rank: the two slots decode on two decoders (the caller's and a twin with
// the same code and parameters) on their own streams, and round r+1's chunk is submitted before
// round r's is waited for, so the next chunk's workgroups take the CUs that a chunk's last frames
// leave idle (with early termination a chunk ends on a few frames running max_iter iterations
// alone).  The exchange runs on a third stream.  Counters are unchanged: chunks are still counted
// in round order, and a chunk decoded past the stop frame is drained, not counted.
// FPLDPC_SIM_OVERLAP=0 submits each chunk after the previous round's exchange, on one decoder.
//
// random_info: each chunk's frames carry fresh information bits (fpldpc_sim_source.hip), encoded and sent
// through the device channel with a codeword per frame, and the decode's hard decisions are counted against
// them, all on the slot's stream (include/fpldpc.h); rounds, exchange and stop rule do not know of it.
//
// Harvest (the *_ber_sim_harvest entry points; fpldpc_harvest.hip): each chunk's decode writes its hard
// decisions, and on the slot's stream, before its `done` event, the scan kernel gives every frame's (weight,
// unsat) and err / syn row, the ordered compaction gathers the codeword-error frames' rows behind the pairs, and
// one copy takes both to pinned memory.  After the stop decision rank 0's thread appends the ranks' chunks to the harvest in frame
// order up to the stop frame, where on_frame is called.  Without a harvest none of this exists.
//
// Bias (the *_ber_sim_biased entry points; fpldpc_bias.hip): each slot has the chunk's log-weights on the device
// and a pinned twin.  The patch kernel follows the slot's channel launch, before the forced positions are
// written; the copy goes with the slot's other copies, before `done`.  In the frame-order loop that serves
// on_frame and the harvest, rank 0's thread adds the weighted sums (include/fpldpc.h, fpldpc_bias_sums) up to
// and including the stop frame: they depend on neither the chunk size nor the number of ranks.  Without a bias
// none of this exists.
//
// Source (the *_ber_sim_source entry points; fpldpc_source.hip): the three places that make noise -- generate, the
// slot's channel launch and its patch launch -- take the noise source; every other entry point passes the Lehmer
// stream and launches and allocates what it did before.
//
// Float (fpldpc_float_ber_sim, fpldpc_float_ber_sim_source): the same loop around fpldpc_decode_float.  The channel --
// host or device, either source, the patch kernel included -- writes FPLDPC_LLR_F64 into slots of 8 bytes per value, the
// forced positions receive the double forced_llr * 2^-frac_bits (fpldpc_sim_source.hip), and there is no int16
// overflow word to zero, copy or test.  Every other entry point issues the HIP calls it issued before.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <cmath>

#include "fpldpc_bias.hpp"
#include "fpldpc_harvest.hpp"
#include "fpldpc_internal.hpp"
#include "fpldpc_layered.hpp"
#include "fpldpc_sim_plan.hpp"
#include "fpldpc_sim_source.hpp"
#include "fpldpc_source.hpp"
#include "fpldpc_testing.h"

using namespace fpldpc;

namespace {

// The decoder behind a rank or a slot: the six things the simulation asks of one, for fpldpc_decoder_t and
// for fpldpc_layered_t (fpldpc_minsum_t enters as the layered object it wraps); fl: the fpldpc_decoder_t decodes
// with fpldpc_decode_float, from double LLRs.
struct Dec {
    fpldpc_decoder_t flood = nullptr;
    fpldpc_layered_t lay = nullptr;
    bool fl = false;
    DecoderCore *core() const { return flood ? static_cast<DecoderCore *>(flood) : lay; }
    explicit operator bool() const { return core() != nullptr; }
    bool operator==(const Dec &o) const { return core() == o.core(); }
    hipStream_t stream() const { return core()->stream; }
    int device() const { return core()->device; }
    fpldpc_code &code() const { return core()->code; }
    int decode(const void *llr, int32_t frames, uint32_t *hard, int32_t *iters, int32_t *bit_errors,
               hipStream_t st) const {
        if (fl)
            return fpldpc_decode_float(flood, static_cast<const double *>(llr), frames, hard, iters, nullptr, nullptr,
                                       bit_errors, nullptr, st);
        return flood ? fpldpc_decode(flood, llr, FPLDPC_LLR_I16, frames, hard, iters, nullptr, nullptr, bit_errors, nullptr, st)
                     : fpldpc_layered_decode(lay, llr, FPLDPC_LLR_I16, frames, hard, iters, nullptr, nullptr, bit_errors,
                                             nullptr, st);
    }
    int set_reference(const int32_t *info_index, const uint8_t *info_bits, int32_t k) const {
        return flood ? fpldpc_set_reference(flood, info_index, info_bits, k)
                     : fpldpc_layered_set_reference(lay, info_index, info_bits, k);
    }
    int create_twin(Dec *out) const {
        out->fl = fl;  // its float state is made by its first decode, as the caller's
        return flood ? decoder_create_twin(flood, &out->flood) : layered_create_twin(lay, &out->lay);
    }
    void destroy() {
        if (flood) (void)fpldpc_decoder_destroy(flood);
        if (lay) (void)fpldpc_layered_destroy(lay);
        flood = nullptr;
        lay = nullptr;
    }
};

struct Slot {
    void *h_llr = nullptr;     // int16 [chunk][n]; float: double
    int32_t *h_out = nullptr;  // [chunk] bit errors, [chunk] iterations, [1] int16 overflow count
    void *d_llr = nullptr;
    int32_t *d_out = nullptr;
    hipEvent_t done = nullptr;
    int64_t frames = 0;
    int64_t first = 0;
    Dec dec;  // decodes this slot's chunks, on its own stream
    // random_info: the chunk's information bits [chunk][k], codewords [chunk][n] and hard decisions
    // [chunk][hard words], and this stream's encoder (an encoder is single-stream)
    uint8_t *d_info = nullptr;
    uint8_t *d_cw = nullptr;
    uint32_t *d_hard = nullptr;
    fpldpc_encoder_t enc = nullptr;
    // harvest: one block on the device and its pinned twin, copied once per chunk -- weight [frames], unsat
    // [frames], then the compaction's records [min(cap, frames)][row words]; every frame's err | syn row
    // [chunk][row words] and the compaction's scratch [chunk] stay on the device
    int32_t *d_hv = nullptr, *h_hv = nullptr, *d_pos = nullptr;
    uint32_t *d_rows = nullptr;
    // bias: the chunk's log-weights [chunk] and their pinned twin
    double *d_logw = nullptr, *h_logw = nullptr;
};

// One rank: a decoder, its stream, two chunk slots.
struct Rank {
    Dec dec;
    Dec twin;  // second decoder (two chunks in flight), owned here
    hipStream_t xs = nullptr;         // the exchange's stream when two chunks are in flight
    bool overlap = false;
    const fpldpc_sim_params *sp = nullptr;
    int chunk = 0, n = 0;
    Slot s[2];
    int32_t *d_forced = nullptr;
    const uint8_t *d_cw = nullptr;
    int32_t *d_info_idx = nullptr;  // random_info: the encoder's info positions [k]
    int k = 0;
    int64_t decoded = 0;
    fpldpc_harvest *hv = nullptr;  // harvest: the object to fill (rank 0's thread does), or null
    uint16_t *d_table = nullptr;   // this device's copy of its check table
    uint8_t *d_hv_cw = nullptr;    // the fixed codeword [n] on the device where the host channel keeps it on the host
    int cap = 0, row_words = 0;    // records per chunk buffer, words per record row (err | syn)
    const fpldpc_bias *bias = nullptr;  // bias: the shift of this simulation's channel, or null
    int32_t *d_bias_pos = nullptr;      // this device's copy of its positions and shifts
    double *d_bias_shift = nullptr;
    int source = FPLDPC_NOISE_LEHMER;  // the noise source of generate, launch_channel and launch_bias_patch
    bool fl = false;                   // float: the slots hold doubles
    int llr_type() const { return fl ? FPLDPC_LLR_F64 : FPLDPC_LLR_I16; }
    size_t llr_size() const { return fl ? sizeof(double) : sizeof(int16_t); }
    double forced_double() const { return std::ldexp((double)sp->forced_llr, -sp->frac_bits); }
    ~Rank() {
        // a rank that left early (an error) may still have a chunk in flight: let it finish before
        // its buffers and the twin decoder go
        for (auto &x : s)
            if (x.dec) (void)hipStreamSynchronize(x.dec.stream());
        twin.destroy();
        if (xs) (void)hipStreamDestroy(xs);
        (void)hipFree(d_forced);
        (void)hipFree(d_info_idx);
        (void)hipFree(d_table);
        (void)hipFree(d_hv_cw);
        (void)hipFree(d_bias_pos);
        (void)hipFree(d_bias_shift);
        for (auto &x : s) {
            (void)hipFree(x.d_logw);
            (void)hipHostFree(x.h_logw);
            (void)hipFree(x.d_hv);
            (void)hipFree(x.d_pos);
            (void)hipFree(x.d_rows);
            (void)hipHostFree(x.h_hv);
            (void)hipFree(x.d_info);
            (void)hipFree(x.d_cw);
            (void)hipFree(x.d_hard);
            if (x.enc) fpldpc_encoder_free(x.enc);
            (void)hipHostFree(x.h_llr);
            (void)hipHostFree(x.h_out);
            (void)hipFree(x.d_llr);
            (void)hipFree(x.d_out);
            if (x.done) (void)hipEventDestroy(x.done);
        }
    }
    hipStream_t exchange_stream() const { return xs ? xs : dec.stream(); }
    int setup() {  // on the decoder's device
        const size_t llr_bytes = (size_t)chunk * n * llr_size();
        s[0].dec = s[1].dec = dec;
        if (overlap) {
            int st = dec.create_twin(&twin);
            if (st) return st;
            s[1].dec = twin;
            HIP_TRY(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking));
        }
        for (auto &x : s) {
            if (!sp->device_channel) HIP_TRY(hipHostMalloc((void **)&x.h_llr, llr_bytes, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc((void **)&x.h_out, ((size_t)chunk * 2 + 1) * sizeof(int32_t), hipHostMallocDefault));
            HIP_TRY(hipMalloc((void **)&x.d_llr, llr_bytes));
            HIP_TRY(hipMalloc((void **)&x.d_out, ((size_t)chunk * 2 + 1) * sizeof(int32_t)));
            HIP_TRY(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
        }
        if (sp->device_channel) {
            if (sp->codeword) {
                HIP_TRY(hipMalloc((void **)&d_forced, sizeof(int32_t) * std::max(sp->n_forced, 0) + n));
                d_cw = reinterpret_cast<const uint8_t *>(d_forced + std::max(sp->n_forced, 0));
                HIP_TRY(hipMemcpy((void *)d_cw, sp->codeword, n, hipMemcpyHostToDevice));
            } else if (sp->n_forced > 0) {
                HIP_TRY(hipMalloc((void **)&d_forced, sizeof(int32_t) * sp->n_forced));
            }
            if (sp->n_forced > 0)
                HIP_TRY(hipMemcpy(d_forced, sp->forced_index, sizeof(int32_t) * sp->n_forced, hipMemcpyHostToDevice));
        }
        if (hv) {
            int st = setup_harvest();
            if (st) return st;
        }
        if (bias) {
            int st = bias_upload_tables(*bias, &d_bias_pos, &d_bias_shift);
            if (st) return st;
            for (auto &x : s) {
                HIP_TRY(hipMalloc((void **)&x.d_logw, (size_t)chunk * sizeof(double)));
                HIP_TRY(hipHostMalloc((void **)&x.h_logw, (size_t)chunk * sizeof(double), hipHostMallocDefault));
            }
        }
        if (sp->random_info) return setup_source();
        if (sp->count_mode == FPLDPC_COUNT_BITS) {
            int st = dec.set_reference(sp->info_index, sp->info_bits, sp->k);
            if (!st && twin) st = twin.set_reference(sp->info_index, sp->info_bits, sp->k);
            return st;
        }
        return FPLDPC_OK;
    }
    // random_info: per slot an encoder derived from the decoder's own code, warmed so that its device tables
    // and packed-info scratch exist before the first chunk, and the chunk's info / codeword / hard buffers
    int setup_source() {
        const size_t hw = ((size_t)n + 31) / 32;
        for (auto &x : s) {
            int st = fpldpc_encoder_from_code(&dec.code(), &x.enc);
            if (st) return st;
            k = x.enc->k;
            if (k < 1) return fail(FPLDPC_ERR_ARG, "random_info: the code has no information bits");
            HIP_TRY(hipMalloc((void **)&x.d_info, (size_t)chunk * k));
            HIP_TRY(hipMalloc((void **)&x.d_cw, (size_t)chunk * n));
            if (!x.d_hard) HIP_TRY(hipMalloc((void **)&x.d_hard, (size_t)chunk * hw * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(x.d_info, 0, (size_t)chunk * k, x.dec.stream()));
            if ((st = fpldpc_encoder_encode(x.enc, x.d_info, chunk, x.d_cw, x.dec.stream()))) return st;
            HIP_TRY(hipStreamSynchronize(x.dec.stream()));
        }
        HIP_TRY(hipMalloc((void **)&d_info_idx, sizeof(int32_t) * k));
        HIP_TRY(hipMemcpy(d_info_idx, s[0].enc->info_index.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice));
        return FPLDPC_OK;
    }
    // harvest: this device's check table, per slot the hard decisions (random_info or not) and the buffers of
    // the scan and the compaction
    int setup_harvest() {
        int st = harvest_upload_table(*hv, &d_table);
        if (st) return st;
        cap = std::min(hv->max_records, chunk);
        row_words = hv->hard_words + hv->syn_words;
        if (sp->codeword && !sp->device_channel) {
            HIP_TRY(hipMalloc((void **)&d_hv_cw, n));
            HIP_TRY(hipMemcpy(d_hv_cw, sp->codeword, n, hipMemcpyHostToDevice));
        }
        for (auto &x : s) {
            HIP_TRY(hipMalloc((void **)&x.d_hard, (size_t)chunk * hv->hard_words * sizeof(uint32_t)));
            const size_t block = ((size_t)chunk * 2 + (size_t)cap * row_words) * sizeof(int32_t);
            HIP_TRY(hipMalloc((void **)&x.d_hv, block));
            HIP_TRY(hipHostMalloc((void **)&x.h_hv, block, hipHostMallocDefault));
            if (cap > 0) {
                HIP_TRY(hipMalloc((void **)&x.d_rows, (size_t)chunk * row_words * sizeof(uint32_t)));
                HIP_TRY(hipMalloc((void **)&x.d_pos, (size_t)chunk * sizeof(int32_t)));
            }
        }
        return FPLDPC_OK;
    }
    // after the chunk's decode, on its stream: scan and compaction, then the one copy the host appends from (the
    // kernels first, so that the stream changes from kernels to copies once per chunk)
    int submit_harvest(Slot &x, hipStream_t st) {
        const int frames = (int)x.frames;
        int32_t *weight = x.d_hv, *unsat = x.d_hv + frames;
        size_t words = (size_t)frames * 2;
        const uint8_t *cw = sp->random_info ? x.d_cw : d_hv_cw ? d_hv_cw : d_cw;
        // once the harvest holds max_records records no later chunk's rows are read: weights only from then on
        uint32_t *rows = cap > 0 && !hv->full.load(std::memory_order_relaxed) ? x.d_rows : nullptr;
        int r = launch_harvest_scan(*hv, d_table, x.d_hard, cw, sp->random_info ? 1 : 0, frames, weight, unsat, rows,
                                    row_words, rows ? rows + hv->hard_words : nullptr, row_words, st);
        if (r) return r;
        if (rows) {
            const int c = std::min(cap, frames);
            if ((r = launch_harvest_compact(weight, rows, row_words, frames, c, x.d_pos, (uint32_t *)(x.d_hv + words), st)))
                return r;
            words += (size_t)c * row_words;
        }
        HIP_TRY(hipMemcpyAsync(x.h_hv, x.d_hv, words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return FPLDPC_OK;
    }
    // Host channel: the chunk's LLRs on host threads (device channel: in submit).
    int generate(Slot &x, plan::Range r) {
        x.first = r.first;
        x.frames = r.frames;
        if (x.frames <= 0 || sp->device_channel) return FPLDPC_OK;
        int st = fpldpc_channel_llr_src_host(source, sp->seed, x.first, (int32_t)x.frames, n, sp->snr, sp->sigma,
                                             sp->frac_bits, sp->codeword, x.h_llr, llr_type(), sp->host_threads);
        if (st) return st;
        if (fl)
            force_host(static_cast<double *>(x.h_llr), x.frames, forced_double());
        else
            force_host(static_cast<int16_t *>(x.h_llr), x.frames, (int16_t)sp->forced_llr);
        return FPLDPC_OK;
    }
    template <typename T>
    void force_host(T *llr, int64_t frames, T value) const {
        for (int64_t f = 0; f < frames; f++)
            for (int i = 0; i < sp->n_forced; i++) llr[(size_t)f * n + sp->forced_index[i]] = value;
    }
    int submit(Slot &x) {
        if (x.frames <= 0) return FPLDPC_OK;
        hipStream_t st = x.dec.stream();
        int r;
        const bool count_bits = sp->count_mode == FPLDPC_COUNT_BITS;
        if (sp->device_channel) {
            int32_t *ovf = fl ? nullptr : x.d_out + 2 * (size_t)chunk;  // float: nothing is quantised
            if (ovf) HIP_TRY(hipMemsetAsync(ovf, 0, sizeof(int32_t), st));
            if (sp->random_info) {  // this chunk's information bits and their codewords, a codeword per frame
                if ((r = fpldpc_info_bits(sp->info_seed, x.first, (int32_t)x.frames, k, x.d_info, st))) return r;
                if ((r = fpldpc_encoder_encode(x.enc, x.d_info, (int32_t)x.frames, x.d_cw, st))) return r;
            }
            if ((r = launch_channel_src(source, sp->seed, x.first, (int)x.frames, n, sp->snr, sp->sigma, sp->frac_bits,
                                        sp->random_info ? x.d_cw : d_cw, sp->random_info ? 1 : 0, x.d_llr, llr_type(),
                                        ovf, st)))
                return r;
            if (bias && (r = launch_bias_patch_src(source, *bias, d_bias_pos, d_bias_shift, sp->seed, x.first, (int)x.frames,
                                                   sp->snr, sp->sigma, sp->frac_bits, sp->random_info ? x.d_cw : d_cw,
                                                   sp->random_info ? 1 : 0, x.d_llr, llr_type(), ovf, x.d_logw, st)))
                return r;
            if (sp->n_forced > 0 &&
                (r = fl ? launch_force_llr_f64(static_cast<double *>(x.d_llr), (int)x.frames, n, d_forced, sp->n_forced,
                                               forced_double(), st)
                        : launch_force_llr(static_cast<int16_t *>(x.d_llr), (int)x.frames, n, d_forced, sp->n_forced,
                                           (int16_t)sp->forced_llr, st)))
                return r;
            if (ovf) HIP_TRY(hipMemcpyAsync(x.h_out + 2 * (size_t)chunk, ovf, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        } else {
            HIP_TRY(hipMemcpyAsync(x.d_llr, x.h_llr, (size_t)x.frames * n * llr_size(), hipMemcpyHostToDevice, st));
        }
        // random_info: the decoder has no reference; its hard decisions are counted against the chunk's own bits
        r = x.dec.decode(x.d_llr, (int32_t)x.frames, sp->random_info || hv ? x.d_hard : nullptr, x.d_out + chunk,
                         count_bits && !sp->random_info ? x.d_out : nullptr, st);
        if (r) return r;
        if (count_bits && sp->random_info &&
            (r = launch_count_info(x.d_hard, (n + 31) / 32, d_info_idx, x.d_info, k, (int)x.frames, x.d_out, st)))
            return r;
        if (hv && (r = submit_harvest(x, st))) return r;
        if (bias) HIP_TRY(hipMemcpyAsync(x.h_logw, x.d_logw, (size_t)x.frames * sizeof(double), hipMemcpyDeviceToHost, st));
        if (count_bits)
            HIP_TRY(hipMemcpyAsync(x.h_out, x.d_out, (size_t)x.frames * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(x.h_out + chunk, x.d_out + chunk, (size_t)x.frames * sizeof(int32_t),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(x.done, st));
        return FPLDPC_OK;
    }
    int wait(Slot &x) {
        if (x.frames <= 0) return FPLDPC_OK;
        HIP_TRY(hipEventSynchronize(x.done));
        if (sp->device_channel && !fl && x.h_out[2 * (size_t)chunk] != 0)
            return fail(FPLDPC_ERR_ARG, "LLR does not fit int16");  // as the host channel
        decoded += x.frames;
        return FPLDPC_OK;
    }
    // blkerror per frame: calculateBER or decode_fixpoint's return value
    const int32_t *blk(const Slot &x) const { return sp->count_mode == FPLDPC_COUNT_BITS ? x.h_out : x.h_out + chunk; }
    const int32_t *its(const Slot &x) const { return x.h_out + chunk; }
};

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

constexpr int kWords = 5;  // exchanged per rank: 4 counters + a status / frames-decoded word

// The exchange between ranks.  Every rank makes the same sequence of calls.  A rank that fails
// anywhere calls abort(): host-mode waiters leave the barrier, and RCCL-mode ranks, which wait for
// their collectives by polling their own stream, abort their own communicator (from their own
// thread, so no communicator is freed under another thread) and return an error.
struct Exchange {
    int ndev = 1;
    Barrier bar{1};
    std::atomic<bool> aborted{false};
    // host mode: double-buffered slots, indexed by call parity (a barrier separates the calls)
    std::vector<int64_t> slots;
    std::vector<int> calls;
    // RCCL mode
    std::vector<ncclComm_t> comms;
    std::vector<int64_t *> dbuf;  // per rank: [kWords] send + [ndev * kWords] receive
    bool rccl = false;
    Exchange(int n, bool use_rccl) : ndev(n), bar(n), slots(2 * (size_t)n * kWords), calls(n, 0), rccl(use_rccl) {}
    ~Exchange() { release(); }
    void release() {
        for (auto *p : dbuf) (void)hipFree(p);
        dbuf.clear();
        for (auto c : comms)  // after a failure, peers may never join a collective: abort, don't destroy
            if (c) (void)(aborted ? ncclCommAbort(c) : ncclCommDestroy(c));
        comms.clear();
    }
    void abort() {
        aborted = true;
        bar.abort();
    }
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
            if (aborted) {
                (void)ncclCommAbort(comms[rank]);
                comms[rank] = nullptr;
                return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed (collective aborted)");
            }
            std::this_thread::yield();
        }
    }
    // all[ndev][kWords] = every rank's `mine`, in rank order
    int allgather(int rank, hipStream_t st, const int64_t *mine, int64_t *all) {
        if (aborted) return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed");
        if (rccl) {
            int64_t *send = dbuf[rank], *recv = dbuf[rank] + kWords;
            HIP_TRY(hipMemcpyAsync(send, mine, sizeof(int64_t) * kWords, hipMemcpyHostToDevice, st));
            ncclResult_t r = ncclAllGather(send, recv, kWords, ncclInt64, comms[rank], st);
            if (r != ncclSuccess) return fail(FPLDPC_ERR_HIP, std::string("ncclAllGather: ") + ncclGetErrorString(r));
            HIP_TRY(hipMemcpyAsync(all, recv, sizeof(int64_t) * kWords * ndev, hipMemcpyDeviceToHost, st));
            return sync(rank, st);
        }
        int64_t *buf = &slots[(size_t)(calls[rank]++ & 1) * ndev * kWords];
        memcpy(buf + (size_t)rank * kWords, mine, sizeof(int64_t) * kWords);
        if (!bar.wait()) return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed");
        memcpy(all, buf, sizeof(int64_t) * kWords * ndev);
        return FPLDPC_OK;
    }
    // sum over ranks of `mine` (kWords)
    int allreduce(int rank, hipStream_t st, const int64_t *mine, int64_t *sum) {
        if (aborted) return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed");
        if (rccl) {
            int64_t *buf = dbuf[rank];
            HIP_TRY(hipMemcpyAsync(buf, mine, sizeof(int64_t) * kWords, hipMemcpyHostToDevice, st));
            ncclResult_t r = ncclAllReduce(buf, buf, kWords, ncclInt64, ncclSum, comms[rank], st);
            if (r != ncclSuccess) return fail(FPLDPC_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
            HIP_TRY(hipMemcpyAsync(sum, buf, sizeof(int64_t) * kWords, hipMemcpyDeviceToHost, st));
            return sync(rank, st);
        }
        std::vector<int64_t> all((size_t)ndev * kWords);
        const int e = allgather(rank, st, mine, all.data());
        if (e) return e;
        for (int w = 0; w < kWords; ++w) {
            sum[w] = 0;
            for (int i = 0; i < ndev; ++i) sum[w] += all[(size_t)i * kWords + w];
        }
        return FPLDPC_OK;
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
    fpldpc_bias_sums wsums{};
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
        if (sp->on_frame || sh.hv || sh.biased) {  // frame order across ranks: rank 0's thread calls back and harvests for everyone
            if (!sh.ex->bar.wait()) return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed");
            if (rank == 0) {
                plan::Sums run = total;
                for (int i = 0; i <= (sr < 0 ? ndev - 1 : sr); ++i) {
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
                        if (sh.biased) {
                            const double lw = xi.h_logw[f], w = exp(lw);
                            const int64_t blk = Ri.blk(xi)[f];
                            const double fe = blk > 0 ? 1.0 : 0.0;
                            fpldpc_bias_sums &b = sh.wsums;
                            ++b.frames;
                            b.frame_errors += blk > 0;
                            b.bit_errors += blk;
                            b.sum_w += w;
                            b.sum_w2 += w * w;
                            b.sum_w_fe += w * fe;
                            b.sum_w2_fe += w * w * fe;
                            b.sum_w_be += w * (double)blk;
                            b.min_logw = std::min(b.min_logw, lw);
                            b.max_logw = std::max(b.max_logw, lw);
                        }
                        run.add_frame(Ri.blk(xi)[f], Ri.its(xi)[f]);
                        if (i == sr && need > 0 && run.frame_errors >= need) break;
                    }
                }
            }
            if (!sh.ex->bar.wait()) return fail(FPLDPC_ERR_HIP, "another rank of the simulation failed");
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

// hv: the harvest to fill; harvesting without one (a *_ber_sim_harvest call with h = NULL) is an error.
// bias: the shift of the channel; a *_ber_sim_biased call (biasing) without one is an error
// source: the noise source (include/fpldpc.h); the entry points without one pass the Lehmer stream
int run_sim(const std::vector<Dec> &dv, const fpldpc_sim_params *sp, int collective, fpldpc_sim_result *out, int32_t *used,
            fpldpc_harvest *hv = nullptr, bool harvesting = false, fpldpc_bias *bias = nullptr, bool biasing = false,
            int source = FPLDPC_NOISE_LEHMER) {
    const int ndev = (int)dv.size();
    if (ndev < 1 || !sp || !out) return fail(FPLDPC_ERR_ARG, "null argument");
    if (source != FPLDPC_NOISE_LEHMER && source != FPLDPC_NOISE_PHILOX)
        return fail(FPLDPC_ERR_ARG, "bad noise source (FPLDPC_NOISE_LEHMER or FPLDPC_NOISE_PHILOX)");
    if (source == FPLDPC_NOISE_PHILOX &&
        (sp->seed < 0 || sp->first_frame < 0 || (sp->max_frames > 0 && sp->first_frame > INT64_MAX - sp->max_frames)))
        return fail(FPLDPC_ERR_ARG, "philox: 0 <= seed and first_frame + max_frames < 2^63");
    if (harvesting && !hv) return fail(FPLDPC_ERR_ARG, "null harvest");
    if (biasing && !bias) return fail(FPLDPC_ERR_ARG, "null bias");
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
    sh.wsums.min_logw = INFINITY;
    sh.wsums.max_logw = -INFINITY;
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
        int st = ranks[i]->setup();
        if (st) return st;
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

// The entry points' handles as Dec (a null handle stays a null Dec; no list at all is an empty one)
Dec from(fpldpc_decoder_t d) {
    Dec x;
    x.flood = d;
    return x;
}
Dec from(fpldpc_layered_t d) {
    Dec x;
    x.lay = d;
    return x;
}
Dec from(fpldpc_minsum_t d) { return from(d ? d->lay : nullptr); }
Dec from_float(fpldpc_decoder_t d) {
    Dec x = from(d);
    x.fl = true;
    return x;
}
template <typename T>
std::vector<Dec> from(const T *decs, int32_t ndev) {
    std::vector<Dec> v;
    for (int i = 0; decs && i < ndev; ++i) v.push_back(from(decs[i]));
    return v;
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

int fpldpc_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return run_sim({from(dec)}, sp, FPLDPC_COLL_HOST, out, nullptr);
}

int fpldpc_ber_sim_multi(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                         fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used);
}

int fpldpc_layered_ber_sim(fpldpc_layered_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return run_sim({from(dec)}, sp, FPLDPC_COLL_HOST, out, nullptr);
}

int fpldpc_layered_ber_sim_multi(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used);
}

int fpldpc_minsum_ber_sim(fpldpc_minsum_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return run_sim({from(dec)}, sp, FPLDPC_COLL_HOST, out, nullptr);
}

int fpldpc_minsum_ber_sim_multi(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                                fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used);
}

int fpldpc_ber_sim_harvest(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                           fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, true);
}

int fpldpc_layered_ber_sim_harvest(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                   int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                   int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, true);
}

int fpldpc_minsum_ber_sim_harvest(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, true);
}

int fpldpc_ber_sim_biased(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, true);
}

int fpldpc_layered_ber_sim_biased(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, true);
}

int fpldpc_minsum_ber_sim_biased(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                 int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, true);
}

int fpldpc_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                          int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, false, source);
}

int fpldpc_layered_ber_sim_source(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                  fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, false, source);
}

int fpldpc_minsum_ber_sim_source(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                 fpldpc_sim_result *out, int32_t *collective_used) {
    return run_sim(from(decs, ndev), sp, collective, out, collective_used, h, false, b, false, source);
}

int fpldpc_float_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return run_sim({from_float(dec)}, sp, FPLDPC_COLL_HOST, out, nullptr);
}

int fpldpc_float_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                fpldpc_sim_result *out, int32_t *collective_used) {
    std::vector<Dec> v;
    for (int i = 0; decs && i < ndev; ++i) v.push_back(from_float(decs[i]));
    return run_sim(v, sp, collective, out, collective_used, h, false, b, false, source);
}

void fpldpc_testing_sim_inject(int32_t fail_rank, int64_t fail_round, int32_t abrupt, int32_t fail_comm_init) {
    g_inject.fail_rank = fail_rank;
    g_inject.fail_round = fail_round;
    g_inject.abrupt = abrupt != 0;
    g_inject.comm_init = fail_comm_init;
}

}  // extern "C"
