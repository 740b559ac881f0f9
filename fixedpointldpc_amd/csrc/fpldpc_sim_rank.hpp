// fpldpc_sim_rank.hpp -- one rank of a simulation (fpldpc_sim.cpp): a decoder, its device, and the chunk pipeline of
// setup, generate, submit, wait and the harvest submit.
//
// Each rank (one decoder, one device, one host thread) holds two pinned / device buffer pairs on its decoder's
// stream, so that the host generates the next chunk's LLRs while the GPU decodes this one (or, with
// device_channel, the LLRs are generated on the device in the same stream, fpldpc_gen.hip).
//
// Two chunks in flight per rank: the two slots decode on two decoders (the caller's and a twin with
// the same code and parameters) on their own streams, and round r+1's chunk is submitted before
// round r's is waited for, so the next chunk's workgroups take the CUs that a chunk's last frames
// leave idle (with early termination a chunk ends on a few frames running max_iter iterations
// alone).  The exchange runs on a third stream.
//
// random_info: each chunk's frames carry fresh information bits (fpldpc_sim_source.hip), encoded and sent
// through the device channel with a codeword per frame, and the decode's hard decisions are counted against
// them, all on the slot's stream (include/fpldpc.h); rounds, exchange and stop rule do not know of it.
//
// Harvest (fpldpc_harvest.hip): each chunk's decode writes its hard decisions, and on the slot's stream, before its
// `done` event, the scan kernel gives every frame's (weight, unsat) and err / syn row, the ordered compaction
// gathers the codeword-error frames' rows behind the pairs, and one copy takes both to pinned memory.  Without a
// harvest none of this exists.
//
// Bias (fpldpc_bias.hip): each slot has the chunk's log-weights on the device and a pinned twin.  The patch kernel
// follows the slot's channel launch, before the forced positions are written; the copy goes with the slot's other
// copies, before `done`.  Without a bias none of this exists.
//
// Source (fpldpc_source.hip): the three places that make noise -- generate, the slot's channel launch and its patch
// launch -- take the noise source; a chunk's channel arguments are built once (chunk_args) and handed to both
// launches.
//
// Float: the same pipeline around fpldpc_decode_float.  The channel -- host or device, either source, the patch
// kernel included -- writes FPLDPC_LLR_F64 into slots of 8 bytes per value, the forced positions receive the double
// forced_llr * 2^-frac_bits (fpldpc_sim_source.hip), and there is no int16 overflow word to zero, copy or test.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fpldpc_bias.hpp"
#include "fpldpc_channel_args.hpp"
#include "fpldpc_harvest.hpp"
#include "fpldpc_internal.hpp"
#include "fpldpc_layered.hpp"
#include "fpldpc_sim_plan.hpp"
#include "fpldpc_sim_source.hpp"
#include "fpldpc_source.hpp"

namespace fpldpc {

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

// A buffer that a rank or a slot owns: device memory (Free = hipFree) or pinned host memory (hipHostFree), allocated
// into p, read as the pointer it holds, freed with its owner.
template <typename T, hipError_t (*Free)(void *)>
struct Buf {
    T *p = nullptr;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { (void)Free(p); }
    operator T *() const { return p; }
};
template <typename T>
using DevBuf = Buf<T, hipFree>;
template <typename T>
using PinBuf = Buf<T, hipHostFree>;

struct Slot {
    PinBuf<void> h_llr;     // int16 [chunk][n]; float: double
    PinBuf<int32_t> h_out;  // [chunk] bit errors, [chunk] iterations, [1] int16 overflow count
    DevBuf<void> d_llr;
    DevBuf<int32_t> d_out;
    hipEvent_t done = nullptr;
    int64_t frames = 0;
    int64_t first = 0;
    Dec dec;  // decodes this slot's chunks, on its own stream
    // random_info: the chunk's information bits [chunk][k], codewords [chunk][n] and hard decisions
    // [chunk][hard words], and this stream's encoder (an encoder is single-stream)
    DevBuf<uint8_t> d_info, d_cw;
    DevBuf<uint32_t> d_hard;
    fpldpc_encoder_t enc = nullptr;
    // harvest: one block on the device and its pinned twin, copied once per chunk -- weight [frames], unsat
    // [frames], then the compaction's records [min(cap, frames)][row words]; every frame's err | syn row
    // [chunk][row words] and the compaction's scratch [chunk] stay on the device
    DevBuf<int32_t> d_hv, d_pos;
    PinBuf<int32_t> h_hv;
    DevBuf<uint32_t> d_rows;
    // bias: the chunk's log-weights [chunk] and their pinned twin
    DevBuf<double> d_logw;
    PinBuf<double> h_logw;
    ~Slot() {
        if (enc) fpldpc_encoder_free(enc);
        if (done) (void)hipEventDestroy(done);
    }
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
    DevBuf<int32_t> d_forced;       // the forced positions and, behind them, the device channel's fixed codeword
    const uint8_t *d_cw = nullptr;  // that codeword [n], inside d_forced's allocation
    DevBuf<int32_t> d_info_idx;     // random_info: the encoder's info positions [k]
    int k = 0;
    int64_t decoded = 0;
    fpldpc_harvest *hv = nullptr;  // harvest: the object to fill (rank 0's thread does), or null
    DevBuf<uint16_t> d_table;      // this device's copy of its check table
    DevBuf<uint8_t> d_hv_cw;       // the fixed codeword [n] on the device where the host channel keeps it on the host
    int cap = 0, row_words = 0;    // records per chunk buffer, words per record row (err | syn)
    const fpldpc_bias *bias = nullptr;  // bias: the shift of this simulation's channel, or null
    DevBuf<int32_t> d_bias_pos;         // this device's copy of its positions and shifts
    DevBuf<double> d_bias_shift;
    int source = FPLDPC_NOISE_LEHMER;  // the noise source of generate, launch_channel and launch_bias_patch
    bool fl = false;                   // float: the slots hold doubles
    int llr_type() const { return fl ? FPLDPC_LLR_F64 : FPLDPC_LLR_I16; }
    size_t llr_size() const { return fl ? sizeof(double) : sizeof(int16_t); }
    double forced_double() const { return std::ldexp((double)sp->forced_llr, -sp->frac_bits); }
    ~Rank() {
        // a rank that left early (an error) may still have a chunk in flight: let it finish before
        // the twin decoder and, with the members, the buffers go
        for (auto &x : s)
            if (x.dec) (void)hipStreamSynchronize(x.dec.stream());
        twin.destroy();
        if (xs) (void)hipStreamDestroy(xs);
    }
    hipStream_t exchange_stream() const { return xs ? xs : dec.stream(); }
    int setup() {  // on the decoder's device
        const size_t llr_bytes = (size_t)chunk * n * llr_size();
        s[0].dec = s[1].dec = dec;
        if (overlap) {
            if (const int st = dec.create_twin(&twin)) return st;
            s[1].dec = twin;
            HIP_TRY(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking));
        }
        for (auto &x : s) {
            if (!sp->device_channel) HIP_TRY(hipHostMalloc(&x.h_llr.p, llr_bytes, hipHostMallocDefault));
            HIP_TRY(hipHostMalloc((void **)&x.h_out.p, ((size_t)chunk * 2 + 1) * sizeof(int32_t), hipHostMallocDefault));
            HIP_TRY(hipMalloc(&x.d_llr.p, llr_bytes));
            HIP_TRY(hipMalloc((void **)&x.d_out.p, ((size_t)chunk * 2 + 1) * sizeof(int32_t)));
            HIP_TRY(hipEventCreateWithFlags(&x.done, hipEventDisableTiming));
        }
        if (sp->device_channel) {
            if (sp->codeword) {
                HIP_TRY(hipMalloc((void **)&d_forced.p, sizeof(int32_t) * std::max(sp->n_forced, 0) + n));
                d_cw = reinterpret_cast<const uint8_t *>(d_forced + std::max(sp->n_forced, 0));
                HIP_TRY(hipMemcpy((void *)d_cw, sp->codeword, n, hipMemcpyHostToDevice));
            } else if (sp->n_forced > 0) {
                HIP_TRY(hipMalloc((void **)&d_forced.p, sizeof(int32_t) * sp->n_forced));
            }
            if (sp->n_forced > 0)
                HIP_TRY(hipMemcpy(d_forced, sp->forced_index, sizeof(int32_t) * sp->n_forced, hipMemcpyHostToDevice));
        }
        if (const int st = hv ? setup_harvest() : FPLDPC_OK) return st;
        if (bias) {
            if (const int st = bias_upload_tables(*bias, &d_bias_pos.p, &d_bias_shift.p)) return st;
            for (auto &x : s) {
                HIP_TRY(hipMalloc((void **)&x.d_logw.p, (size_t)chunk * sizeof(double)));
                HIP_TRY(hipHostMalloc((void **)&x.h_logw.p, (size_t)chunk * sizeof(double), hipHostMallocDefault));
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
            HIP_TRY(hipMalloc((void **)&x.d_info.p, (size_t)chunk * k));
            HIP_TRY(hipMalloc((void **)&x.d_cw.p, (size_t)chunk * n));
            if (!x.d_hard) HIP_TRY(hipMalloc((void **)&x.d_hard.p, (size_t)chunk * hw * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(x.d_info, 0, (size_t)chunk * k, x.dec.stream()));
            if ((st = fpldpc_encoder_encode(x.enc, x.d_info, chunk, x.d_cw, x.dec.stream()))) return st;
            HIP_TRY(hipStreamSynchronize(x.dec.stream()));
        }
        HIP_TRY(hipMalloc((void **)&d_info_idx.p, sizeof(int32_t) * k));
        HIP_TRY(hipMemcpy(d_info_idx, s[0].enc->info_index.data(), sizeof(int32_t) * k, hipMemcpyHostToDevice));
        return FPLDPC_OK;
    }
    // harvest: this device's check table, per slot the hard decisions (random_info or not) and the buffers of
    // the scan and the compaction
    int setup_harvest() {
        if (const int st = harvest_upload_table(*hv, &d_table.p)) return st;
        cap = std::min(hv->max_records, chunk);
        row_words = hv->hard_words + hv->syn_words;
        if (sp->codeword && !sp->device_channel) {
            HIP_TRY(hipMalloc((void **)&d_hv_cw.p, n));
            HIP_TRY(hipMemcpy(d_hv_cw, sp->codeword, n, hipMemcpyHostToDevice));
        }
        for (auto &x : s) {
            HIP_TRY(hipMalloc((void **)&x.d_hard.p, (size_t)chunk * hv->hard_words * sizeof(uint32_t)));
            const size_t block = ((size_t)chunk * 2 + (size_t)cap * row_words) * sizeof(int32_t);
            HIP_TRY(hipMalloc((void **)&x.d_hv.p, block));
            HIP_TRY(hipHostMalloc((void **)&x.h_hv.p, block, hipHostMallocDefault));
            if (cap > 0) {
                HIP_TRY(hipMalloc((void **)&x.d_rows.p, (size_t)chunk * row_words * sizeof(uint32_t)));
                HIP_TRY(hipMalloc((void **)&x.d_pos.p, (size_t)chunk * sizeof(int32_t)));
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
        const uint8_t *cw = sp->random_info ? x.d_cw.p : d_hv_cw ? d_hv_cw.p : d_cw;
        // once the harvest holds max_records records no later chunk's rows are read: weights only from then on
        uint32_t *rows = cap > 0 && !hv->full.load(std::memory_order_relaxed) ? x.d_rows.p : nullptr;
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
            force_host(static_cast<double *>(x.h_llr.p), x.frames, forced_double());
        else
            force_host(static_cast<int16_t *>(x.h_llr.p), x.frames, (int16_t)sp->forced_llr);
        return FPLDPC_OK;
    }
    template <typename T>
    void force_host(T *llr, int64_t frames, T value) const {
        for (int64_t f = 0; f < frames; f++)
            for (int i = 0; i < sp->n_forced; i++) llr[(size_t)f * n + sp->forced_index[i]] = value;
    }
    // The device channel's arguments for the slot's chunk: random_info sends the chunk's own codewords, one per frame
    ChannelArgs chunk_args(const Slot &x, int32_t *overflow) const {
        return {sp->seed, x.first, (int)x.frames, n, sp->snr, sp->sigma, sp->frac_bits, sp->random_info ? x.d_cw.p : d_cw,
                sp->random_info ? 1 : 0, x.d_llr, llr_type(), overflow, x.d_logw};
    }
    int submit(Slot &x) {
        if (x.frames <= 0) return FPLDPC_OK;
        hipStream_t st = x.dec.stream();
        int r;
        const bool count_bits = sp->count_mode == FPLDPC_COUNT_BITS;
        if (sp->device_channel) {
            // float: nothing is quantised, so there is no overflow word
            const ChannelArgs a = chunk_args(x, fl ? nullptr : x.d_out + 2 * (size_t)chunk);
            if (a.overflow) HIP_TRY(hipMemsetAsync(a.overflow, 0, sizeof(int32_t), st));
            if (sp->random_info) {  // this chunk's information bits and their codewords, a codeword per frame
                if ((r = fpldpc_info_bits(sp->info_seed, x.first, (int32_t)x.frames, k, x.d_info, st))) return r;
                if ((r = fpldpc_encoder_encode(x.enc, x.d_info, (int32_t)x.frames, x.d_cw, st))) return r;
            }
            if ((r = launch_channel_src(source, a, st))) return r;
            if (bias && (r = launch_bias_patch_src(source, *bias, d_bias_pos, d_bias_shift, a, st))) return r;
            if (sp->n_forced > 0 &&
                (r = fl ? launch_force_llr_f64(static_cast<double *>(x.d_llr.p), (int)x.frames, n, d_forced, sp->n_forced,
                                               forced_double(), st)
                        : launch_force_llr(static_cast<int16_t *>(x.d_llr.p), (int)x.frames, n, d_forced, sp->n_forced,
                                           (int16_t)sp->forced_llr, st)))
                return r;
            if (a.overflow)
                HIP_TRY(hipMemcpyAsync(x.h_out + 2 * (size_t)chunk, a.overflow, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        } else {
            HIP_TRY(hipMemcpyAsync(x.d_llr, x.h_llr, (size_t)x.frames * n * llr_size(), hipMemcpyHostToDevice, st));
        }
        // random_info: the decoder has no reference; its hard decisions are counted against the chunk's own bits
        r = x.dec.decode(x.d_llr, (int32_t)x.frames, sp->random_info || hv ? x.d_hard.p : nullptr, x.d_out + chunk,
                         count_bits && !sp->random_info ? x.d_out.p : nullptr, st);
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

}  // namespace fpldpc
