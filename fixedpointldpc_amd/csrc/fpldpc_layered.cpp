// fpldpc_layered.cpp -- the layered decoder object and its entry points of the C ABI
// (include/fpldpc.h, fpldpc_layered_*).  Kernels and their choice: fpldpc_layered.hip.
// As with the flooding decoder there is no CPU decode path: without a HIP device creation fails.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "fpldpc_host_plan.hpp"
#include "fpldpc_layered.hpp"

using namespace fpldpc;

namespace {

void free_layered(fpldpc_layered *d) {
    if (!d) return;
    DeviceGuard g(d->device);
    (void)hipFree(d->d_vidx);
    (void)hipFree(d->d_cdeg);
    (void)hipFree(d->d_counter);
    (void)hipFree(d->d_scratch);
    core_free(*d);
    delete d;
}

// The device side of a decoder whose code, parameters, device and choice are set: its tables, counter block,
// scratch and stream (creation and layered_create_twin; on the decoder's device).
int upload(fpldpc_layered *d) {
    const fpldpc_code &c = d->code;
    // slot-major index table in the code's own check order: vidx[k][c] = clist[c][k]; a layer's lanes read
    // consecutive entries (a computed code's kernels read the degrees only)
    const plan::SlotTable t = plan::slot_table(c.m, c.dc_max, c.cdeg.data(), c.clist.data(), c.dc_max, c.m, nullptr, 0);
    HIP_TRY(hipMalloc(&d->d_cdeg, t.cdeg.size()));
    HIP_TRY(hipMemcpy(d->d_cdeg, t.cdeg.data(), t.cdeg.size(), hipMemcpyHostToDevice));
    if (!d->lc.computed) {
        HIP_TRY(hipMalloc(&d->d_vidx, t.vidx.size() * sizeof(uint16_t)));
        HIP_TRY(hipMemcpy(d->d_vidx, t.vidx.data(), t.vidx.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMalloc(&d->d_counter, kLayeredCounterInts * sizeof(int32_t)));  // zero between calls
    HIP_TRY(hipMemset(d->d_counter, 0, kLayeredCounterInts * sizeof(int32_t)));
    if (d->lc.scratch_bytes) HIP_TRY(hipMalloc(&d->d_scratch, d->lc.scratch_bytes));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    return FPLDPC_OK;
}

// The three creation entry points (the arguments of the saturated and the min-sum decoder are validated
// before anything touches HIP).
// kFlood: the flooding min-sum decoder (fpldpc_minsum_create) over the same object; layer_checks unused.
// kFloodSxor: the saturated flooding decoder (fpldpc_flood_create_sat_placed), likewise; scale_16 and offset unused,
// `state` is its state placement (FPLDPC_STATE_*; unused by the other kinds).
enum Kind { kUnsat, kSat, kMinsum, kFlood, kFloodSxor };

int create(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, Kind kind, int32_t post_bits,
           int32_t msg_bits, int32_t scale_16, int32_t offset, fpldpc_layered_t *out, int32_t state = FPLDPC_STATE_LDS) {
    const bool sat = kind == kSat;
    if (!code || !out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_params p;
    int st = resolve_params(params, &p);
    if (st) return st;
    int mode = kLayUnsat;
    if (sat) {
        if (!(2 <= msg_bits && msg_bits < post_bits && post_bits <= 24))
            return fail(FPLDPC_ERR_ARG, "saturated layered decoder: need 2 <= msg_bits < post_bits <= 24");
        // a posterior pinned at S_p minus its own message (at most S_m + C) must keep its sign
        if (sat_limit(post_bits) <= sat_limit(msg_bits) + constant_c(p.frac_bits))
            return fail(FPLDPC_ERR_ARG, "saturated layered decoder: need S_p > S_m + C (2^(post_bits-1) - 1 > 2^(msg_bits-1) - 1 + " +
                                            std::to_string(constant_c(p.frac_bits)) + ")");
        const char *state = getenv("FPLDPC_LAYERED_STATE");  // diagnostic: int32 state where int16 would be chosen
        mode = post_bits <= 16 && !(state && !strcmp(state, "i32")) ? kLaySat16 : kLaySat32;
    }
    if (kind == kMinsum || kind == kFlood) {
        const std::string who = kind == kMinsum ? "layered min-sum decoder" : "flooding min-sum decoder";
        // S_p > S_m keeps the sign of a pinned posterior minus its own message (at most S_m); int16 state
        if (!(2 <= msg_bits && msg_bits < post_bits && post_bits <= 16))
            return fail(FPLDPC_ERR_ARG, who + ": need 2 <= msg_bits < post_bits <= 16");
        if (scale_16 < 1 || scale_16 > 16) return fail(FPLDPC_ERR_ARG, who + ": need 1 <= scale_16 <= 16");
        if (offset < 0 || offset > sat_limit(msg_bits))
            return fail(FPLDPC_ERR_ARG, who + ": need 0 <= offset <= S_m (" + std::to_string(sat_limit(msg_bits)) + ")");
        mode = kind == kMinsum ? kLayMinsum : kFloodMinsum;
    }
    if (kind == kFloodSxor) {
        if (!(2 <= msg_bits && msg_bits < post_bits && post_bits <= 16))
            return fail(FPLDPC_ERR_ARG, "saturated flooding decoder: need 2 <= msg_bits < post_bits <= 16");
        // fpldpc_layered_create_sat's reason: a posterior pinned at S_p minus its own message (at most S_m + C) must
        // keep its sign; S_m + C <= 32767 follows, so the per-edge state is int16
        if (sat_limit(post_bits) <= sat_limit(msg_bits) + constant_c(p.frac_bits))
            return fail(FPLDPC_ERR_ARG, "saturated flooding decoder: need S_p > S_m + C (2^(post_bits-1) - 1 > 2^(msg_bits-1) - 1 + " +
                                            std::to_string(constant_c(p.frac_bits)) + ")");
        if (state != FPLDPC_STATE_LDS && state != FPLDPC_STATE_GLOBAL && state != FPLDPC_STATE_AUTO)
            return fail(FPLDPC_ERR_ARG, "saturated flooding decoder: state " + std::to_string(state) +
                                            " is none of FPLDPC_STATE_LDS (0), FPLDPC_STATE_GLOBAL (1), FPLDPC_STATE_AUTO (2)");
        mode = kFloodSat;
    }
    const bool flooding = kind == kFlood || kind == kFloodSxor;
    int L = code->m, layers = 1;  // flooding: every check of the frame in one step
    st = flooding ? 0 : code_layering(*code, layer_checks, &L, &layers);
    if (st) return st;
    int dev = -1;
    st = select_device(p.device, &dev);
    if (st) return st;
    DeviceGuard g(dev);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");

    std::unique_ptr<fpldpc_layered, void (*)(fpldpc_layered *)> d(new fpldpc_layered(), free_layered);
    d->code = *code;
    d->params = p;
    d->device = dev;
    d->L = L;
    d->layers = layers;
    d->post_bits = kind != kUnsat ? post_bits : 0;
    d->msg_bits = kind != kUnsat ? msg_bits : 0;
    if (kind == kMinsum || kind == kFlood) {
        d->scale_16 = scale_16;
        d->offset = offset;
    }
    st = kind == kFlood       ? flood_minsum_choose(d->code, dev, &d->lc)
         : kind == kFloodSxor ? flood_sat_choose(d->code, dev, state, &d->lc)
         : kind == kMinsum    ? layered_minsum_choose(d->code, L, dev, &d->lc)
                              : layered_choose(d->code, L, dev, mode, &d->lc);
    if (st) return st;
    st = upload(d.get());
    if (st) return st;
    *out = d.release();
    return FPLDPC_OK;
}

// One decode on device buffers and `stream` (on the decoder's device).
int launch(const fpldpc_layered &dec, const DecodeBuffers &b, int32_t llr_type, int32_t batch, void *stream) {
    const fpldpc_code &c = dec.code;
    LayeredArgs a;
    a.llr = b.llr;
    a.llr_i16 = llr_type == FPLDPC_LLR_I16;
    a.n = c.n;
    a.m = c.m;
    a.dc_max = c.dc_max;
    a.L = dec.L;
    a.layers = dec.layers;
    a.array_p = dec.lc.computed ? c.array_p : 0;
    a.table_lds = dec.lc.table_lds;
    a.batch = batch;
    a.max_iter = dec.params.max_iter;
    a.C = constant_c(dec.params.frac_bits);
    a.mask = dec.params.width_mask;
    a.early_term = dec.params.early_term;
    a.precheck = dec.params.precheck;
    a.vidx = dec.d_vidx;
    a.cdeg = dec.d_cdeg;
    a.hard = b.hard;
    a.hard_words = (c.n + 31) / 32;
    a.iters = b.iters;
    a.syn_ok = b.syn_ok;
    a.post = static_cast<int32_t *>(b.post);
    a.bit_errors = b.bit_errors;
    a.totals = reinterpret_cast<unsigned long long *>(b.totals);
    a.info_idx = dec.d_info_idx;
    a.info_bits = dec.d_info_bits;
    a.k_info = dec.k_info;
    a.counters = dec.d_counter;
    a.c2v_scratch = dec.d_scratch;
    if (dec.lc.mode != kLayUnsat) {
        a.sat_post = sat_limit(dec.post_bits);
        a.sat_msg = sat_limit(dec.msg_bits);
    }
    if (dec.lc.mode == kLayMinsum) return layered_minsum_launch(dec.lc, a, dec.scale_16, dec.offset, stream);
    if (dec.lc.mode == kFloodMinsum) return flood_minsum_launch(dec.lc, a, dec.scale_16, dec.offset, stream);
    if (dec.lc.mode == kFloodSat) return flood_sat_launch(dec.lc, a, stream);
    return layered_launch(dec.lc, a, stream);
}

// fpldpc_layered_decode and fpldpc_minsum_decode; ref: the family's set_reference, for the error text.
// stream null: the host form, staged on the decoder's own stream.
int decode(fpldpc_layered_t dec, const char *ref, const DecodeBuffers &b, int32_t llr_type, int32_t batch, void *stream,
           bool host) {
    DeviceGuard g;
    bool run = false;
    const int st = decode_prologue(dec, b.llr, &llr_type, batch, b.bit_errors, ref, &g, &run);
    if (st || !run) return st;
    if (!host) return launch(*dec, b, llr_type, batch, stream);
    return staged_decode(*dec, b, batch, llr_type == FPLDPC_LLR_I16 ? 2 : 4, 4, true,
                         [&](const DecodeBuffers &d, hipStream_t s) { return launch(*dec, d, llr_type, batch, s); });
}

const char kLayeredRef[] = "fpldpc_layered_set_reference", kMinsumRef[] = "fpldpc_minsum_set_reference";

}  // namespace

namespace fpldpc {
int layered_create_twin(fpldpc_layered_t src, fpldpc_layered_t *out) {
    if (!src || !out) return fail(FPLDPC_ERR_ARG, "null decoder");
    DeviceGuard g(src->device);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    std::unique_ptr<fpldpc_layered, void (*)(fpldpc_layered *)> d(new fpldpc_layered(), free_layered);
    d->code = src->code;
    d->params = src->params;
    d->device = src->device;
    d->L = src->L;
    d->layers = src->layers;
    d->post_bits = src->post_bits;
    d->msg_bits = src->msg_bits;
    d->scale_16 = src->scale_16;
    d->offset = src->offset;
    d->lc = src->lc;  // as chosen at src's creation: the environment is not read again
    const int st = upload(d.get());
    if (st) return st;
    *out = d.release();
    return FPLDPC_OK;
}
}  // namespace fpldpc

extern "C" {

int fpldpc_layered_create(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, fpldpc_layered_t *out) {
    return create(code, params, layer_checks, kUnsat, 0, 0, 0, 0, out);
}

int fpldpc_layered_create_sat(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, int32_t post_bits,
                              int32_t msg_bits, fpldpc_layered_t *out) {
    return create(code, params, layer_checks, kSat, post_bits, msg_bits, 0, 0, out);
}

int fpldpc_layered_create_minsum(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, int32_t post_bits,
                                 int32_t msg_bits, int32_t scale_16, int32_t offset, fpldpc_layered_t *out) {
    return create(code, params, layer_checks, kMinsum, post_bits, msg_bits, scale_16, offset, out);
}

int fpldpc_layered_destroy(fpldpc_layered_t dec) {
    free_layered(dec);
    return FPLDPC_OK;
}

int fpldpc_layered_describe(fpldpc_layered_t dec, char *buf, size_t cap) {
    if (!dec || !buf || cap == 0) return fail(FPLDPC_ERR_ARG, "null argument");
    const int w = snprintf(buf, cap, "%s L=%d layers=%d grid=%d threads=%d lds=%zu device=%d", dec->lc.name, dec->L,
                           dec->layers, dec->lc.grid, dec->lc.threads, dec->lc.lds_bytes, dec->device);
    if (dec->lc.mode == kLayMinsum && w > 0 && (size_t)w < cap) {
        const int w2 = snprintf(buf + w, cap - w, " sat=%d/%d ms=%d/16-%d state=compressed", dec->post_bits, dec->msg_bits,
                                dec->scale_16, dec->offset);
        // the global form: the bytes of its scratch
        if (!dec->lc.lds_state && w2 > 0 && (size_t)(w + w2) < cap)
            snprintf(buf + w + w2, cap - w - w2, " scratch=%zu", dec->lc.scratch_bytes);
    } else if (dec->lc.mode != kLayUnsat && w > 0 && (size_t)w < cap) {
        snprintf(buf + w, cap - w, " sat=%d/%d state=%s", dec->post_bits, dec->msg_bits,
                 dec->lc.mode == kLaySat16 ? "i16" : "i32");
    }
    return FPLDPC_OK;
}

int fpldpc_layered_set_reference(fpldpc_layered_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k) {
    return set_reference(dec, info_index, info_bits, k);
}

int fpldpc_layered_decode(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                          int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                          void *stream) {
    return decode(dec, kLayeredRef, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, llr_type, batch, stream, false);
}

int fpldpc_layered_decode_host(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                               int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors,
                               int64_t *totals) {
    return decode(dec, kLayeredRef, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, llr_type, batch, nullptr, true);
}

// The flooding min-sum decoder (fpldpc_minsum_t): the same object in mode kFloodMinsum behind a handle type
// of its own, so that staging, reference bits and the argument struct exist once.  fpldpc_flood_create_sat_placed
// (and fpldpc_flood_create_sat, its FPLDPC_STATE_LDS) makes the same handle in mode kFloodSat (the sxor fold, int16
// c2v per edge).

int fpldpc_minsum_create(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                         int32_t scale_16, int32_t offset, fpldpc_minsum_t *out) {
    if (!out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_layered_t lay = nullptr;
    const int st = create(code, params, 0, kFlood, post_bits, msg_bits, scale_16, offset, &lay);
    if (st) return st;
    *out = new fpldpc_minsum{lay};
    return FPLDPC_OK;
}

int fpldpc_flood_create_sat_placed(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                                   int32_t state, fpldpc_minsum_t *out) {
    if (!out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_layered_t lay = nullptr;
    const int st = create(code, params, 0, kFloodSxor, post_bits, msg_bits, 0, 0, &lay, state);
    if (st) return st;
    *out = new fpldpc_minsum{lay};
    return FPLDPC_OK;
}

int fpldpc_flood_create_sat(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                            fpldpc_minsum_t *out) {
    return fpldpc_flood_create_sat_placed(code, params, post_bits, msg_bits, FPLDPC_STATE_LDS, out);
}

int fpldpc_minsum_destroy(fpldpc_minsum_t dec) {
    if (!dec) return FPLDPC_OK;
    free_layered(dec->lay);
    delete dec;
    return FPLDPC_OK;
}

int fpldpc_minsum_describe(fpldpc_minsum_t dec, char *buf, size_t cap) {
    if (!dec || !buf || cap == 0) return fail(FPLDPC_ERR_ARG, "null argument");
    const fpldpc_layered *d = dec->lay;
    if (d->lc.mode == kFloodSat) {
        const int w = snprintf(buf, cap, "%s grid=%d threads=%d lds=%zu device=%d sat=%d/%d state=i16", d->lc.name, d->lc.grid,
                               d->lc.threads, d->lc.lds_bytes, d->device, d->post_bits, d->msg_bits);
        // the global form: the bytes of its scratch
        if (!d->lc.lds_state && w > 0 && (size_t)w < cap) snprintf(buf + w, cap - w, " scratch=%zu", d->lc.scratch_bytes);
        return FPLDPC_OK;
    }
    const int w = snprintf(buf, cap, "%s grid=%d threads=%d lds=%zu device=%d sat=%d/%d ms=%d/16-%d state=compressed",
                           d->lc.name, d->lc.grid, d->lc.threads, d->lc.lds_bytes, d->device, d->post_bits, d->msg_bits,
                           d->scale_16, d->offset);
    // the global form: the bytes of its scratch
    if (!d->lc.lds_state && w > 0 && (size_t)w < cap) snprintf(buf + w, cap - w, " scratch=%zu", d->lc.scratch_bytes);
    return FPLDPC_OK;
}

int fpldpc_minsum_set_reference(fpldpc_minsum_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k) {
    return set_reference(dec ? dec->lay : nullptr, info_index, info_bits, k);
}

int fpldpc_minsum_decode(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                         int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                         void *stream) {
    return decode(dec ? dec->lay : nullptr, kMinsumRef, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, llr_type,
                  batch, stream, false);
}

int fpldpc_minsum_decode_host(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                              int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals) {
    return decode(dec ? dec->lay : nullptr, kMinsumRef, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, llr_type,
                  batch, nullptr, true);
}

}  // extern "C"
