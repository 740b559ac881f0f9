// fpldpc_layered.cpp -- the layered decoder object and its entry points of the C ABI
// (include/fpldpc.h, fpldpc_layered_*).  Kernels and their choice: fpldpc_layered.hip.
// As with the flooding decoder there is no CPU decode path: without a HIP device creation fails.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "fpldpc_layered.hpp"

using namespace fpldpc;

namespace {

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (dev >= 0 && dev != prev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

#define HIP_TRY(expr)                                             \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return fail_hip((int)_e, #expr);    \
    } while (0)

void free_layered(fpldpc_layered *d) {
    if (!d) return;
    DeviceGuard g(d->device);
    (void)hipFree(d->d_vidx);
    (void)hipFree(d->d_cdeg);
    (void)hipFree(d->d_counter);
    (void)hipFree(d->d_scratch);
    (void)hipFree(d->d_info_idx);
    (void)hipFree(d->d_info_bits);
    (void)hipFree(d->d_stage);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

// The device side of a decoder whose code, parameters, device and choice are set: its tables, counter block,
// scratch and stream (creation and layered_create_twin; on the decoder's device).
int upload(fpldpc_layered *d) {
    const fpldpc_code &c = d->code;
    std::vector<uint8_t> cdeg(c.m);
    for (int r = 0; r < c.m; r++) cdeg[r] = (uint8_t)c.cdeg[r];
    HIP_TRY(hipMalloc(&d->d_cdeg, cdeg.size()));
    HIP_TRY(hipMemcpy(d->d_cdeg, cdeg.data(), cdeg.size(), hipMemcpyHostToDevice));
    if (!d->lc.computed) {
        // slot-major index table in the code's own check order: vidx[k][c] = clist[c][k]; a layer's
        // lanes read consecutive entries
        std::vector<uint16_t> vidx((size_t)c.dc_max * c.m, 0);
        for (int r = 0; r < c.m; r++)
            for (int k = 0; k < c.cdeg[r]; k++) vidx[(size_t)k * c.m + r] = (uint16_t)c.clist[(size_t)r * c.dc_max + k];
        HIP_TRY(hipMalloc(&d->d_vidx, vidx.size() * sizeof(uint16_t)));
        HIP_TRY(hipMemcpy(d->d_vidx, vidx.data(), vidx.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMalloc(&d->d_counter, kLayeredCounterInts * sizeof(int32_t)));  // zero between calls
    HIP_TRY(hipMemset(d->d_counter, 0, kLayeredCounterInts * sizeof(int32_t)));
    if (d->lc.scratch_bytes) HIP_TRY(hipMalloc(&d->d_scratch, d->lc.scratch_bytes));
    HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    return FPLDPC_OK;
}

// Constant = int((5.0/8.0) * (1 << FRAC_WIDTH)) (ArrayLDPCMacro.h:175)
int constant_c(int frac_bits) { return (int)((5.0 / 8.0) * (1 << frac_bits)); }

int sat_limit(int bits) { return (1 << (bits - 1)) - 1; }

// The three creation entry points (the arguments of the saturated and the min-sum decoder are validated
// before anything touches HIP).
// kFlood: the flooding min-sum decoder (fpldpc_minsum_create) over the same object; layer_checks unused.
enum Kind { kUnsat, kSat, kMinsum, kFlood };

int create(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, Kind kind, int32_t post_bits,
           int32_t msg_bits, int32_t scale_16, int32_t offset, fpldpc_layered_t *out) {
    const bool sat = kind == kSat;
    if (!code || !out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_params p;
    fpldpc_params_default(&p);
    if (params) p = *params;
    if (p.max_iter < 1 || p.max_iter > 100000) return fail(FPLDPC_ERR_ARG, "max_iter out of range (1..100000)");
    if (p.frac_bits < 0 || p.frac_bits > 16) return fail(FPLDPC_ERR_ARG, "frac_bits out of range");
    if (p.width_mask <= 0) return fail(FPLDPC_ERR_ARG, "width_mask must be positive");
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
    int L = code->m, layers = 1;  // flooding: every check of the frame in one step
    int st = kind == kFlood ? 0 : code_layering(*code, layer_checks, &L, &layers);
    if (st) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FPLDPC_ERR_HIP, "no HIP device available (the decoder has no CPU path)");
    int dev = p.device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= ndev) return fail(FPLDPC_ERR_ARG, "device ordinal out of range");
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
    st = kind == kFlood    ? flood_minsum_choose(d->code, dev, &d->lc)
         : kind == kMinsum ? layered_minsum_choose(d->code, L, dev, &d->lc)
                           : layered_choose(d->code, L, dev, mode, &d->lc);
    if (st) return st;
    st = upload(d.get());
    if (st) return st;
    *out = d.release();
    return FPLDPC_OK;
}

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
    if (!dec || k < 0 || (k > 0 && (!info_index || !info_bits))) return fail(FPLDPC_ERR_ARG, "bad reference");
    for (int i = 0; i < k; i++)
        if (info_index[i] < 0 || info_index[i] >= dec->code.n) return fail(FPLDPC_ERR_ARG, "info index out of range");
    DeviceGuard g(dec->device);
    (void)hipFree(dec->d_info_idx);
    (void)hipFree(dec->d_info_bits);
    dec->d_info_idx = nullptr;
    dec->d_info_bits = nullptr;
    dec->k_info = 0;
    if (k == 0) return FPLDPC_OK;
    std::vector<uint8_t> bits(info_bits, info_bits + k);
    for (auto &b : bits) b &= 1;
    HIP_TRY(hipMalloc(&dec->d_info_idx, sizeof(int32_t) * k));
    HIP_TRY(hipMalloc(&dec->d_info_bits, k));
    HIP_TRY(hipMemcpy(dec->d_info_idx, info_index, sizeof(int32_t) * k, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dec->d_info_bits, bits.data(), k, hipMemcpyHostToDevice));
    dec->k_info = k;
    return FPLDPC_OK;
}

int fpldpc_layered_decode(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                          int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                          void *stream) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (batch < 0) return fail(FPLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return FPLDPC_OK;
    if (!llr) return fail(FPLDPC_ERR_ARG, "null llr");
    if (llr_type != FPLDPC_LLR_I32 && llr_type != FPLDPC_LLR_I16) return fail(FPLDPC_ERR_ARG, "bad llr_type");
    if (bit_errors && dec->k_info == 0)
        return fail(FPLDPC_ERR_ARG, "bit_errors requested without fpldpc_layered_set_reference");
    DeviceGuard g(dec->device);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    const fpldpc_code &c = dec->code;
    LayeredArgs a;
    a.llr = llr;
    a.llr_i16 = llr_type == FPLDPC_LLR_I16;
    a.n = c.n;
    a.m = c.m;
    a.dc_max = c.dc_max;
    a.L = dec->L;
    a.layers = dec->layers;
    a.array_p = dec->lc.computed ? c.array_p : 0;
    a.table_lds = dec->lc.table_lds;
    a.batch = batch;
    a.max_iter = dec->params.max_iter;
    a.C = constant_c(dec->params.frac_bits);
    a.mask = dec->params.width_mask;
    a.early_term = dec->params.early_term;
    a.precheck = dec->params.precheck;
    a.vidx = dec->d_vidx;
    a.cdeg = dec->d_cdeg;
    a.hard = hard;
    a.hard_words = (c.n + 31) / 32;
    a.iters = iters;
    a.syn_ok = syndrome_ok;
    a.post = post;
    a.bit_errors = bit_errors;
    a.totals = reinterpret_cast<unsigned long long *>(totals);
    a.info_idx = dec->d_info_idx;
    a.info_bits = dec->d_info_bits;
    a.k_info = dec->k_info;
    a.counters = dec->d_counter;
    a.c2v_scratch = dec->d_scratch;
    if (dec->lc.mode != kLayUnsat) {
        a.sat_post = sat_limit(dec->post_bits);
        a.sat_msg = sat_limit(dec->msg_bits);
    }
    if (dec->lc.mode == kLayMinsum) return layered_minsum_launch(dec->lc, a, dec->scale_16, dec->offset, stream);
    if (dec->lc.mode == kFloodMinsum) return flood_minsum_launch(dec->lc, a, dec->scale_16, dec->offset, stream);
    return layered_launch(dec->lc, a, stream);
}

int fpldpc_layered_decode_host(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                               int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors,
                               int64_t *totals) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (batch < 0) return fail(FPLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return FPLDPC_OK;
    if (!llr) return fail(FPLDPC_ERR_ARG, "null llr");
    if (llr_type != FPLDPC_LLR_I32 && llr_type != FPLDPC_LLR_I16) return fail(FPLDPC_ERR_ARG, "bad llr_type");
    DeviceGuard g(dec->device);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    const size_t n = dec->code.n, hw = (n + 31) / 32, B = batch;
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t llr_raw = B * n * (llr_type == FPLDPC_LLR_I16 ? 2 : 4);
    const size_t llr_b = align(llr_raw), hard_b = align(B * hw * 4), it_b = align(B * 4), ok_b = align(B),
                 post_b = align(B * n * 4), be_b = align(B * 4), tot_b = align(32);
    const size_t need = llr_b + hard_b + it_b + ok_b + post_b + be_b + tot_b;
    if (need > dec->stage_bytes) {
        (void)hipFree(dec->d_stage);
        dec->d_stage = nullptr;
        dec->stage_bytes = 0;
        HIP_TRY(hipMalloc(&dec->d_stage, need));
        dec->stage_bytes = need;
    }
    char *p = static_cast<char *>(dec->d_stage);
    void *d_llr = p;
    p += llr_b;
    uint32_t *d_hard = hard ? reinterpret_cast<uint32_t *>(p) : nullptr;
    p += hard_b;
    int32_t *d_it = iters ? reinterpret_cast<int32_t *>(p) : nullptr;
    p += it_b;
    uint8_t *d_ok = syndrome_ok ? reinterpret_cast<uint8_t *>(p) : nullptr;
    p += ok_b;
    int32_t *d_post = post ? reinterpret_cast<int32_t *>(p) : nullptr;
    p += post_b;
    int32_t *d_be = bit_errors ? reinterpret_cast<int32_t *>(p) : nullptr;
    p += be_b;
    int64_t *d_tot = totals ? reinterpret_cast<int64_t *>(p) : nullptr;
    hipStream_t s = dec->stream;
    HIP_TRY(hipMemcpyAsync(d_llr, llr, llr_raw, hipMemcpyHostToDevice, s));
    // posteriors are left untouched on a pre-check pass: seed the device copy with the caller's buffer
    if (d_post) HIP_TRY(hipMemcpyAsync(d_post, post, B * n * 4, hipMemcpyHostToDevice, s));
    if (d_tot) HIP_TRY(hipMemcpyAsync(d_tot, totals, 32, hipMemcpyHostToDevice, s));
    int st = fpldpc_layered_decode(dec, d_llr, llr_type, batch, d_hard, d_it, d_ok, d_post, d_be, d_tot, s);
    if (st) return st;
    if (d_hard) HIP_TRY(hipMemcpyAsync(hard, d_hard, B * hw * 4, hipMemcpyDeviceToHost, s));
    if (d_it) HIP_TRY(hipMemcpyAsync(iters, d_it, B * 4, hipMemcpyDeviceToHost, s));
    if (d_ok) HIP_TRY(hipMemcpyAsync(syndrome_ok, d_ok, B, hipMemcpyDeviceToHost, s));
    if (d_post) HIP_TRY(hipMemcpyAsync(post, d_post, B * n * 4, hipMemcpyDeviceToHost, s));
    if (d_be) HIP_TRY(hipMemcpyAsync(bit_errors, d_be, B * 4, hipMemcpyDeviceToHost, s));
    if (d_tot) HIP_TRY(hipMemcpyAsync(totals, d_tot, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FPLDPC_OK;
}

// The flooding min-sum decoder (fpldpc_minsum_t): the same object in mode kFloodMinsum behind a handle type
// of its own, so that staging, reference bits and the argument struct exist once.

int fpldpc_minsum_create(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                         int32_t scale_16, int32_t offset, fpldpc_minsum_t *out) {
    if (!out) return fail(FPLDPC_ERR_ARG, "null argument");
    fpldpc_layered_t lay = nullptr;
    const int st = create(code, params, 0, kFlood, post_bits, msg_bits, scale_16, offset, &lay);
    if (st) return st;
    *out = new fpldpc_minsum{lay};
    return FPLDPC_OK;
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
    const int w = snprintf(buf, cap, "%s grid=%d threads=%d lds=%zu device=%d sat=%d/%d ms=%d/16-%d state=compressed",
                           d->lc.name, d->lc.grid, d->lc.threads, d->lc.lds_bytes, d->device, d->post_bits, d->msg_bits,
                           d->scale_16, d->offset);
    // the global form: the bytes of its scratch
    if (!d->lc.lds_state && w > 0 && (size_t)w < cap) snprintf(buf + w, cap - w, " scratch=%zu", d->lc.scratch_bytes);
    return FPLDPC_OK;
}

int fpldpc_minsum_set_reference(fpldpc_minsum_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "bad reference");
    return fpldpc_layered_set_reference(dec->lay, info_index, info_bits, k);
}

int fpldpc_minsum_decode(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                         int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                         void *stream) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (bit_errors && dec->lay->k_info == 0)
        return fail(FPLDPC_ERR_ARG, "bit_errors requested without fpldpc_minsum_set_reference");
    return fpldpc_layered_decode(dec->lay, llr, llr_type, batch, hard, iters, syndrome_ok, post, bit_errors, totals, stream);
}

int fpldpc_minsum_decode_host(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                              int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (bit_errors && dec->lay->k_info == 0)
        return fail(FPLDPC_ERR_ARG, "bit_errors requested without fpldpc_minsum_set_reference");
    return fpldpc_layered_decode_host(dec->lay, llr, llr_type, batch, hard, iters, syndrome_ok, post, bit_errors, totals);
}

}  // extern "C"
