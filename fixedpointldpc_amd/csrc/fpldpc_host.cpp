// fpldpc_host.cpp -- the host plumbing every decoder object shares (fpldpc_host.hpp).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fpldpc_host.hpp"
#include "fpldpc_host_plan.hpp"

namespace fpldpc {

int resolve_params(const fpldpc_params *params, fpldpc_params *p) {
    fpldpc_params_default(p);
    if (params) *p = *params;
    if (p->max_iter < 1 || p->max_iter > 100000) return fail(FPLDPC_ERR_ARG, "max_iter out of range (1..100000)");
    if (p->frac_bits < 0 || p->frac_bits > 16) return fail(FPLDPC_ERR_ARG, "frac_bits out of range");
    if (p->width_mask <= 0) return fail(FPLDPC_ERR_ARG, "width_mask must be positive");
    return FPLDPC_OK;
}

int select_device(int requested, int *dev) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FPLDPC_ERR_HIP, "no HIP device available (the decoder has no CPU path)");
    *dev = requested;
    if (*dev < 0) HIP_TRY(hipGetDevice(dev));
    if (*dev >= ndev) return fail(FPLDPC_ERR_ARG, "device ordinal out of range");
    return FPLDPC_OK;
}

void core_free(DecoderCore &core) {
    (void)hipFree(core.d_info_idx);
    (void)hipFree(core.d_info_bits);
    (void)hipFree(core.d_stage);
    if (core.stream) (void)hipStreamDestroy(core.stream);
}

int set_reference(DecoderCore *core, const int32_t *info_index, const uint8_t *info_bits, int32_t k) {
    if (!core || k < 0 || (k > 0 && (!info_index || !info_bits))) return fail(FPLDPC_ERR_ARG, "bad reference");
    for (int i = 0; i < k; i++)
        if (info_index[i] < 0 || info_index[i] >= core->code.n) return fail(FPLDPC_ERR_ARG, "info index out of range");
    DeviceGuard g(core->device);
    (void)hipFree(core->d_info_idx);
    (void)hipFree(core->d_info_bits);
    core->d_info_idx = nullptr;
    core->d_info_bits = nullptr;
    core->k_info = 0;
    if (k == 0) return FPLDPC_OK;
    std::vector<uint8_t> bits(info_bits, info_bits + k);
    for (auto &b : bits) b &= 1;
    HIP_TRY(hipMalloc(&core->d_info_idx, sizeof(int32_t) * k));
    HIP_TRY(hipMalloc(&core->d_info_bits, k));
    HIP_TRY(hipMemcpy(core->d_info_idx, info_index, sizeof(int32_t) * k, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(core->d_info_bits, bits.data(), k, hipMemcpyHostToDevice));
    core->k_info = k;
    return FPLDPC_OK;
}

int decode_prologue(const DecoderCore *core, const void *llr, const int32_t *llr_type, int32_t batch,
                    const int32_t *bit_errors, const char *set_reference_name, DeviceGuard *g, bool *run) {
    *run = false;
    if (!core) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (batch < 0) return fail(FPLDPC_ERR_ARG, "negative batch");
    if (batch == 0) return FPLDPC_OK;  // an empty batch needs no buffers
    if (!llr) return fail(FPLDPC_ERR_ARG, "null llr");
    if (llr_type && *llr_type != FPLDPC_LLR_I32 && *llr_type != FPLDPC_LLR_I16) return fail(FPLDPC_ERR_ARG, "bad llr_type");
    if (bit_errors && core->k_info == 0)
        return fail(FPLDPC_ERR_ARG, std::string("bit_errors requested without ") + set_reference_name);
    g->enter(core->device);
    if (!g->ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    *run = true;
    return FPLDPC_OK;
}

int staged_decode(DecoderCore &core, const DecodeBuffers &host, int32_t batch, size_t llr_elem, size_t post_elem,
                  bool seed_post, const std::function<int(const DecodeBuffers &, hipStream_t)> &decode) {
    const size_t n = core.code.n, hw = (n + 31) / 32, B = batch;
    const unsigned want = (host.hard ? plan::kHard : 0) | (host.iters ? plan::kIters : 0) | (host.syn_ok ? plan::kSynOk : 0) |
                          (host.post ? plan::kPost : 0) | (host.bit_errors ? plan::kBitErrors : 0) |
                          (host.totals ? plan::kTotals : 0);
    const plan::StageLayout l = plan::stage_layout(B, n, llr_elem, post_elem, want);
    if (l.bytes > core.stage_bytes) {
        (void)hipFree(core.d_stage);
        core.d_stage = nullptr;
        core.stage_bytes = 0;
        HIP_TRY(hipMalloc(&core.d_stage, l.bytes));
        core.stage_bytes = l.bytes;
    }
    char *base = static_cast<char *>(core.d_stage);
    auto at = [base](size_t off) { return off == plan::kNoRegion ? nullptr : base + off; };
    DecodeBuffers d;
    d.llr = at(l.llr);
    d.hard = reinterpret_cast<uint32_t *>(at(l.hard));
    d.iters = reinterpret_cast<int32_t *>(at(l.iters));
    d.syn_ok = reinterpret_cast<uint8_t *>(at(l.syn_ok));
    d.post = at(l.post);
    d.bit_errors = reinterpret_cast<int32_t *>(at(l.bit_errors));
    d.totals = reinterpret_cast<int64_t *>(at(l.totals));
    hipStream_t s = core.stream;
    HIP_TRY(hipMemcpyAsync(at(l.llr), host.llr, B * n * llr_elem, hipMemcpyHostToDevice, s));
    // Posteriors are left untouched on a pre-check pass (the reference keeps the previous frame's
    // Posteriori_fp, ArrayLDPC_Decoder.cpp:443-450): seed the device copy with the caller's buffer.
    if (d.post && seed_post) HIP_TRY(hipMemcpyAsync(d.post, host.post, B * n * post_elem, hipMemcpyHostToDevice, s));
    if (d.totals) HIP_TRY(hipMemcpyAsync(d.totals, host.totals, 32, hipMemcpyHostToDevice, s));
    const int st = decode(d, s);
    if (st) return st;
    if (d.hard) HIP_TRY(hipMemcpyAsync(host.hard, d.hard, B * hw * 4, hipMemcpyDeviceToHost, s));
    if (d.iters) HIP_TRY(hipMemcpyAsync(host.iters, d.iters, B * 4, hipMemcpyDeviceToHost, s));
    if (d.syn_ok) HIP_TRY(hipMemcpyAsync(host.syn_ok, d.syn_ok, B, hipMemcpyDeviceToHost, s));
    if (d.post) HIP_TRY(hipMemcpyAsync(host.post, d.post, B * n * post_elem, hipMemcpyDeviceToHost, s));
    if (d.bit_errors) HIP_TRY(hipMemcpyAsync(host.bit_errors, d.bit_errors, B * 4, hipMemcpyDeviceToHost, s));
    if (d.totals) HIP_TRY(hipMemcpyAsync(host.totals, d.totals, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FPLDPC_OK;
}

}  // namespace fpldpc
