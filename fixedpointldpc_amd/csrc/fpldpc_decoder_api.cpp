// fpldpc_decoder_api.cpp -- the flooding decoder's entry points of the C ABI (include/fpldpc.h) that read the
// decoder object or stage host buffers around a device decode.
//
// A translation unit of its own, outside the kernel build id (fixedpointldpc_amd/_build.py HASHED_TUS): nothing
// here is read by a kernel or decides how one is chosen or launched (that is fpldpc_decoder.cpp and the kernel
// units), so an edit here leaves the committed counters those of the shipped kernels.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "fpldpc_host.hpp"
#include "fpldpc_testing.h"

using namespace fpldpc;

namespace {

// The decoder's counter block once the last call's kernels are done, on whichever stream they ran.
int last_counters(fpldpc_decoder_t dec, int32_t c[kCounterInts]) {
    DeviceGuard g(dec->device);
    HIP_TRY(hipEventSynchronize(dec->last_done));
    HIP_TRY(hipMemcpy(c, dec->d_counter, sizeof(int32_t) * kCounterInts, hipMemcpyDeviceToHost));
    return FPLDPC_OK;
}

}  // namespace

extern "C" {

void fpldpc_params_default(fpldpc_params *p) {
    if (!p) return;
    p->max_iter = 30;     // ArrayLDPCMacro.h:17
    p->frac_bits = 4;     // ArrayLDPCMacro.h:36
    p->width_mask = 0xff; // ArrayLDPCMacro.h:29
    p->early_term = 1;    // ArrayLDPC_Decoder.cpp:164-167
    p->precheck = 0;
    p->device = -1;
}

int fpldpc_decoder_describe(fpldpc_decoder_t dec, char *buf, size_t cap) {
    if (!dec || !buf || cap == 0) return fail(FPLDPC_ERR_ARG, "null argument");
    snprintf(buf, cap, "%s grid=%d threads=%d lds=%zu device=%d", dec->kc.name, dec->kc.grid, dec->kc.threads,
             dec->kc.lds_bytes, dec->device);
    return FPLDPC_OK;
}

int fpldpc_decoder_hard_words(fpldpc_decoder_t dec) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null argument");
    return (dec->code.n + 31) / 32;
}

int fpldpc_decoder_fallback_counts(fpldpc_decoder_t dec, int32_t counts[2]) {
    if (!dec || !counts) return fail(FPLDPC_ERR_ARG, "null argument");
    counts[0] = counts[1] = 0;
    if (dec->kc.fallback == Variant::kNone) return FPLDPC_OK;
    int32_t c[kCounterInts];
    const int st = last_counters(dec, c);
    if (st) return st;
    counts[0] = c[kCountFb0Last];
    counts[1] = dec->kc.fallback2 == Variant::kNone ? 0 : c[kCountFb1Last];  // (no list 1: the stationary exits' word)
    return FPLDPC_OK;
}

// Test-only (include/fpldpc_testing.h): frames the last completed decode call ended by the stationary exit.
int fpldpc_testing_stationary_exits(void *decoder, int32_t *count) {
    fpldpc_decoder_t dec = static_cast<fpldpc_decoder_t>(decoder);
    if (!dec || !count) return fail(FPLDPC_ERR_ARG, "null argument");
    *count = 0;
    if (dec->kc.fallback == Variant::kNone || dec->kc.fallback2 != Variant::kNone) return FPLDPC_OK;
    int32_t c[kCounterInts];
    const int st = last_counters(dec, c);
    if (st) return st;
    *count = c[kCountFb1Last];
    return FPLDPC_OK;
}

// Test-only (include/fpldpc_testing.h): frames the last completed decode call ended by the cycle exit.
int fpldpc_testing_cycle_exits(void *decoder, int32_t *count) {
    fpldpc_decoder_t dec = static_cast<fpldpc_decoder_t>(decoder);
    if (!dec || !count) return fail(FPLDPC_ERR_ARG, "null argument");
    *count = 0;
    if (dec->kc.fallback == Variant::kNone || dec->kc.fallback2 != Variant::kNone) return FPLDPC_OK;
    int32_t c[kCounterInts];
    const int st = last_counters(dec, c);
    if (st) return st;
    *count = c[kCountCycLast];
    return FPLDPC_OK;
}

int fpldpc_edge_ram_words(fpldpc_decoder_t dec, int64_t *words) {
    if (!dec || !words) return fail(FPLDPC_ERR_ARG, "null argument");
    *words = (int64_t)dec->code.dc_max * dec->code.m;
    return FPLDPC_OK;
}

int fpldpc_decode_host(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                       int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals) {
    DeviceGuard g;
    bool run = false;
    const int st = decode_prologue(dec, llr, &llr_type, batch, bit_errors, "fpldpc_set_reference", &g, &run);
    if (st || !run) return st;
    return staged_decode(*dec, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, batch,
                         llr_type == FPLDPC_LLR_I16 ? 2 : 4, 4, true, [&](const DecodeBuffers &d, hipStream_t s) {
                             return fpldpc_decode(dec, d.llr, llr_type, batch, d.hard, d.iters, d.syn_ok,
                                                  static_cast<int32_t *>(d.post), d.bit_errors, d.totals, s);
                         });
}

// The float decode writes every frame's posteriors (it has no pre-check), so the caller's are not sent up.
int fpldpc_decode_float_host(fpldpc_decoder_t dec, const double *llr, int32_t batch, uint32_t *hard, int32_t *iters,
                             uint8_t *syndrome_ok, double *post, int32_t *bit_errors, int64_t *totals) {
    DeviceGuard g;
    bool run = false;
    const int st = decode_prologue(dec, llr, nullptr, batch, bit_errors, "fpldpc_set_reference", &g, &run);
    if (st || !run) return st;
    return staged_decode(*dec, {llr, hard, iters, syndrome_ok, post, bit_errors, totals}, batch, 8, 8, false,
                         [&](const DecodeBuffers &d, hipStream_t s) {
                             return fpldpc_decode_float(dec, static_cast<const double *>(d.llr), batch, d.hard, d.iters,
                                                        d.syn_ok, static_cast<double *>(d.post), d.bit_errors, d.totals, s);
                         });
}

int fpldpc_decode_frame_host(fpldpc_decoder_t dec, const int32_t *llr, int32_t keep_edges, int32_t *edge_ram,
                             uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok, int32_t *post) {
    if (!dec) return fail(FPLDPC_ERR_ARG, "null decoder");
    if (!llr || !edge_ram) return fail(FPLDPC_ERR_ARG, "null llr or edge RAM");
    DeviceGuard g(dec->device);
    if (!g.ok) return fail(FPLDPC_ERR_HIP, "hipSetDevice failed");
    const size_t n = dec->code.n, hw = (n + 31) / 32, ew = (size_t)dec->code.dc_max * dec->code.m;
    // One staging block, the same layout in pinned host memory and on the device: llr [n], edge RAM
    // [ew], post [n], hard [hw], iters, syndrome flag.  The reference's callers decode one frame per
    // call (PerfTest.cpp:121-128), so a call is one host-to-device copy of the inputs, the kernel and
    // one copy back of the outputs (3 submissions), not one pageable copy per buffer.
    const size_t in_words = 2 * n + ew, words = in_words + hw + 2;
    if (!dec->d_edge_stage) HIP_TRY(hipMalloc(&dec->d_edge_stage, sizeof(int32_t) * words));
    if (!dec->h_edge_stage) HIP_TRY(hipHostMalloc((void **)&dec->h_edge_stage, sizeof(int32_t) * words, hipHostMallocDefault));
    int32_t *h = dec->h_edge_stage;
    memcpy(h, llr, n * 4);
    memcpy(h + n, edge_ram, ew * 4);  // kept as is by a pre-check pass
    if (post) memcpy(h + n + ew, post, n * 4);  // likewise (:443-450)
    int32_t *d_llr = dec->d_edge_stage, *d_edge = d_llr + n, *d_post = d_edge + ew;
    uint32_t *d_hard = reinterpret_cast<uint32_t *>(d_post + n);
    int32_t *d_it = reinterpret_cast<int32_t *>(d_hard + hw);
    uint8_t *d_ok = reinterpret_cast<uint8_t *>(d_it + 1);
    hipStream_t s = dec->stream;
    HIP_TRY(hipMemcpyAsync(d_llr, h, (post ? in_words : n + ew) * 4, hipMemcpyHostToDevice, s));
    int st = fpldpc_decode_frame(dec, d_llr, FPLDPC_LLR_I32, keep_edges, d_edge, d_hard, d_it, d_ok,
                                 post ? d_post : nullptr, s);
    if (st) return st;
    HIP_TRY(hipMemcpyAsync(h + n, d_edge, (words - n) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(edge_ram, h + n, ew * 4);
    if (post) memcpy(post, h + n + ew, n * 4);
    if (hard) memcpy(hard, h + in_words, hw * 4);
    if (iters) memcpy(iters, h + in_words + hw, 4);
    if (syndrome_ok) *syndrome_ok = *reinterpret_cast<const uint8_t *>(h + in_words + hw + 1);
    return FPLDPC_OK;
}

}  // extern "C"
