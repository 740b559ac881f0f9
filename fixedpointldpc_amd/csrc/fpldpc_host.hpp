// fpldpc_host.hpp -- the host plumbing every decoder object shares (fpldpc_host.cpp): the device guard, the
// HIP-error-to-status macro, the parameter and device checks of creation, the reference bits of the state every
// decoder object has (DecoderCore, fpldpc_internal.hpp), the checks every decode call starts with and the staged
// host decode.
//
// Outside the kernel build id (fixedpointldpc_amd/_build.py HASHED_TUS): nothing here is read by a kernel or
// decides how one is chosen or launched.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>

#include <hip/hip_runtime_api.h>

#include "fpldpc_internal.hpp"

namespace fpldpc {

// Makes `dev` the calling thread's device (dev < 0: leaves it) and restores the caller's on the way out.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    DeviceGuard() = default;  // holds nothing until enter()
    explicit DeviceGuard(int dev) { enter(dev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
    void enter(int dev) {
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

// Constant = int((5.0/8.0) * (1 << FRAC_WIDTH)) (ArrayLDPCMacro.h:175)
inline int constant_c(int frac_bits) { return (int)((5.0 / 8.0) * (1 << frac_bits)); }
// The largest magnitude of a `bits`-wide saturated value
inline int sat_limit(int bits) { return (1 << (bits - 1)) - 1; }

// *p = the defaults, or *params when given, range-checked.
int resolve_params(const fpldpc_params *params, fpldpc_params *p);
// *dev = `requested`, or the current device when it is negative; fails without a HIP device (there is no CPU
// path) and for an ordinal the machine does not have.
int select_device(int requested, int *dev);

// Frees what the core (DecoderCore, fpldpc_internal.hpp) owns (on the decoder's device: the caller holds the guard).
void core_free(DecoderCore &core);
// Uploads (k > 0) or drops (k == 0) the reference bits; FPLDPC_ERR_ARG "bad reference" for a null core.
int set_reference(DecoderCore *core, const int32_t *info_index, const uint8_t *info_bits, int32_t k);

// The checks every decode call starts with, in this order: a null decoder, a negative batch, an empty batch
// (*run stays false: the call is done, FPLDPC_OK), a null llr, *llr_type (null: not checked) neither
// FPLDPC_LLR_I32 nor FPLDPC_LLR_I16, bit_errors without reference bits ("... without <set_reference_name>"),
// then `g` enters the decoder's device.  *run = true: go on.
int decode_prologue(const DecoderCore *core, const void *llr, const int32_t *llr_type, int32_t batch,
                    const int32_t *bit_errors, const char *set_reference_name, DeviceGuard *g, bool *run);

// The buffers of a decode call (host memory for the caller of staged_decode, device memory for the decode
// it runs); post has 4-byte (fixed-point) or 8-byte (float) elements.
struct DecodeBuffers {
    const void *llr = nullptr;
    uint32_t *hard = nullptr;
    int32_t *iters = nullptr;
    uint8_t *syn_ok = nullptr;
    void *post = nullptr;
    int32_t *bit_errors = nullptr;
    int64_t *totals = nullptr;
};

// A decode of host buffers through the decoder's staging block (plan::stage_layout) on the decoder's own
// stream: LLRs and the starting totals up, `decode` on the block's device pointers, every output present
// back, then that stream alone is synchronised.  seed_post: the posteriors go up as well (a decoder with a
// pre-check leaves a passing frame's untouched).  On the decoder's device (the caller holds the guard).
int staged_decode(DecoderCore &core, const DecodeBuffers &host, int32_t batch, size_t llr_elem, size_t post_elem,
                  bool seed_post, const std::function<int(const DecodeBuffers &, hipStream_t)> &decode);

}  // namespace fpldpc
