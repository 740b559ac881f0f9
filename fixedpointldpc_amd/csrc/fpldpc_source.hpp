// fpldpc_source.hpp -- the counter-based noise source (include/fpldpc.h, FPLDPC_NOISE_PHILOX): Philox4x32-10
// and the two 53-bit uniforms of a pair, for the host twins (fpldpc_channel.cpp) and the device kernels
// (fpldpc_source.hip), and what fpldpc_sim.cpp takes from fpldpc_source.hip: the two launchers that stand beside
// launch_channel and launch_bias_patch.
#pragma once
#include <cstdint>

#include "fpldpc_bias.hpp"
#include "fpldpc_internal.hpp"

#if defined(__HIP__)
#define FPLDPC_HD __host__ __device__ inline
#else
#define FPLDPC_HD inline
#endif

namespace fpldpc {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
FPLDPC_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t r[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    r[0] = c0;
    r[1] = c1;
    r[2] = c2;
    r[3] = c3;
}

// The uniforms of pair `pair` of frame `frame` under `seed`: u1 in (0, 1], u2 in [0, 1), 53 bits each.  Counter word
// 1 is the stream id (0 = channel noise).
FPLDPC_HD void philox_uniforms(uint64_t seed, uint64_t frame, uint32_t pair, double *u1, double *u2) {
    uint32_t r[4];
    philox4x32_10(pair, 0u, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const uint64_t a = ((uint64_t)r[0] | (uint64_t)r[1] << 32) >> 11, b = ((uint64_t)r[2] | (uint64_t)r[3] << 32) >> 11;
    *u1 = (double)(a + 1) * 0x1p-53;  // exact: a + 1 <= 2^53
    *u2 = (double)b * 0x1p-53;
}

// What FPLDPC_NOISE_PHILOX asks of seed and frame range: 0 <= seed, 0 <= first_frame, first_frame + frames < 2^63
// (the Lehmer stream's rules stay with its own entry points).
inline bool philox_range_ok(int64_t seed, int64_t first_frame, int32_t frames) {
    return seed >= 0 && first_frame >= 0 && frames >= 0 && first_frame <= INT64_MAX - (int64_t)frames;
}

// The Philox channel over `frames` frames, launch_channel's arguments.
int launch_channel_philox(int64_t seed, int64_t first_frame, int frames, int n, double snr, double sigma, int frac_bits,
                          const uint8_t *cw, int cw_per_frame, void *out, int out_type, int *overflow, void *stream);
// The patch kernel behind it, launch_bias_patch's arguments.
int launch_bias_patch_philox(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, int64_t seed,
                             int64_t first_frame, int frames, double snr, double sigma, int frac_bits, const uint8_t *cw,
                             int cw_per_frame, void *out, int out_type, int *overflow, double *logw, void *stream);

// launch_channel / launch_bias_patch on either source (the caller has checked `source`)
inline int launch_channel_src(int source, int64_t seed, int64_t first_frame, int frames, int n, double snr, double sigma,
                              int frac_bits, const uint8_t *cw, int cw_per_frame, void *out, int out_type, int *overflow,
                              void *stream) {
    return (source == FPLDPC_NOISE_PHILOX ? launch_channel_philox : launch_channel)(
        seed, first_frame, frames, n, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, overflow, stream);
}
inline int launch_bias_patch_src(int source, const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, int64_t seed,
                                 int64_t first_frame, int frames, double snr, double sigma, int frac_bits, const uint8_t *cw,
                                 int cw_per_frame, void *out, int out_type, int *overflow, double *logw, void *stream) {
    return (source == FPLDPC_NOISE_PHILOX ? launch_bias_patch_philox : launch_bias_patch)(
        b, d_pos, d_shift, seed, first_frame, frames, snr, sigma, frac_bits, cw, cw_per_frame, out, out_type, overflow, logw,
        stream);
}

}  // namespace fpldpc
