// fpldpc_source.hpp -- the counter-based noise source (include/fpldpc.h, FPLDPC_NOISE_PHILOX): Philox4x32-10
// and the two 53-bit uniforms of a pair, for the host twins (fpldpc_channel.cpp) and the device kernels
// (fpldpc_source.hip), their shared argument rules, and what the simulation (fpldpc_sim_rank.hpp) takes from
// fpldpc_source.hip: the two launchers that stand beside launch_channel and launch_bias_patch.
#pragma once
#include <cstdint>

#include "fpldpc_bias.hpp"
#include "fpldpc_channel_args.hpp"
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

// The argument rules of a channel call on the Philox source, for the host twins and the device entry points alike:
// the channel's own, with 0 <= seed, 0 <= first_frame and first_frame + frames < 2^63 in place of the Lehmer stream's.
inline int philox_rules(const ChannelArgs &a) {
    if (!a.out || a.n <= 0 || a.frac_bits < 0 || a.frac_bits > 24 || a.seed < 0 || a.first_frame < 0 || a.frames < 0 ||
        a.first_frame > INT64_MAX - (int64_t)a.frames)
        return fail(FPLDPC_ERR_ARG, "bad channel arguments (philox: 0 <= seed, first_frame + frames < 2^63)");
    if (a.out_type != FPLDPC_LLR_I32 && a.out_type != FPLDPC_LLR_I16 && a.out_type != FPLDPC_LLR_F64)
        return fail(FPLDPC_ERR_ARG, "bad out_type");
    if (a.cw_per_frame != 0 && a.cw_per_frame != 1) return fail(FPLDPC_ERR_ARG, "cw_per_frame must be 0 or 1");
    return FPLDPC_OK;
}

// The Philox channel over a.frames frames, as launch_channel (a.logw unused).
int launch_channel_philox(const ChannelArgs &a, void *stream);
// The patch kernel behind it, as launch_bias_patch.
int launch_bias_patch_philox(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, const ChannelArgs &a,
                             void *stream);

// launch_channel / launch_bias_patch on either source (the caller has checked `source`)
inline int launch_channel_src(int source, const ChannelArgs &a, void *stream) {
    if (source == FPLDPC_NOISE_PHILOX) return launch_channel_philox(a, stream);
    return launch_channel(a.seed, a.first_frame, a.frames, a.n, a.snr, a.sigma, a.frac_bits, a.cw, a.cw_per_frame, a.out,
                          a.out_type, a.overflow, stream);
}
inline int launch_bias_patch_src(int source, const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift,
                                 const ChannelArgs &a, void *stream) {
    return (source == FPLDPC_NOISE_PHILOX ? launch_bias_patch_philox : launch_bias_patch)(b, d_pos, d_shift, a, stream);
}

}  // namespace fpldpc
