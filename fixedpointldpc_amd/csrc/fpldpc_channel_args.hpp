// fpldpc_channel_args.hpp -- the arguments of one channel call (include/fpldpc.h, fpldpc_channel_llr and its biased
// and *_src forms), as one block: what the host channel loop (fpldpc_channel.cpp), the device launchers
// (fpldpc_source.hpp, fpldpc_bias.hpp) and a simulation's chunk (fpldpc_sim_rank.hpp) hand to each other.  No HIP.
#pragma once
#include <cstdint>

namespace fpldpc {

struct ChannelArgs {
    int64_t seed = 0, first_frame = 0;
    int frames = 0, n = 0;
    double snr = 0.0, sigma = 0.0;
    int frac_bits = 0;
    const uint8_t *cw = nullptr;  // null: the all-zero codeword
    int cw_per_frame = 0;         // 1: cw is [frames][n]
    void *out = nullptr;          // [frames][n] of out_type
    int out_type = 0;
    int *overflow = nullptr;      // device calls: the int16 overflow count, or null
    double *logw = nullptr;       // biased calls: [frames], or null
};

}  // namespace fpldpc
