// fpldpc_bias.hpp -- the bias object (fpldpc_bias_t) of mean-shift importance sampling, what the simulation
// (fpldpc_sim_rank.hpp) and fpldpc_channel.cpp take from fpldpc_bias.hip -- the per-device tables and the launcher of
// the patch kernel that follows the channel kernel on its stream -- and the weighted sums' frame step.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fpldpc.h"
#include "fpldpc_channel_args.hpp"

// One bias: the positions and their shifts (copied at creation), the device tables of the public channel call
// (bound on first use, as a harvest's check table), and the weighted sums of the last simulation.
struct fpldpc_bias {
    int n = 0;
    std::vector<int32_t> pos;   // [count] strictly ascending, 0 <= pos < n
    std::vector<double> shift;  // [count] finite, in units of the transmitted amplitude
    int device = -1;            // fpldpc_bias_channel_llr: the device the tables live on
    int32_t *d_pos = nullptr;
    double *d_shift = nullptr;
    fpldpc_bias_sums sums{};
    ~fpldpc_bias();
    int count() const { return (int)pos.size(); }
};

namespace fpldpc {

// The positions and shifts on the current device.  The caller frees both with hipFree (count = 0: both stay
// null, nothing is allocated).
int bias_upload_tables(const fpldpc_bias &b, int32_t **d_pos, double **d_shift);

// fpldpc_bias_channel_llr's first use of a bias on a device: the current device's tables into b (a bias stays with
// the device of its first call).
int bias_bind(fpldpc_bias *b);

// The patch kernel over a.frames frames of a channel call with the same arguments (include/fpldpc.h,
// fpldpc_bias_channel_llr): on `stream`, after launch_channel wrote a.out; n is the bias's.  a.logw may be null.
int launch_bias_patch(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, const ChannelArgs &a, void *stream);

// The weighted sums of a simulation (include/fpldpc.h, fpldpc_bias_sums) before its first frame, and one frame
// added to them: its log-weight and its block error count, in frame order.  The order of the additions is part of
// the definition.
inline fpldpc_bias_sums bias_sums_start() {
    fpldpc_bias_sums b{};
    b.min_logw = INFINITY;
    b.max_logw = -INFINITY;
    return b;
}
inline void bias_sums_add(fpldpc_bias_sums &b, double logw, int64_t blk) {
    const double w = exp(logw);
    const double fe = blk > 0 ? 1.0 : 0.0;
    ++b.frames;
    b.frame_errors += blk > 0;
    b.bit_errors += blk;
    b.sum_w += w;
    b.sum_w2 += w * w;
    b.sum_w_fe += w * fe;
    b.sum_w2_fe += w * w * fe;
    b.sum_w_be += w * (double)blk;
    b.min_logw = std::min(b.min_logw, logw);
    b.max_logw = std::max(b.max_logw, logw);
}

}  // namespace fpldpc
