// fpldpc_bias.hpp -- the bias object (fpldpc_bias_t) of mean-shift importance sampling and what
// fpldpc_sim.cpp and fpldpc_channel.cpp take from fpldpc_bias.hip: the per-device tables and the launcher of
// the patch kernel that follows the channel kernel on its stream.
#pragma once
#include <cstdint>
#include <vector>

#include "fpldpc_internal.hpp"

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

// The patch kernel over `frames` frames of a channel call with the same arguments (include/fpldpc.h,
// fpldpc_bias_channel_llr): on `stream`, after launch_channel wrote `out`.  logw [frames] may be null.
int launch_bias_patch(const fpldpc_bias &b, const int32_t *d_pos, const double *d_shift, int64_t seed, int64_t first_frame,
                      int frames, double snr, double sigma, int frac_bits, const uint8_t *cw, int cw_per_frame, void *out,
                      int out_type, int *overflow, double *logw, void *stream);

}  // namespace fpldpc
