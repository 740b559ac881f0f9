// fpldpc_sim_source.hpp -- what fpldpc_sim.cpp takes from fpldpc_sim_source.hip besides the public
// fpldpc_info_bits: the count of a chunk's decoded information bits against the bits its frames were sent with.
#pragma once
#include <cstdint>

namespace fpldpc {
// blkerror[f] = #{ i < k : bit info_idx[i] of hard[f][hard_words] != info[f][i] } for f < frames; device
// pointers, asynchronous on stream (hipStream_t).
int launch_count_info(const uint32_t *hard, int hard_words, const int32_t *info_idx, const uint8_t *info, int k,
                      int frames, int32_t *blkerror, void *stream);
// The float simulation's forced positions: llr[f][idx[i]] = value for f < frames, i < n_idx on a double [frames][n]
// array, launch_force_llr's counterpart (idx values in [0, n), checked by the simulation's validation).
int launch_force_llr_f64(double *llr, int frames, int n, const int32_t *idx, int n_idx, double value, void *stream);
}  // namespace fpldpc
