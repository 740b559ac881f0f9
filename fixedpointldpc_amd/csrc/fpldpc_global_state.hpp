// fpldpc_global_state.hpp -- what the kernels with their state in global memory share (fpldpc_minsum_global.hip,
// fpldpc_flood_sat_global.hip): the LDS they keep (the frame's int16 vector, the control words and, where it
// still fits, the degree table), the rounding of a workgroup's slice of the scratch, and the reads of a flooding
// accumulator that integer atomics changed one step earlier.  Included by those translation units only, after
// fpldpc_layered_host.hpp.
#pragma once
#include "fpldpc_layered_device.hpp"

namespace fpldpc {
namespace {

// LDS: vec [n] int16 (up to a whole word) | misc [kLayMisc] | (!EXACT, where it fits) cdeg [m] uint8
__host__ __device__ constexpr size_t mg_misc_word(int n) { return ((size_t)n * sizeof(int16_t) + 3) / 4; }
__host__ __device__ constexpr size_t mg_base_bytes(int n) { return (mg_misc_word(n) + kLayMisc) * sizeof(int); }
__host__ __device__ constexpr bool mg_deg_in_lds(int n, int m) { return mg_base_bytes(n) + (size_t)m <= kLdsMax; }

__host__ __device__ constexpr size_t mg_round_slice(size_t bytes) { return (bytes + 255) / 256 * 256; }

// The degree table of a predicated kernel: staged behind the control words where it fits, else a.cdeg.
// (The first frame pull's barriers come between the staging and the first read.)
template <bool EXACT>
__device__ __forceinline__ const uint8_t *mg_degrees(const LayeredArgs &a, int *smem) {
    if constexpr (EXACT) {
        return nullptr;
    } else {
        if (!mg_deg_in_lds(a.n, a.m)) return a.cdeg;
        uint8_t *const ld = reinterpret_cast<uint8_t *>(smem) + mg_base_bytes(a.n);
        for (int i = threadIdx.x; i < a.m; i += blockDim.x) ld[i] = a.cdeg[i];
        return ld;
    }
}

__device__ __forceinline__ int fg_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// An accumulator word as lay_syndrome reads it (post[v] <= 0), through fg_load.
struct FgAcc {
    int raw;
    __device__ __forceinline__ bool operator<=(int x) const { return fg_load(&raw) <= x; }
};

}  // namespace
}  // namespace fpldpc
