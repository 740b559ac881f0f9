// fpldpc_layered_device.hpp -- device code the layered kernels share (fpldpc_layered.hip: the sxor fold;
// fpldpc_layered_minsum.hip: min-sum with compressed check state; fpldpc_minsum.hip: the same rule on the
// flooding schedule; fpldpc_minsum_global.hip: both with the state in global memory; fpldpc_flood_sat.hip: the
// sxor fold on the flooding schedule; fpldpc_flood_sat_global.hip: the same with the state in global memory):
// the frame framework's constants, the frame pull and the way out of
// the kernel, the LLR load, the box-plus, the syndrome and the frame epilogue.  Included by those translation
// units (the min-sum units through fpldpc_minsum_device.hpp, the check rule they share).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpldpc_layered.hpp"

namespace fpldpc {
namespace {

constexpr int kLayMaxNT = 256;  // largest workgroup (4 waves); a decoder uses min(256, L rounded up to 64)
constexpr int kLayMisc = 4;     // per-workgroup control words after the posteriors: [0] frame, [1] bit errors
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kExactDc = 47;  // the straight-line instantiation: the p = 47 array codes (A, R)

__device__ __forceinline__ int lay_clamp(int x, int S) { return min(max(x, -S), S); }

// x [+] y (ArrayLDPC_Decoder.cpp:677-694, sgn(0) = -1 ArrayLDPCMacro.h:222-224), as boxplus() of
// fpldpc_flood_device.hpp: sgn(x) sgn(y) is +1 iff (x > 0) == (y > 0).  The sxor of fpldpc_layered.hip and
// fpldpc_flood_sat.hip.
__device__ __forceinline__ int lay_boxplus(int x, int y, int C, int mask) {
    const int a = x < 0 ? -x : x;
    const int b = y < 0 ? -y : y;
    const int s = ((a + b) & mask) >> 2;
    const int d = ((a > b ? a - b : b - a) & mask) >> 2;
    const int p1 = max(C - s, 0);
    const int p2 = max(C - d, 0);
    const int r = min(a, b) + p1 - p2;
    return ((x > 0) == (y > 0)) ? r : -r;
}

__device__ __forceinline__ int lay_load_llr(const LayeredArgs &a, size_t i) {
    return a.llr_i16 ? (int)static_cast<const int16_t *>(a.llr)[i] : static_cast<const int32_t *>(a.llr)[i];
}

// The next frame of this workgroup from the work counter, or -1 when the batch is taken; clears the frame's
// bit-error word.  Two barriers: the first keeps the previous frame's readers of misc ahead of the write.
__device__ __forceinline__ int lay_next_frame(const LayeredArgs &a, int *misc) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const int wi = atomicAdd(&a.counters[0], 1);
        misc[0] = wi < a.batch ? wi : -1;
        misc[1] = 0;
    }
    __syncthreads();
    return misc[0];
}

// Leaving the kernel: the last workgroup out resets the counter block for the next call (every workgroup
// has made its last work-counter access, a returning atomic, before counting itself out).
__device__ __forceinline__ void lay_leave(const LayeredArgs &a) {
    if (threadIdx.x == 0 && atomicAdd(&a.counters[1], 1) == (int)gridDim.x - 1) {
        a.counters[0] = 0;
        a.counters[1] = 0;
    }
}

// 1 if some check is unsatisfied by hard[v] = post[v] > 0 ? 0 : 1 (workgroup-uniform; a barrier).
// cdeg: the degree table (LDS), unused when every check has degree DC (EXACT).
template <int DC, bool EXACT, typename ST>
__device__ __forceinline__ int lay_syndrome(const LayeredArgs &a, const uint16_t *vidx, const uint8_t *cdeg,
                                            const ST *post) {
    const int m = a.m, p = a.array_p;
    int fail = 0;
    for (int c = threadIdx.x; c < m; c += blockDim.x) {
        const int deg = EXACT ? DC : (int)cdeg[c];
        int ci = 0, col = 0;
        if (!vidx) {
            ci = c / p;
            col = c - ci * p;
        }
        int par = 0;
        for (int k = 0; k < deg; ++k) {
            const int v = vidx ? (int)vidx[(size_t)k * m + c] : k * p + col;
            col += ci;
            if (col >= p) col -= p;
            par ^= post[v] <= 0;
        }
        fail |= par;
    }
    return __syncthreads_or(fail);
}

// Frame epilogue: posteriors, packed hard decisions, per-frame bit errors and totals
// ({bit errors, frames with errors, frames, iteration sum}, added to).
template <typename ST>
__device__ __forceinline__ void lay_store(const LayeredArgs &a, int cw, const ST *post, bool write_post, int iters,
                                          int ok, int *misc) {
    const int n = a.n, NT = blockDim.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.post && write_post)
        for (int v = tid; v < n; v += NT) a.post[(size_t)cw * n + v] = post[v];
    if (a.hard) {
        uint32_t *h = a.hard + (size_t)cw * a.hard_words;
        for (int base = wave * 64; base < n; base += NT) {
            const int v = base + lane;
            const unsigned long long b = __ballot(v < n && post[v] <= 0);
            if (lane == 0) {
                const int w = base >> 5;
                h[w] = (uint32_t)b;
                if (w + 1 < a.hard_words) h[w + 1] = (uint32_t)(b >> 32);
            }
        }
    }
    int errors = 0;
    if (a.k_info > 0) {
        int e = 0;
        for (int i = tid; i < a.k_info; i += NT) e += ((post[a.info_idx[i]] <= 0) ? 1 : 0) != a.info_bits[i];
        if (e) atomicAdd(&misc[1], e);
        __syncthreads();
        errors = misc[1];
    }
    if (tid == 0) {
        if (a.iters) a.iters[cw] = iters;
        if (a.syn_ok) a.syn_ok[cw] = (uint8_t)ok;
        if (a.bit_errors) a.bit_errors[cw] = errors;
        if (a.totals) {
            atomicAdd(&a.totals[0], (unsigned long long)errors);
            atomicAdd(&a.totals[1], (unsigned long long)(errors > 0));
            atomicAdd(&a.totals[2], 1ull);
            atomicAdd(&a.totals[3], (unsigned long long)iters);
        }
    }
}

}  // namespace
}  // namespace fpldpc
