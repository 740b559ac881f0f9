// fpldpc_layered_minsum.hip -- gfx950 (CDNA4) layered min-sum decoder with compressed check state
// (fpldpc_layered_create_minsum, include/fpldpc.h; DESIGN.md "Layered min-sum decoder").
//
// The schedule, the clamps and the frame framework are the saturated layered decoder's
// (fpldpc_layered.hip): persistent grid, one workgroup per frame, frames pulled from a work counter that
// the last workgroup out resets, lane j on check l*L + j, one barrier between layers, int16 posteriors in
// LDS.  The check rule is normalised / offset min-sum: with f(x) = max(((x * scale_16) >> 4) - offset, 0)
//     t[k] = clamp(post[v_k] - c2v[c][k], S_m);  s[k] = t[k] <= 0
//     m1 = min |t|, k1 a slot attaining it, m2 = min over the other slots
//     new[k] = (parity of s over j != k) ? -f(k == k1 ? m2 : m1) : f(k == k1 ? m2 : m1)
//     c2v[c][k] = new[k];  post[v_k] = clamp(t[k] + new[k], S_p)
//
// A check's messages take only two magnitudes, so its state is compressed: 16 bytes whatever the degree,
//     { int16 f(m1), int16 f(m2), int32 k1, uint64 sign word (bit k = s[k]) }
// one entry per check in LDS, lane j of a layer on entry l*L + j (one 16-byte access per lane, consecutive
// lanes on consecutive entries).  Message k is rebuilt as magnitude k == k1 ? f(m2) : f(m1) with sign
// parity(sign word) ^ s[k]; an all-zero entry rebuilds every message to 0, the frame's initial state.
// There is no per-edge c2v array and no global scratch for any code.
//
// A check is a gather and two passes over its slots.  The gather issues every post[v_k] read before any
// is waited for and keeps v_k (uint16) and the posterior packed in one register per slot.  Pass 1 rebuilds
// the old message, puts t[k] (int16: |t| <= S_m < 2^15) in the posterior's place and tracks m1, m2, k1
// and the sign word.  Pass 2 emits new[k] and stores the posteriors.  No lane reads a posterior that
// another lane of its layer writes (no variable occurs twice inside a layer).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fpldpc_layered_device.hpp"

namespace fpldpc {
namespace {

struct MinsumArgs {
    LayeredArgs a;  // as the other layered kernels read it (C, mask and c2v_scratch unused)
    int scale_16 = 16, offset = 0;
};

constexpr size_t kMsStateBytes = 16;  // per check

// bytes of the posteriors and control words, rounded up to the 16-byte alignment of the state entries
__host__ __device__ constexpr size_t ms_state_offset(int n) {
    return ((((size_t)n * sizeof(int16_t) + 3) / 4 + kLayMisc) * sizeof(int) + 15) / 16 * 16;
}

__device__ __forceinline__ int ms_correct(int x, int scale_16, int offset) { return max(((x * scale_16) >> 4) - offset, 0); }

// (x ^ neg) - neg: x for neg = 0, -x for neg = -1
__device__ __forceinline__ int ms_signed(int x, int neg) { return (x ^ neg) - neg; }
// -(bit k of the 64-bit word hi:lo) for a constant k: one signed bit-field extract
__device__ __forceinline__ int ms_neg_bit(uint32_t lo, uint32_t hi, int k) {
    return (int)((k < 32 ? lo : hi) << (31 - (k & 31))) >> 31;
}

// LDS: post [n] int16 (up to a whole word) | misc [kLayMisc] | (to 16 bytes) state [m] uint4
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8
// DC / EXACT as layered_generic: the exact degree 47 in straight-line code, else the next of 8 / 16 / 32 /
// 48 / 64 with the slots predicated on the check's degree.  COMPUTED: forward array code, v = k*p +
// (j + i*k) mod p; else the index table (a.vidx, staged in LDS with a.table_lds).
// Signs are arithmetic (0 / -1 words, bit-field extracts), not lane masks: the unrolled slots would
// otherwise hold one scalar register pair each.
template <int DC, bool EXACT, bool COMPUTED>
__global__ void __launch_bounds__(kLayMaxNT) layered_minsum(MinsumArgs ma) {
    const LayeredArgs &a = ma.a;
    extern __shared__ __attribute__((aligned(16))) int lay_smem[];
    const int n = a.n, m = a.m, p = a.array_p;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    int16_t *const post = reinterpret_cast<int16_t *>(lay_smem);
    int *const misc = lay_smem + ((size_t)n * sizeof(int16_t) + 3) / 4;
    uint4 *const state = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(lay_smem) + ms_state_offset(n));
    const size_t edges = (size_t)a.dc_max * m;
    const uint16_t *vidx = COMPUTED ? nullptr : a.vidx;
    if (!COMPUTED && a.table_lds) {
        uint16_t *const lv = reinterpret_cast<uint16_t *>(state + m);
        for (int i = tid; i < (int)edges; i += NT) lv[i] = a.vidx[i];
        vidx = lv;
    }
    const uint8_t *cdeg = nullptr;
    if constexpr (!EXACT) {
        uint8_t *const ld = reinterpret_cast<uint8_t *>(state + m) + (!COMPUTED && a.table_lds ? edges * sizeof(uint16_t) : 0);
        for (int i = tid; i < m; i += NT) ld[i] = a.cdeg[i];
        cdeg = ld;
    }

    for (;;) {
        __syncthreads();
        if (tid == 0) {
            const int wi = atomicAdd(&a.counters[0], 1);
            misc[0] = wi < a.batch ? wi : -1;
            misc[1] = 0;
        }
        __syncthreads();
        const int cw = misc[0];
        if (cw < 0) break;
        for (int v = tid; v < n; v += NT) post[v] = (int16_t)lay_clamp(lay_load_llr(a, (size_t)cw * n + v), Sp);
        for (int c = tid; c < m; c += NT) state[c] = make_uint4(0, 0, 0, 0);  // every c2v = 0
        __syncthreads();
        // the channel pre-check, as the other layered kernels: 0 iterations, posteriors left untouched
        if (a.precheck && !lay_syndrome<DC, EXACT>(a, vidx, cdeg, post)) {
            lay_store(a, cw, post, false, 0, 1, misc);
            continue;
        }
        int iters = 0, fail = 1;
        for (int it = 1; it <= a.max_iter; ++it) {
            for (int l = 0; l < a.layers; ++l) {
                for (int j = tid; j < a.L; j += NT) {
                    const int c = l * a.L + j;
                    const int deg = EXACT ? DC : (int)cdeg[c];
                    int ci = 0, col = 0;
                    if constexpr (COMPUTED) {
                        ci = c / p;
                        col = c - ci * p;
                    }
                    // the check's state: x = f(m1) | f(m2) << 16, y = k1, (z, w) = sign word
                    const uint4 st = state[c];
                    const int oM1 = (int)(st.x & 0xffff), oM2 = (int)(st.x >> 16), ok1 = (int)st.y;
                    // bit k of (olo, ohi): old message k is negative (its sign bit ^ the check's parity)
                    const uint32_t oflip = 0u - (uint32_t)((__popc(st.z) + __popc(st.w)) & 1);
                    const uint32_t olo = st.z ^ oflip, ohi = st.w ^ oflip;
                    // gather: every read of the check in flight at once; pk[k] = v_k << 16 | (uint16) post[v_k]
                    uint32_t pk[DC];
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        pk[k] = 0;
                        if (k < deg) {
                            uint32_t v;
                            if constexpr (COMPUTED) {
                                v = (uint32_t)(k * p + col);
                                col += ci;
                                col = (int)min((uint32_t)col, (uint32_t)(col - p));  // mod p (col < 2p)
                            } else {
                                v = vidx[(size_t)k * m + c];
                            }
                            pk[k] = v << 16 | (uint16_t)post[v];
                        }
                    }
                    // pass 1: pk[k] becomes v_k << 16 | (uint16) t[k]
                    int m1 = 0x7fff, m2 = 0x7fff, k1 = 0;
                    uint32_t lo = 0, hi = 0;
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if (k >= deg) continue;
                        const int old = ms_signed(k == ok1 ? oM2 : oM1, ms_neg_bit(olo, ohi, k));
                        const int t = lay_clamp((int)(int16_t)(pk[k] & 0xffffu) - old, Sm);
                        const int mag = max(t, -t);
                        const uint32_t s = (uint32_t)(t - 1) >> 31;  // t <= 0
                        if (k < 32)
                            lo |= s << (k & 31);
                        else
                            hi |= s << (k & 31);
                        m2 = min(m2, max(mag, m1));
                        k1 = mag < m1 ? k : k1;
                        m1 = min(m1, mag);
                        pk[k] = (pk[k] & 0xffff0000u) | ((uint32_t)t & 0xffffu);
                    }
                    const int M1 = ms_correct(m1, ma.scale_16, ma.offset), M2 = ms_correct(m2, ma.scale_16, ma.offset);
                    state[c] = make_uint4((uint32_t)M1 | (uint32_t)M2 << 16, (uint32_t)k1, lo, hi);
                    const uint32_t flip = 0u - (uint32_t)((__popc(lo) + __popc(hi)) & 1);
                    lo ^= flip;  // bit k: new message k is negative
                    hi ^= flip;
                    // pass 2
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if (k >= deg) continue;
                        const int t = (int)(int16_t)(pk[k] & 0xffffu), v = (int)(pk[k] >> 16);
                        const int nw = ms_signed(k == k1 ? M2 : M1, ms_neg_bit(lo, hi, k));
                        post[v] = (int16_t)lay_clamp(t + nw, Sp);
                    }
                }
                __syncthreads();  // the next layer reads the posteriors this one wrote
            }
            fail = lay_syndrome<DC, EXACT>(a, vidx, cdeg, post);
            iters = it;
            if (a.early_term && !fail) break;
        }
        lay_store(a, cw, post, true, iters, !fail, misc);
    }
    // the last workgroup out resets the counter block for the next call (every workgroup has made
    // its last work-counter access, a returning atomic, before counting itself out)
    if (tid == 0 && atomicAdd(&a.counters[1], 1) == (int)gridDim.x - 1) {
        a.counters[0] = 0;
        a.counters[1] = 0;
    }
}

using MinsumFn = void (*)(MinsumArgs);
template <bool COMPUTED>
MinsumFn minsum_fn_of(int dc, bool exact) {
    if (exact) return layered_minsum<kExactDc, true, COMPUTED>;
    switch (dc) {
        case 8: return layered_minsum<8, false, COMPUTED>;
        case 16: return layered_minsum<16, false, COMPUTED>;
        case 32: return layered_minsum<32, false, COMPUTED>;
        case 48: return layered_minsum<48, false, COMPUTED>;
        case 64: return layered_minsum<64, false, COMPUTED>;
    }
    return nullptr;
}

MinsumFn minsum_fn(const LayeredChoice &lc) {
    return lc.computed ? minsum_fn_of<true>(lc.dc, lc.exact) : minsum_fn_of<false>(lc.dc, lc.exact);
}

}  // namespace

// Envelope: check degrees 2..64, any valid layer size, and the int16 posteriors, the control words, 16
// bytes per check and one byte per check of the degree table (unless the kernel's DC is every check's
// degree) within the CU's 160 KiB of LDS.
int layered_minsum_choose(const fpldpc_code &code, int L, int device, LayeredChoice *out) {
    for (int r = 0; r < code.m; r++)
        if (code.cdeg[r] < 2) return fail(FPLDPC_ERR_UNSUPPORTED, "check of degree < 2 (reference behaviour undefined)");
    int dc = 0;
    for (int d : {8, 16, 32, 48, 64})
        if (!dc && code.dc_max <= d) dc = d;
    if (!dc) return fail(FPLDPC_ERR_UNSUPPORTED, "layered decoder: check degree above 64");
    LayeredChoice lc;
    lc.mode = kLayMinsum;
    lc.exact = code.regular_checks && code.dc_max == kExactDc;
    lc.dc = lc.exact ? kExactDc : dc;
    lc.computed = code.array_forward && code.array_p > 0;
    lc.lds_state = true;
    lc.threads = std::min(kLayMaxNT, (L + 63) / 64 * 64);
    const size_t base = ms_state_offset(code.n) + kMsStateBytes * code.m + (lc.exact ? 0 : (size_t)code.m);
    if (base > kLdsMax)
        return fail(FPLDPC_ERR_UNSUPPORTED, "layered min-sum decoder: posteriors and check state do not fit 160 KiB of LDS");
    const size_t tab_bytes = lc.computed ? 0 : (size_t)code.dc_max * code.m * sizeof(uint16_t);
    const MinsumFn fn = minsum_fn(lc);
    hipError_t e = hipSuccess;
    auto resident = [&](size_t lds) {
        int per_cu = 0;
        if (e == hipSuccess && lds > 64 * 1024) e = raise_dynamic_lds((const void *)fn, lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, lc.threads, lds);
        return e == hipSuccess ? per_cu : 0;
    };
    // the index table joins the state in LDS only where that costs no resident workgroup, as in
    // layered_choose; FPLDPC_LAYERED_TABLE=global / lds places it regardless
    if (tab_bytes && base + tab_bytes <= kLdsMax) {
        const char *table = getenv("FPLDPC_LAYERED_TABLE");
        if (table && (!strcmp(table, "lds") || !strcmp(table, "global")))
            lc.table_lds = !strcmp(table, "lds");
        else
            lc.table_lds = resident(base + tab_bytes) == resident(base);
        if (e != hipSuccess) return fail_hip(e, "layered min-sum kernel occupancy");
    }
    lc.lds_bytes = base + (lc.table_lds ? tab_bytes : 0);
    const int per_cu = resident(lc.lds_bytes);
    if (e != hipSuccess) return fail_hip(e, "layered min-sum kernel occupancy");
    if (per_cu < 1) return fail(FPLDPC_ERR_UNSUPPORTED, "layered min-sum kernel cannot be resident (occupancy 0)");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    lc.grid = per_cu * prop.multiProcessorCount;
    snprintf(lc.name, sizeof lc.name, "layered_minsum<DC=%d,addr=%s,deg=%s>", lc.dc,
             lc.computed ? "computed" : lc.table_lds ? "table" : "gtable", lc.exact ? "exact" : "table");
    *out = lc;
    return FPLDPC_OK;
}

int layered_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    if (args.batch <= 0) return FPLDPC_OK;
    const MinsumFn fn = minsum_fn(lc);
    if (!fn) return fail(FPLDPC_ERR_ARG, "layered min-sum decoder has no kernel");
    MinsumArgs ma;
    ma.a = args;
    ma.scale_16 = scale_16;
    ma.offset = offset;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fn, dim3(std::min(lc.grid, args.batch)), dim3(lc.threads), lc.lds_bytes, s, ma);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        // a launch that fails leaves the counter block for the next call to find non-zero: re-zero it
        (void)hipMemsetAsync(args.counters, 0, kLayeredCounterInts * sizeof(int32_t), s);
        return fail_hip(e, "layered min-sum kernel launch");
    }
    return FPLDPC_OK;
}

}  // namespace fpldpc
