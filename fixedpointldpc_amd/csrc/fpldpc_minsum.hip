// fpldpc_minsum.hip -- gfx950 (CDNA4) flooding min-sum decoder with compressed check state
// (fpldpc_minsum_create, include/fpldpc.h; DESIGN.md "Flooding min-sum decoder").
//
// The check rule, the clamps and the 16-byte check state are the layered min-sum decoder's
// (fpldpc_layered_minsum.hip); the schedule is flooding: within a step every check of the frame reads the
// same posteriors, so one lane takes one check over ALL m checks of the frame (A: 235 of 256 lanes), lanes
// loop where m exceeds the workgroup (R: 1128 checks), and there is no barrier inside a step.  With
// f(x) = max(((x * scale_16) >> 4) - offset, 0), per step
//     t[k] = clamp(post[v_k] - c2v[c][k], S_m);  s[k] = t[k] <= 0
//     m1 = min |t|, k1 a slot attaining it, m2 = min over the other slots
//     new[k] = (parity of s over j != k) ? -f(k == k1 ? m2 : m1) : f(k == k1 ? m2 : m1)
//     c2v[c][k] = new[k];  post'[v] = clamp(L[v] + sum of the new messages on v's edges, S_p)
//
// Posteriors are int32 accumulators in LDS, three buffers that rotate.  In step t the checks gather from
// `cur` (the reader clamps: post[v] = clamp(cur[v], S_p); the raw sum has the same sign), add new[k] into
// `nxt` with LDS integer atomics (order-free and exact), and every lane first refills `spare` with L[v]
// for step t + 1: nobody else touches it in this step.  Then one barrier, the syndrome on `nxt` (a second
// barrier), and the buffers rotate.  |L + sum| <= S_p + dv_max * S_m < 2^31: int32 is always enough.
// A check is the gather and the two passes of layered_minsum; pass 2 issues the atomics where the layered
// kernel stores posteriors.  There is no per-edge state, no per-variable pass and no global scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fpldpc_layered_device.hpp"

namespace fpldpc {
namespace {

struct FloodMsArgs {
    LayeredArgs a;  // as the layered kernels read it (L, layers, C, mask and c2v_scratch unused)
    int scale_16 = 16, offset = 0;
};

constexpr size_t kFmStateBytes = 16;  // per check

// bytes before the index table: state [m] uint4 | acc [3][n] int32 | llr [n] int16 (to a word) | misc
__host__ __device__ constexpr size_t fm_llr_offset(int n, int m) { return kFmStateBytes * (size_t)m + 3 * sizeof(int) * (size_t)n; }
__host__ __device__ constexpr size_t fm_misc_offset(int n, int m) {
    return fm_llr_offset(n, m) + ((size_t)n * sizeof(int16_t) + 3) / 4 * 4;
}
__host__ __device__ constexpr size_t fm_table_offset(int n, int m) { return fm_misc_offset(n, m) + kLayMisc * sizeof(int); }

__device__ __forceinline__ int fm_correct(int x, int scale_16, int offset) { return max(((x * scale_16) >> 4) - offset, 0); }
// (x ^ neg) - neg: x for neg = 0, -x for neg = -1
__device__ __forceinline__ int fm_signed(int x, int neg) { return (x ^ neg) - neg; }
// -(bit k of the 64-bit word hi:lo) for a constant k: one signed bit-field extract
__device__ __forceinline__ int fm_neg_bit(uint32_t lo, uint32_t hi, int k) {
    return (int)((k < 32 ? lo : hi) << (31 - (k & 31))) >> 31;
}

// LDS: state [m] uint4 | acc [3][n] int32 | llr [n] int16 (up to a whole word) | misc [kLayMisc]
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8
// DC / EXACT / COMPUTED as layered_minsum: the exact degree 47 in straight-line code, else the next of
// 8 / 16 / 32 / 48 / 64 with the slots predicated on the check's degree; forward array codes compute
// v = k*p + (j + i*k) mod p, the others read the index table (a.vidx, staged in LDS with a.table_lds).
template <int DC, bool EXACT, bool COMPUTED>
__global__ void __launch_bounds__(kLayMaxNT) flood_minsum(FloodMsArgs fa) {
    const LayeredArgs &a = fa.a;
    extern __shared__ __attribute__((aligned(16))) int fm_smem[];
    const int n = a.n, m = a.m, p = a.array_p;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    char *const smem = reinterpret_cast<char *>(fm_smem);
    uint4 *const state = reinterpret_cast<uint4 *>(smem);
    int *const acc = reinterpret_cast<int *>(smem + kFmStateBytes * (size_t)m);
    int16_t *const llr = reinterpret_cast<int16_t *>(smem + fm_llr_offset(n, m));
    int *const misc = reinterpret_cast<int *>(smem + fm_misc_offset(n, m));
    const size_t edges = (size_t)a.dc_max * m;
    const uint16_t *vidx = COMPUTED ? nullptr : a.vidx;
    if (!COMPUTED && a.table_lds) {
        uint16_t *const lv = reinterpret_cast<uint16_t *>(smem + fm_table_offset(n, m));
        for (int i = tid; i < (int)edges; i += NT) lv[i] = a.vidx[i];
        vidx = lv;
    }
    const uint8_t *cdeg = nullptr;
    if constexpr (!EXACT) {
        uint8_t *const ld = reinterpret_cast<uint8_t *>(smem + fm_table_offset(n, m)) +
                            (!COMPUTED && a.table_lds ? edges * sizeof(uint16_t) : 0);
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
        // offsets into acc of the three accumulators: step 1 reads L from `cur` and adds into `nxt`
        int cur = 0, nxt = n, spare = 2 * n;
        for (int v = tid; v < n; v += NT) {
            const int x = lay_clamp(lay_load_llr(a, (size_t)cw * n + v), Sp);
            llr[v] = (int16_t)x;
            acc[cur + v] = x;
            acc[nxt + v] = x;
        }
        for (int c = tid; c < m; c += NT) state[c] = make_uint4(0, 0, 0, 0);  // every c2v = 0
        __syncthreads();
        // the channel pre-check, as the layered decoders: 0 iterations, posteriors left untouched
        if (a.precheck && !lay_syndrome<DC, EXACT>(a, vidx, cdeg, llr)) {
            lay_store(a, cw, llr, false, 0, 1, misc);
            continue;
        }
        int iters = 0, fail = 1;
        for (int it = 1; it <= a.max_iter; ++it) {
            // the accumulator of step it + 1 starts at L (idle in this step: last read before the syndrome barrier)
            for (int v = tid; v < n; v += NT) acc[spare + v] = llr[v];
            for (int c = tid; c < m; c += NT) {
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
                        pk[k] = v << 16 | ((uint32_t)lay_clamp(acc[cur + (int)v], Sp) & 0xffffu);
                    }
                }
                // pass 1: t[k] into the minima and the sign word (pass 2 needs v_k only, not t[k])
                int m1 = 0x7fff, m2 = 0x7fff, k1 = 0;
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k >= deg) continue;
                    const int old = fm_signed(k == ok1 ? oM2 : oM1, fm_neg_bit(olo, ohi, k));
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
                }
                const int M1 = fm_correct(m1, fa.scale_16, fa.offset), M2 = fm_correct(m2, fa.scale_16, fa.offset);
                state[c] = make_uint4((uint32_t)M1 | (uint32_t)M2 << 16, (uint32_t)k1, lo, hi);
                const uint32_t flip = 0u - (uint32_t)((__popc(lo) + __popc(hi)) & 1);
                lo ^= flip;  // bit k: new message k is negative
                hi ^= flip;
                // pass 2: new[k] into the next step's accumulator
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k >= deg) continue;
                    const int nw = fm_signed(k == k1 ? M2 : M1, fm_neg_bit(lo, hi, k));
                    atomicAdd(&acc[nxt + (int)(pk[k] >> 16)], nw);
                }
            }
            __syncthreads();  // every message of the step is in `nxt`
            fail = lay_syndrome<DC, EXACT>(a, vidx, cdeg, acc + nxt);  // the raw sum has the posterior's sign
            iters = it;
            if ((a.early_term && !fail) || it == a.max_iter) break;
            const int done = cur;
            cur = nxt;
            nxt = spare;
            spare = done;
        }
        // the frame's posteriors: the last step's accumulator, clamped in place
        for (int v = tid; v < n; v += NT) acc[nxt + v] = lay_clamp(acc[nxt + v], Sp);
        __syncthreads();
        lay_store(a, cw, acc + nxt, true, iters, !fail, misc);
    }
    // the last workgroup out resets the counter block for the next call (every workgroup has made
    // its last work-counter access, a returning atomic, before counting itself out)
    if (tid == 0 && atomicAdd(&a.counters[1], 1) == (int)gridDim.x - 1) {
        a.counters[0] = 0;
        a.counters[1] = 0;
    }
}

using FloodMsFn = void (*)(FloodMsArgs);
template <bool COMPUTED>
FloodMsFn flood_fn_of(int dc, bool exact) {
    if (exact) return flood_minsum<kExactDc, true, COMPUTED>;
    switch (dc) {
        case 8: return flood_minsum<8, false, COMPUTED>;
        case 16: return flood_minsum<16, false, COMPUTED>;
        case 32: return flood_minsum<32, false, COMPUTED>;
        case 48: return flood_minsum<48, false, COMPUTED>;
        case 64: return flood_minsum<64, false, COMPUTED>;
    }
    return nullptr;
}

FloodMsFn flood_fn(const LayeredChoice &lc) {
    return lc.computed ? flood_fn_of<true>(lc.dc, lc.exact) : flood_fn_of<false>(lc.dc, lc.exact);
}

}  // namespace

// Envelope: check degrees 2..64, and the check state, three int32 accumulators, the int16 LLRs, the control
// words and one byte per check of the degree table (unless the kernel's DC is every check's degree) within
// the CU's 160 KiB of LDS.
int flood_minsum_choose(const fpldpc_code &code, int device, LayeredChoice *out) {
    for (int r = 0; r < code.m; r++)
        if (code.cdeg[r] < 2) return fail(FPLDPC_ERR_UNSUPPORTED, "check of degree < 2 (reference behaviour undefined)");
    int dc = 0;
    for (int d : {8, 16, 32, 48, 64})
        if (!dc && code.dc_max <= d) dc = d;
    if (!dc) return fail(FPLDPC_ERR_UNSUPPORTED, "flooding min-sum decoder: check degree above 64");
    LayeredChoice lc;
    lc.mode = kFloodMinsum;
    lc.exact = code.regular_checks && code.dc_max == kExactDc;
    lc.dc = lc.exact ? kExactDc : dc;
    lc.computed = code.array_forward && code.array_p > 0;
    lc.lds_state = true;
    lc.threads = std::min(kLayMaxNT, (code.m + 63) / 64 * 64);
    const size_t base = fm_table_offset(code.n, code.m) + (lc.exact ? 0 : (size_t)code.m);
    if (base > kLdsMax || code.n > 65535)
        return fail(FPLDPC_ERR_UNSUPPORTED, "flooding min-sum decoder: accumulators and check state do not fit 160 KiB of LDS");
    const size_t tab_bytes = lc.computed ? 0 : (size_t)code.dc_max * code.m * sizeof(uint16_t);
    const FloodMsFn fn = flood_fn(lc);
    hipError_t e = hipSuccess;
    auto resident = [&](size_t lds) {
        int per_cu = 0;
        if (e == hipSuccess && lds > 64 * 1024) e = raise_dynamic_lds((const void *)fn, lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, lc.threads, lds);
        return e == hipSuccess ? per_cu : 0;
    };
    // the index table joins the state in LDS only where that costs no resident workgroup, as in the
    // layered decoders; FPLDPC_MINSUM_TABLE=global / lds places it regardless
    if (tab_bytes && base + tab_bytes <= kLdsMax) {
        const char *table = getenv("FPLDPC_MINSUM_TABLE");
        if (table && (!strcmp(table, "lds") || !strcmp(table, "global")))
            lc.table_lds = !strcmp(table, "lds");
        else
            lc.table_lds = resident(base + tab_bytes) == resident(base);
        if (e != hipSuccess) return fail_hip(e, "flooding min-sum kernel occupancy");
    }
    lc.lds_bytes = base + (lc.table_lds ? tab_bytes : 0);
    const int per_cu = resident(lc.lds_bytes);
    if (e != hipSuccess) return fail_hip(e, "flooding min-sum kernel occupancy");
    if (per_cu < 1) return fail(FPLDPC_ERR_UNSUPPORTED, "flooding min-sum kernel cannot be resident (occupancy 0)");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    lc.grid = per_cu * prop.multiProcessorCount;
    snprintf(lc.name, sizeof lc.name, "flood_minsum<DC=%d,addr=%s,deg=%s>", lc.dc,
             lc.computed ? "computed" : lc.table_lds ? "table" : "gtable", lc.exact ? "exact" : "table");
    *out = lc;
    return FPLDPC_OK;
}

int flood_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    if (args.batch <= 0) return FPLDPC_OK;
    const FloodMsFn fn = flood_fn(lc);
    if (!fn) return fail(FPLDPC_ERR_ARG, "flooding min-sum decoder has no kernel");
    FloodMsArgs fa;
    fa.a = args;
    fa.scale_16 = scale_16;
    fa.offset = offset;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fn, dim3(std::min(lc.grid, args.batch)), dim3(lc.threads), lc.lds_bytes, s, fa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        // a launch that fails leaves the counter block for the next call to find non-zero: re-zero it
        (void)hipMemsetAsync(args.counters, 0, kLayeredCounterInts * sizeof(int32_t), s);
        return fail_hip(e, "flooding min-sum kernel launch");
    }
    return FPLDPC_OK;
}

}  // namespace fpldpc
