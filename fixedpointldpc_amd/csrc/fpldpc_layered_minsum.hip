// fpldpc_layered_minsum.hip -- gfx950 (CDNA4) layered min-sum decoder with compressed check state
// (fpldpc_layered_create_minsum, include/fpldpc.h; DESIGN.md "Layered min-sum decoder").
//
// The schedule, the clamps and the frame framework are the saturated layered decoder's
// (fpldpc_layered.hip): persistent grid, one workgroup per frame, frames pulled from a work counter that
// the last workgroup out resets, lane j on check l*L + j, one barrier between layers, int16 posteriors in
// LDS.  The check rule is normalised / offset min-sum with 16 bytes of state per check, as
// fpldpc_minsum_device.hpp defines it; with its t[k] and new[k] a layer does
//     post[v_k] = clamp(t[k] + new[k], S_p)
// One state entry per check in LDS, lane j of a layer on entry l*L + j (one 16-byte access per lane,
// consecutive lanes on consecutive entries).  There is no per-edge c2v array for any code and, in the kernel
// of this unit, no global scratch: a code whose state does not fit LDS takes layered_minsum_global
// (fpldpc_minsum_global.hip), which layered_minsum_choose / layered_minsum_launch below delegate to.
//
// A check is a gather and two passes over its slots.  The gather issues every post[v_k] read before any
// is waited for and keeps v_k (uint16) and the posterior packed in one register per slot.  Pass 1 rebuilds
// the old message, puts t[k] (int16: |t| <= S_m < 2^15) in the posterior's place and tracks m1, m2, k1
// and the sign word.  Pass 2 emits new[k] and stores the posteriors.  No lane reads a posterior that
// another lane of its layer writes (no variable occurs twice inside a layer).
#include "fpldpc_layered_host.hpp"
#include "fpldpc_minsum_device.hpp"

namespace fpldpc {
namespace {

// bytes of the posteriors and control words, rounded up to the 16-byte alignment of the state entries
__host__ __device__ constexpr size_t ms_state_offset(int n) {
    return ((((size_t)n * sizeof(int16_t) + 3) / 4 + kLayMisc) * sizeof(int) + 15) / 16 * 16;
}

// LDS: post [n] int16 (up to a whole word) | misc [kLayMisc] | (to 16 bytes) state [m] uint4
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8
// DC / EXACT as layered_generic: the exact degree 47 in straight-line code, else the next of 8 / 16 / 32 /
// 48 / 64 with the slots predicated on the check's degree.  COMPUTED: forward array code, v = k*p +
// (j + i*k) mod p; else the index table (a.vidx, staged in LDS with a.table_lds).
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
        const int cw = lay_next_frame(a, misc);
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
                    MsSlots<COMPUTED> slots(vidx, m, p, c);
                    const MsMessages old(state[c]);
                    // gather: every read of the check in flight at once; pk[k] = v_k << 16 | (uint16) post[v_k]
                    uint32_t pk[DC];
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        pk[k] = 0;
                        if (k < deg) {
                            const uint32_t v = slots.next(k);
                            pk[k] = v << 16 | (uint16_t)post[v];
                        }
                    }
                    // pass 1: pk[k] becomes v_k << 16 | (uint16) t[k]
                    MsTrack track;
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if (k >= deg) continue;
                        const int t = lay_clamp((int)(int16_t)(pk[k] & 0xffffu) - old(k), Sm);
                        track.add(k, t);
                        pk[k] = (pk[k] & 0xffff0000u) | ((uint32_t)t & 0xffffu);
                    }
                    const MsMessages nw = track.finish(&state[c], ma);
                    // pass 2
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if (k >= deg) continue;
                        const int t = (int)(int16_t)(pk[k] & 0xffffu), v = (int)(pk[k] >> 16);
                        post[v] = (int16_t)lay_clamp(t + nw(k), Sp);
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
    lay_leave(a);
}

using MinsumFn = void (*)(MinsumArgs);
template <bool COMPUTED>
MinsumFn minsum_fn_of(int dc, bool exact) {
    return lay_for_dc(dc, exact, [](auto d, auto e) -> MinsumFn { return layered_minsum<decltype(d)::value, decltype(e)::value, COMPUTED>; });
}
MinsumFn minsum_fn(const LayeredChoice &lc) {
    return lc.computed ? minsum_fn_of<true>(lc.dc, lc.exact) : minsum_fn_of<false>(lc.dc, lc.exact);
}

}  // namespace

// Envelope: check degrees 2..255, any valid layer size and n <= 65535.  A code with a check degree above 64,
// and every code under FPLDPC_MINSUM_FORM=wide, takes the wide form (fpldpc_minsum_wide.hip).  Else the
// kernels of this unit where the
// int16 posteriors, the control words, 16 bytes per check and one byte per check of the degree table
// (unless the kernel's DC is every check's degree) fit the CU's 160 KiB of LDS; there the index table is
// placed as in layered_choose (FPLDPC_LAYERED_TABLE=global / lds places it regardless).  Every other code,
// and every code under FPLDPC_LAYERED_MINSUM_STATE=global, takes the global form (fpldpc_minsum_global.hip).
int layered_minsum_choose(const fpldpc_code &code, int L, int device, LayeredChoice *out) {
    if (code.dc_max > 64 || minsum_form_forced_wide())
        return minsum_wide_choose(code, kLayMinsum, std::min(kLayMaxNT, (L + 63) / 64 * 64), "FPLDPC_LAYERED_TABLE",
                                  minsum_state_forced_global("FPLDPC_LAYERED_MINSUM_STATE"), device, out);
    LayeredChoice lc;
    if (int st = lay_choice_of_code(code, kLayMinsum, "layered", &lc)) return st;
    lc.threads = std::min(kLayMaxNT, (L + 63) / 64 * 64);
    const size_t base = ms_state_offset(code.n) + kMsStateBytes * code.m + (lc.exact ? 0 : (size_t)code.m);
    if (base > kLdsMax || minsum_state_forced_global("FPLDPC_LAYERED_MINSUM_STATE")) {
        if (int st = minsum_global_choose(code, device, &lc)) return st;
    } else if (int st = lay_choose_lds(minsum_fn(lc), code, base, "FPLDPC_LAYERED_TABLE", device, "layered min-sum", "layered_minsum", &lc)) {
        return st;
    }
    *out = lc;
    return FPLDPC_OK;
}

int layered_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    if (lc.wide) return minsum_wide_launch(lc, args, scale_16, offset, stream);
    if (!lc.lds_state) return minsum_global_launch(lc, args, scale_16, offset, stream);
    return lay_launch(minsum_fn(lc), lc, args, MinsumArgs{args, scale_16, offset}, stream, "layered min-sum");
}

}  // namespace fpldpc
