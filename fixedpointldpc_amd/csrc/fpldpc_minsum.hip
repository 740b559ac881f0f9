// fpldpc_minsum.hip -- gfx950 (CDNA4) flooding min-sum decoder with compressed check state
// (fpldpc_minsum_create, include/fpldpc.h; DESIGN.md "Flooding min-sum decoder").
//
// The check rule, the clamps and the 16-byte check state are the layered min-sum decoder's, defined once in
// fpldpc_minsum_device.hpp; the schedule is flooding: within a step every check of the frame reads the
// same posteriors, so one lane takes one check over ALL m checks of the frame (A: 235 of 256 lanes), lanes
// loop where m exceeds the workgroup (R: 1128 checks), and there is no barrier inside a step.  With the
// rule's t[k] and new[k], per step
//     post'[v] = clamp(L[v] + sum of the new messages on v's edges, S_p)
//
// Posteriors are int32 accumulators in LDS, three buffers that rotate.  In step t the checks gather from
// `cur` (the reader clamps: post[v] = clamp(cur[v], S_p); the raw sum has the same sign), add new[k] into
// `nxt` with LDS integer atomics (order-free and exact), and every lane first refills `spare` with L[v]
// for step t + 1: nobody else touches it in this step.  Then one barrier, the syndrome on `nxt` (a second
// barrier), and the buffers rotate.  |L + sum| <= S_p + dv_max * S_m < 2^31: int32 is always enough.
// A check is the gather and the two passes of layered_minsum; pass 2 issues the atomics where the layered
// kernel stores posteriors.  There is no per-edge state, no per-variable pass and, in the kernels of this
// unit, no global scratch: a code whose state does not fit LDS takes flood_minsum_global
// (fpldpc_minsum_global.hip), which flood_minsum_choose / flood_minsum_launch below delegate to.
#include "fpldpc_layered_host.hpp"
#include "fpldpc_minsum_device.hpp"

namespace fpldpc {
namespace {

// bytes before the index table: state [m] uint4 | acc [3][n] int32 | llr [n] int16 (to a word) | misc
__host__ __device__ constexpr size_t fm_llr_offset(int n, int m) { return kMsStateBytes * (size_t)m + 3 * sizeof(int) * (size_t)n; }
__host__ __device__ constexpr size_t fm_misc_offset(int n, int m) {
    return fm_llr_offset(n, m) + ((size_t)n * sizeof(int16_t) + 3) / 4 * 4;
}
__host__ __device__ constexpr size_t fm_table_offset(int n, int m) { return fm_misc_offset(n, m) + kLayMisc * sizeof(int); }

// LDS: state [m] uint4 | acc [3][n] int32 | llr [n] int16 (up to a whole word) | misc [kLayMisc]
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8
// DC / EXACT / COMPUTED as layered_minsum: the exact degree 47 in straight-line code, else the next of
// 8 / 16 / 32 / 48 / 64 with the slots predicated on the check's degree; forward array codes compute
// v = k*p + (j + i*k) mod p, the others read the index table (a.vidx, staged in LDS with a.table_lds).
template <int DC, bool EXACT, bool COMPUTED>
__global__ void __launch_bounds__(kLayMaxNT) flood_minsum(MinsumArgs ma) {
    const LayeredArgs &a = ma.a;
    extern __shared__ __attribute__((aligned(16))) int fm_smem[];
    const int n = a.n, m = a.m, p = a.array_p;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    char *const smem = reinterpret_cast<char *>(fm_smem);
    uint4 *const state = reinterpret_cast<uint4 *>(smem);
    int *const acc = reinterpret_cast<int *>(smem + kMsStateBytes * (size_t)m);
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
        const int cw = lay_next_frame(a, misc);
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
                MsSlots<COMPUTED> slots(vidx, m, p, c);
                const MsMessages old(state[c]);
                // gather: every read of the check in flight at once; pk[k] = v_k << 16 | (uint16) post[v_k]
                uint32_t pk[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    pk[k] = 0;
                    if (k < deg) {
                        const uint32_t v = slots.next(k);
                        pk[k] = v << 16 | ((uint32_t)lay_clamp(acc[cur + (int)v], Sp) & 0xffffu);
                    }
                }
                // pass 1: t[k] into the minima and the sign word (pass 2 needs v_k only, not t[k])
                MsTrack track;
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k >= deg) continue;
                    track.add(k, lay_clamp((int)(int16_t)(pk[k] & 0xffffu) - old(k), Sm));
                }
                const MsMessages nw = track.finish(&state[c], ma);
                // pass 2: new[k] into the next step's accumulator
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k >= deg) continue;
                    atomicAdd(&acc[nxt + (int)(pk[k] >> 16)], nw(k));
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
    lay_leave(a);
}

using FloodMsFn = void (*)(MinsumArgs);
template <bool COMPUTED>
FloodMsFn flood_fn_of(int dc, bool exact) {
    return lay_for_dc(dc, exact, [](auto d, auto e) -> FloodMsFn { return flood_minsum<decltype(d)::value, decltype(e)::value, COMPUTED>; });
}
FloodMsFn flood_fn(const LayeredChoice &lc) {
    return lc.computed ? flood_fn_of<true>(lc.dc, lc.exact) : flood_fn_of<false>(lc.dc, lc.exact);
}

}  // namespace

// Envelope: check degrees 2..255 and n <= 65535.  A code with a check degree above 64, and every code under
// FPLDPC_MINSUM_FORM=wide, takes the wide form (fpldpc_minsum_wide.hip).  Else the kernels of this unit where the check state, three int32
// accumulators, the int16 LLRs, the control words and one byte per check of the degree table (unless the
// kernel's DC is every check's degree) fit the CU's 160 KiB of LDS; there the index table is placed as in
// the layered decoders, under a switch of its own (FPLDPC_MINSUM_TABLE=global / lds places it regardless).
// Every other code, and every code under FPLDPC_MINSUM_STATE=global, takes the global form
// (fpldpc_minsum_global.hip).
int flood_minsum_choose(const fpldpc_code &code, int device, LayeredChoice *out) {
    if (code.dc_max > 64 || minsum_form_forced_wide())
        return minsum_wide_choose(code, kFloodMinsum, std::min(kLayMaxNT, (code.m + 63) / 64 * 64), "FPLDPC_MINSUM_TABLE",
                                  minsum_state_forced_global("FPLDPC_MINSUM_STATE"), device, out);
    LayeredChoice lc;
    if (int st = lay_choice_of_code(code, kFloodMinsum, "flooding min-sum", &lc)) return st;
    lc.threads = std::min(kLayMaxNT, (code.m + 63) / 64 * 64);
    const size_t base = fm_table_offset(code.n, code.m) + (lc.exact ? 0 : (size_t)code.m);
    if (base > kLdsMax || code.n > 65535 || minsum_state_forced_global("FPLDPC_MINSUM_STATE")) {
        if (int st = minsum_global_choose(code, device, &lc)) return st;
    } else if (int st = lay_choose_lds(flood_fn(lc), code, base, "FPLDPC_MINSUM_TABLE", device, "flooding min-sum", "flood_minsum", &lc)) {
        return st;
    }
    *out = lc;
    return FPLDPC_OK;
}

int flood_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    if (lc.wide) return minsum_wide_launch(lc, args, scale_16, offset, stream);
    if (!lc.lds_state) return minsum_global_launch(lc, args, scale_16, offset, stream);
    return lay_launch(flood_fn(lc), lc, args, MinsumArgs{args, scale_16, offset}, stream, "flooding min-sum");
}

}  // namespace fpldpc
