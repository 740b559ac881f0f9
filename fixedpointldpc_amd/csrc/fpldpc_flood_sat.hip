// fpldpc_flood_sat.hip -- gfx950 (CDNA4) saturated flooding decoder with the reference's sxor fold
// (fpldpc_flood_create_sat, include/fpldpc.h; DESIGN.md "Saturated flooding decoder").
//
// The reference's own schedule and check rule -- flooding, the box-plus FP_Decoder::sxor in the serial
// forward/backward fold -- with posteriors post_bits wide and messages msg_bits wide: per frame
//     L[v] = clamp(LLR[v], S_p);  post[v] = L[v];  c2v[c][k] = 0
//     per step, for every check c, all reading the same post:
//         t[k] = clamp(post[v_k] - c2v[c][k], S_m);  new = fold(t);  c2v[c][k] = new[k]
//     post'[v] = clamp(L[v] + sum of the new messages on v's edges, S_p)
// Every fold value and every c2v is at most S_m + C <= 32767 (the creation rule), so the per-edge state is
// int16 whatever the widths.
//
// The schedule is flood_minsum's (fpldpc_minsum.hip): one lane per check over ALL m checks of the frame,
// lanes looping where m exceeds the workgroup, no barrier inside a step; posteriors are three rotating int32
// accumulators in LDS -- the checks gather from `cur` (the reader clamps; the raw sum has the posterior's
// sign), add new[k] into `nxt` with LDS integer atomics (order-free and exact), and every lane first refills
// `spare` with L[v] for the step after -- then one barrier, the syndrome on `nxt`, and the buffers rotate.
// |L + sum| <= S_p + dv_max * (S_m + C) < 2^31.  The check is layered_generic's (fpldpc_layered.hip): gather
// t[k], the backward chain, then the forward chain with the outputs.  A check's c2v column is only ever
// touched by the lane that owns the check: it needs no synchronisation of its own.
#include "fpldpc_layered_host.hpp"

namespace fpldpc {
namespace {

// bytes before the index table: c2v [dc_max][m] int16 (up to a whole word) | acc [3][n] int32
// | llr [n] int16 (up to a whole word) | misc
__host__ __device__ constexpr size_t fs_acc_offset(int dc_max, int m) { return ((size_t)dc_max * m * sizeof(int16_t) + 3) / 4 * 4; }
__host__ __device__ constexpr size_t fs_llr_offset(int n, int dc_max, int m) { return fs_acc_offset(dc_max, m) + 3 * sizeof(int) * (size_t)n; }
__host__ __device__ constexpr size_t fs_misc_offset(int n, int dc_max, int m) {
    return fs_llr_offset(n, dc_max, m) + ((size_t)n * sizeof(int16_t) + 3) / 4 * 4;
}
__host__ __device__ constexpr size_t fs_table_offset(int n, int dc_max, int m) { return fs_misc_offset(n, dc_max, m) + kLayMisc * sizeof(int); }

// t[k] of a packed slot word
__device__ __forceinline__ int fs_t(uint32_t pk) { return (int)(int16_t)(pk & 0xffffu); }
// x, as a value the compiler knows nothing about
__device__ __forceinline__ int fs_opaque(int x) {
    asm("" : "+v"(x));
    return x;
}

// LDS: c2v [dc_max][m] int16 (slot-major: a lane owns its check's column; up to a whole word)
//      | acc [3][n] int32 | llr [n] int16 (up to a whole word) | misc [kLayMisc]
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8
// DC / EXACT / COMPUTED as flood_minsum: the exact degree 47 in straight-line code, else the next of
// 8 / 16 / 32 / 48 / 64 with the slots predicated on the check's degree; forward array codes compute
// v = k*p + (j + i*k) mod p, the others read the index table (a.vidx, staged in LDS with a.table_lds).
template <int DC, bool EXACT, bool COMPUTED>
__global__ void __launch_bounds__(kLayMaxNT) flood_sat(LayeredArgs a) {
    extern __shared__ __attribute__((aligned(16))) int fs_smem[];
    const int n = a.n, m = a.m, p = a.array_p;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    char *const smem = reinterpret_cast<char *>(fs_smem);
    int16_t *const c2v = reinterpret_cast<int16_t *>(smem);
    int *const acc = reinterpret_cast<int *>(smem + fs_acc_offset(a.dc_max, m));
    int16_t *const llr = reinterpret_cast<int16_t *>(smem + fs_llr_offset(n, a.dc_max, m));
    int *const misc = reinterpret_cast<int *>(smem + fs_misc_offset(n, a.dc_max, m));
    const size_t edges = (size_t)a.dc_max * m;
    const uint16_t *vidx = COMPUTED ? nullptr : a.vidx;
    if (!COMPUTED && a.table_lds) {
        uint16_t *const lv = reinterpret_cast<uint16_t *>(smem + fs_table_offset(n, a.dc_max, m));
        for (int i = tid; i < (int)edges; i += NT) lv[i] = a.vidx[i];
        vidx = lv;
    }
    const uint8_t *cdeg = nullptr;
    if constexpr (!EXACT) {
        uint8_t *const ld = reinterpret_cast<uint8_t *>(smem + fs_table_offset(n, a.dc_max, m)) +
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
        __syncthreads();
        // the channel pre-check, as the other saturated decoders: 0 iterations, posteriors left untouched
        if (a.precheck && !lay_syndrome<DC, EXACT>(a, vidx, cdeg, llr)) {
            lay_store(a, cw, llr, false, 0, 1, misc);
            continue;
        }
        int iters = 0, fail = 1;
        for (int it = 1; it <= a.max_iter; ++it) {
            // the accumulator of step it + 1 starts at L (idle in this step: last read before the syndrome barrier)
            for (int v = tid; v < n; v += NT) acc[spare + v] = llr[v];
            // c2v = 0 before the first update: step 1 reads the column as it stands (the previous frame's) and drops it
            const int seen = it > 1 ? -1 : 0;
            for (int c = tid; c < m; c += NT) {
                const int deg = EXACT ? DC : (int)cdeg[c];
                int ci = 0, col = 0;
                if constexpr (COMPUTED) {
                    ci = c / p;
                    col = c - ci * p;
                }
                // gather: pk[k] = v_k << 16 | (uint16) t[k], |t[k]| <= S_m < 2^15
                uint32_t pk[DC];
                int e = c;  // the check's column of c2v (and of the index table), slot by slot
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    pk[k] = 0;
                    if (k < deg) {
                        uint32_t v;
                        if constexpr (COMPUTED) {
                            v = (uint32_t)(k * p + col);
                            col += ci;
                            col = (int)min((uint32_t)col, (uint32_t)(col - p));  // mod p (col < 2p), as MsSlots::next
                        } else {
                            v = vidx[e];
                        }
                        const int old = (int)c2v[e] & seen;
                        const int t = lay_clamp(lay_clamp(acc[cur + (int)v], Sp) - old, Sm);
                        pk[k] = (uint32_t)fs_opaque((int)(v << 16 | ((uint32_t)t & 0xffffu)));
                    }
                    e += m;
                }
                // forward / backward fold (ArrayLDPC_Decoder.cpp:83-116), the reference's order; every value
                // of either chain is at most S_m + C
                int B[DC];
                B[DC - 1] = fs_t(pk[DC - 1]);
#pragma unroll
                for (int k = DC - 2; k >= 1; --k) B[k] = k < deg - 1 ? lay_boxplus(B[k + 1], fs_t(pk[k]), a.C, a.mask) : fs_t(pk[k]);
                // The forward chain unpacks t[k] and walks the column again behind fs_opaque: what the backward
                // chain derived from them (|t|, the sign, every slot's address) would otherwise stay live across
                // both chains, several registers per slot.
                int F = fs_t(pk[0]);
                e = fs_opaque(c);
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    if (k < deg) {
                        const int bn = B[k + 1 < DC ? k + 1 : k];  // (unused in the last slot)
                        const int o = k == 0 ? bn : k == deg - 1 ? F : lay_boxplus(F, bn, a.C, a.mask);
                        if (k > 0) F = lay_boxplus(F, fs_opaque(fs_t(pk[k])), a.C, a.mask);
                        c2v[e] = (int16_t)o;  // |o| <= S_m + C <= 32767
                        atomicAdd(&acc[nxt + (int)(pk[k] >> 16)], o);
                    }
                    e += m;
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

using FloodSatFn = void (*)(LayeredArgs);
template <bool COMPUTED>
FloodSatFn flood_sat_fn_of(int dc, bool exact) {
    return lay_for_dc(dc, exact, [](auto d, auto e) -> FloodSatFn { return flood_sat<decltype(d)::value, decltype(e)::value, COMPUTED>; });
}
FloodSatFn flood_sat_fn(const LayeredChoice &lc) {
    return lc.computed ? flood_sat_fn_of<true>(lc.dc, lc.exact) : flood_sat_fn_of<false>(lc.dc, lc.exact);
}

}  // namespace

// Envelope: check degrees 2..64 and n <= 65535 in every placement.  The LDS form (FPLDPC_STATE_LDS) holds the
// whole state on chip: the int16 c2v of every edge, three int32 accumulators, the int16 LLRs, the control words
// and one byte per check of the degree table (unless the kernel's DC is every check's degree) within the CU's
// 160 KiB; its index table is placed as in the layered decoders, under a switch of its own
// (FPLDPC_FLOOD_SAT_TABLE=global / lds places it regardless).  FPLDPC_STATE_GLOBAL takes the global form
// (fpldpc_flood_sat_global.hip) for any code of the envelope, FPLDPC_STATE_AUTO the LDS form wherever its bytes
// fit -- the same choice as FPLDPC_STATE_LDS makes -- and the global form otherwise.
int flood_sat_choose(const fpldpc_code &code, int device, int state, LayeredChoice *out) {
    LayeredChoice lc;
    if (int st = lay_choice_of_code(code, kFloodSat, "saturated flooding", &lc)) return st;
    if (code.n > 65535) return fail(FPLDPC_ERR_UNSUPPORTED, "saturated flooding decoder: code length above 65535");
    lc.threads = std::min(kLayMaxNT, (code.m + 63) / 64 * 64);
    const size_t base = fs_table_offset(code.n, code.dc_max, code.m) + (lc.exact ? 0 : (size_t)code.m);
    if (state == FPLDPC_STATE_GLOBAL || (state == FPLDPC_STATE_AUTO && base > kLdsMax)) {
        if (int st = flood_sat_global_choose(code, device, &lc)) return st;
        *out = lc;
        return FPLDPC_OK;
    }
    if (base > kLdsMax)
        return fail(FPLDPC_ERR_UNSUPPORTED, "saturated flooding decoder: " + std::to_string(base) +
                                                " bytes of state (int16 c2v per edge, three int32 accumulators, the LLRs) do not fit 160 KiB of LDS"
                                                " (FPLDPC_STATE_GLOBAL or FPLDPC_STATE_AUTO of fpldpc_flood_create_sat_placed keeps them in global memory)");
    if (int st = lay_choose_lds(flood_sat_fn(lc), code, base, "FPLDPC_FLOOD_SAT_TABLE", device, "saturated flooding", "flood_sat", &lc))
        return st;
    *out = lc;
    return FPLDPC_OK;
}

int flood_sat_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream) {
    if (!lc.lds_state) return flood_sat_global_launch(lc, args, stream);
    return lay_launch(flood_sat_fn(lc), lc, args, args, stream, "saturated flooding");
}

}  // namespace fpldpc
