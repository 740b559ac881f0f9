// fpldpc_flood_sat_global.hip -- gfx950 (CDNA4) "global" placement of the saturated flooding decoder
// (fpldpc_flood_sat.hip; fpldpc_flood_create_sat_placed with FPLDPC_STATE_GLOBAL / _AUTO, include/fpldpc.h;
// DESIGN.md "Saturated flooding decoder: state off chip"), for codes whose int16 c2v per edge and three int32
// accumulators do not fit the CU's 160 KiB of LDS.
//
// Nothing of the definition changes: the loop below is flood_sat's (gather, the backward chain B[DC], the
// forward chain with the outputs, fs_opaque, the first step's `c2v & seen` in place of a clear) and the frame
// framework is fpldpc_layered_device.hpp's.  What moves is where the state lives, as in flood_minsum_global
// (fpldpc_minsum_global.hip): LDS keeps the clamped int16 LLRs, the control words and, where it still fits,
// the degree table; c2v and the accumulators live in slice blockIdx.x of the decoder's scratch (d_scratch).
// Table addressing only, the index table in global memory (addr=gtable): a forward array code that lands
// here reads the table too.
//
// Memory ordering.  A slice is touched by one workgroup only.  A check's c2v column is read and written only by
// the lane that owns the check: plain loads and stores, and the scratch is never cleared (step 1 masks what it
// reads).  The accumulators are changed by integer atomics that return nothing and read again one step later,
// after a barrier, by other lanes of the same workgroup: those reads (the gather, the syndrome, the final
// clamp) are relaxed agent-scope atomic loads, so they are served where the atomics were performed and never
// by a line the CU's vector L1 kept from an earlier read of the same buffer.  Plain stores (the refill with L,
// the final clamp) are complete at the barrier that follows them.
#include "fpldpc_layered_host.hpp"
#include "fpldpc_global_state.hpp"

namespace fpldpc {
namespace {

// a workgroup's slice of the scratch: c2v [dc_max][m] int16 (slot-major, up to a whole word) | acc [3][n] int32
__host__ __device__ constexpr size_t fsg_acc_offset(int dc_max, int m) { return ((size_t)dc_max * m * sizeof(int16_t) + 3) / 4 * 4; }
__host__ __device__ constexpr size_t fsg_slice_bytes(int n, int dc_max, int m) {
    return mg_round_slice(fsg_acc_offset(dc_max, m) + 3 * sizeof(int) * (size_t)n);
}

// t[k] of a packed slot word
__device__ __forceinline__ int fs_t(uint32_t pk) { return (int)(int16_t)(pk & 0xffffu); }
// x, as a value the compiler knows nothing about
__device__ __forceinline__ int fs_opaque(int x) {
    asm("" : "+v"(x));
    return x;
}

// flood_sat with c2v and the accumulators in the workgroup's slice.  DC / EXACT as there.
// LDS: llr [n] int16 (up to a whole word) | misc [kLayMisc] | (!EXACT, where it fits) cdeg [m] uint8
template <int DC, bool EXACT>
__global__ void __launch_bounds__(kLayMaxNT) flood_sat_global(LayeredArgs a) {
    extern __shared__ __attribute__((aligned(16))) int fsg_smem[];
    const int n = a.n, m = a.m;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    int16_t *const llr = reinterpret_cast<int16_t *>(fsg_smem);
    int *const misc = fsg_smem + mg_misc_word(n);
    const uint16_t *const vidx = a.vidx;
    const uint8_t *const cdeg = mg_degrees<EXACT>(a, fsg_smem);
    char *const slice = static_cast<char *>(a.c2v_scratch) + (size_t)blockIdx.x * fsg_slice_bytes(n, a.dc_max, m);
    int16_t *const c2v = reinterpret_cast<int16_t *>(slice);
    int *const acc = reinterpret_cast<int *>(slice + fsg_acc_offset(a.dc_max, m));

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
            // c2v = 0 before the first update: step 1 reads the column as it stands (the previous frame's, or what
            // the allocation held) and drops it
            const int seen = it > 1 ? -1 : 0;
            for (int c = tid; c < m; c += NT) {
                const int deg = EXACT ? DC : (int)cdeg[c];
                // gather: pk[k] = v_k << 16 | (uint16) t[k], |t[k]| <= S_m < 2^15
                uint32_t pk[DC];
                int e = c;  // the check's column of c2v (and of the index table), slot by slot
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    pk[k] = 0;
                    if (k < deg) {
                        const uint32_t v = vidx[e];
                        const int old = (int)c2v[e] & seen;
                        const int t = lay_clamp(lay_clamp(fg_load(&acc[cur + (int)v]), Sp) - old, Sm);
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
                // The forward chain unpacks t[k] and walks the column again behind fs_opaque, as flood_sat's.
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
            // the raw sum has the posterior's sign
            fail = lay_syndrome<DC, EXACT>(a, vidx, cdeg, reinterpret_cast<const FgAcc *>(acc + nxt));
            iters = it;
            if ((a.early_term && !fail) || it == a.max_iter) break;
            const int done = cur;
            cur = nxt;
            nxt = spare;
            spare = done;
        }
        // the frame's posteriors: the last step's accumulator, clamped in place
        for (int v = tid; v < n; v += NT) acc[nxt + v] = lay_clamp(fg_load(&acc[nxt + v]), Sp);
        __syncthreads();
        lay_store(a, cw, acc + nxt, true, iters, !fail, misc);
    }
    lay_leave(a);
}

using FloodSatFn = void (*)(LayeredArgs);
FloodSatFn global_fn(const LayeredChoice &lc) {
    return lay_for_dc(lc.dc, lc.exact, [](auto d, auto e) -> FloodSatFn { return flood_sat_global<decltype(d)::value, decltype(e)::value>; });
}

}  // namespace

// The rest of the saturated flooding decoder's choice in the global form, from the part the code decides (mode,
// dc, exact) and the workgroup size, as minsum_global_choose: the index table is built and stays in global
// memory, LDS is the int16 LLRs, the control words and the degree table where it fits, the grid is the
// occupancy query's and the scratch one slice per workgroup.
int flood_sat_global_choose(const fpldpc_code &code, int device, LayeredChoice *lc) {
    lc->computed = false;
    lc->lds_state = false;
    lc->table_lds = false;
    lc->lds_bytes = mg_base_bytes(code.n) + (!lc->exact && mg_deg_in_lds(code.n, code.m) ? (size_t)code.m : 0);
    LayResidency<FloodSatFn> resident{global_fn(*lc), lc->threads};
    const int per_cu = resident(lc->lds_bytes);
    if (int st = lay_grid(per_cu, resident.e, device, "saturated flooding", &lc->grid)) return st;
    lc->scratch_bytes = (size_t)lc->grid * fsg_slice_bytes(code.n, code.dc_max, code.m);
    snprintf(lc->name, sizeof lc->name, "flood_sat<DC=%d,addr=gtable,deg=%s,mem=global>", lc->dc, lc->exact ? "exact" : "table");
    return FPLDPC_OK;
}

int flood_sat_global_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream) {
    return lay_launch(global_fn(lc), lc, args, args, stream, "saturated flooding");
}

}  // namespace fpldpc
