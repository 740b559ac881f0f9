// fpldpc_minsum_global.hip -- gfx950 (CDNA4) "global" placement of the two min-sum decoders: the flooding
// (fpldpc_minsum.hip) and the layered one (fpldpc_layered_minsum.hip) for codes whose working set does not
// fit the CU's 160 KiB of LDS (DESIGN.md "Min-sum decoders: state off chip").
//
// Nothing of the definitions changes: the check rule and the 16-byte check state are
// fpldpc_minsum_device.hpp's, the frame framework (persistent grid, one workgroup per frame, work counter,
// syndrome, epilogue) is fpldpc_layered_device.hpp's, and the loops below are those of flood_minsum and
// layered_minsum.  What moves is where the state lives: LDS keeps the int16 vector of the frame (the
// clamped LLRs of the flooding decoder, the posteriors of the layered one; at most 131,070 B), the control
// words and, where it still fits, the degree table; the compressed check state -- and the three int32
// accumulators of the flooding decoder -- live in slice blockIdx.x of the decoder's scratch (d_scratch).
// Table addressing only, the index table in global memory (addr=gtable): a forward array code that is
// forced here reads the table too.
//
// Memory ordering.  A slice is touched by one workgroup only.  State entries and the layered decoder's
// posteriors are plain loads and stores ordered by __syncthreads().  The flooding accumulators are changed
// by integer atomics that return nothing and read again one step later, after a barrier, by other lanes
// of the same workgroup: those reads (the gather, the syndrome, the final clamp) are relaxed agent-scope
// atomic loads, so they are served where the atomics were performed and never by a line the CU's vector L1
// kept from an earlier read of the same buffer.  Plain stores (the refill with L, the final clamp) are
// complete at the barrier that follows them.
#include "fpldpc_layered_host.hpp"
#include "fpldpc_global_state.hpp"
#include "fpldpc_minsum_device.hpp"

namespace fpldpc {
namespace {

// The LDS layout, mg_round_slice, mg_degrees, fg_load and FgAcc: fpldpc_global_state.hpp.
// a workgroup's slice of the scratch.  Flooding: state [m] uint4 | acc [3][n] int32; layered: state [m] uint4
__host__ __device__ constexpr size_t fg_slice_bytes(int n, int m) {
    return mg_round_slice(kMsStateBytes * (size_t)m + 3 * sizeof(int) * (size_t)n);
}
__host__ __device__ constexpr size_t lg_slice_bytes(int m) { return mg_round_slice(kMsStateBytes * (size_t)m); }

// flood_minsum with its check state and accumulators in the workgroup's slice.  DC / EXACT as there.
template <int DC, bool EXACT>
__global__ void __launch_bounds__(kLayMaxNT) flood_minsum_global(MinsumArgs ma) {
    const LayeredArgs &a = ma.a;
    extern __shared__ __attribute__((aligned(16))) int mg_smem[];
    const int n = a.n, m = a.m;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    int16_t *const llr = reinterpret_cast<int16_t *>(mg_smem);
    int *const misc = mg_smem + mg_misc_word(n);
    const uint16_t *const vidx = a.vidx;
    const uint8_t *const cdeg = mg_degrees<EXACT>(a, mg_smem);
    char *const slice = static_cast<char *>(a.c2v_scratch) + (size_t)blockIdx.x * fg_slice_bytes(n, m);
    uint4 *const state = reinterpret_cast<uint4 *>(slice);
    int *const acc = reinterpret_cast<int *>(slice + kMsStateBytes * (size_t)m);

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
                MsSlots<false> slots(vidx, m, 0, c);
                const MsMessages old(state[c]);
                // gather: every read of the check in flight at once; pk[k] = v_k << 16 | (uint16) post[v_k]
                uint32_t pk[DC];
#pragma unroll
                for (int k = 0; k < DC; ++k) {
                    pk[k] = 0;
                    if (k < deg) {
                        const uint32_t v = slots.next(k);
                        pk[k] = v << 16 | ((uint32_t)lay_clamp(fg_load(&acc[cur + (int)v]), Sp) & 0xffffu);
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

// layered_minsum with its check state in the workgroup's slice.  DC / EXACT as there.
template <int DC, bool EXACT>
__global__ void __launch_bounds__(kLayMaxNT) layered_minsum_global(MinsumArgs ma) {
    const LayeredArgs &a = ma.a;
    extern __shared__ __attribute__((aligned(16))) int mg_smem[];
    const int n = a.n, m = a.m;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int Sp = a.sat_post, Sm = a.sat_msg;
    int16_t *const post = reinterpret_cast<int16_t *>(mg_smem);
    int *const misc = mg_smem + mg_misc_word(n);
    const uint16_t *const vidx = a.vidx;
    const uint8_t *const cdeg = mg_degrees<EXACT>(a, mg_smem);
    uint4 *const state = reinterpret_cast<uint4 *>(static_cast<char *>(a.c2v_scratch) + (size_t)blockIdx.x * lg_slice_bytes(m));

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
                    MsSlots<false> slots(vidx, m, 0, c);
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
MinsumFn global_fn(const LayeredChoice &lc) {
    if (lc.mode == kFloodMinsum)
        return lay_for_dc(lc.dc, lc.exact, [](auto d, auto e) -> MinsumFn { return flood_minsum_global<decltype(d)::value, decltype(e)::value>; });
    return lay_for_dc(lc.dc, lc.exact, [](auto d, auto e) -> MinsumFn { return layered_minsum_global<decltype(d)::value, decltype(e)::value>; });
}

}  // namespace

bool minsum_state_forced_global(const char *env) {
    const char *s = getenv(env);
    return s && !strcmp(s, "global");
}

// The rest of a min-sum decoder's choice in the global form, from the part the code decides (mode, dc,
// exact) and the workgroup size: the index table is built and stays in global memory, LDS is the int16
// vector, the control words and the degree table where it fits, the grid is the occupancy query's and the
// scratch one slice per workgroup.
int minsum_global_choose(const fpldpc_code &code, int device, LayeredChoice *lc) {
    const bool flood = lc->mode == kFloodMinsum;
    const char *who = flood ? "flooding min-sum" : "layered min-sum";
    if (code.n > 65535) return fail(FPLDPC_ERR_UNSUPPORTED, std::string(who) + " decoder: more than 65535 variables");
    lc->computed = false;
    lc->lds_state = false;
    lc->table_lds = false;
    lc->lds_bytes = mg_base_bytes(code.n) + (!lc->exact && mg_deg_in_lds(code.n, code.m) ? (size_t)code.m : 0);
    LayResidency<MinsumFn> resident{global_fn(*lc), lc->threads};
    const int per_cu = resident(lc->lds_bytes);
    if (int st = lay_grid(per_cu, resident.e, device, who, &lc->grid)) return st;
    lc->scratch_bytes = (size_t)lc->grid * (flood ? fg_slice_bytes(code.n, code.m) : lg_slice_bytes(code.m));
    snprintf(lc->name, sizeof lc->name, "%s<DC=%d,addr=gtable,deg=%s,mem=global>", flood ? "flood_minsum" : "layered_minsum",
             lc->dc, lc->exact ? "exact" : "table");
    return FPLDPC_OK;
}

int minsum_global_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream) {
    return lay_launch(global_fn(lc), lc, args, MinsumArgs{args, scale_16, offset}, stream,
                      lc.mode == kFloodMinsum ? "flooding min-sum" : "layered min-sum");
}

}  // namespace fpldpc
