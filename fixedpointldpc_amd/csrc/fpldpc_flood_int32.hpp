// fpldpc_flood_int32.hpp -- the exact int32 flooding kernels: flood_reg (c2v in registers), flood_gmem
// (c2v in a global scratch), flood_edges (the stateful single-frame decode) and flood_array (array
// codes, computed addressing, sign/magnitude fold).  They are every code's general path and the last
// link of the packed kernels' fallback chains.  Included by fpldpc_kernels.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpldpc_flood_device.hpp"

namespace fpldpc {
namespace {

// OR over the workgroup of a per-thread flag through a zeroed control word in the dynamic LDS, one
// barrier.  (__syncthreads_or keeps 256 bytes of static LDS, which come out of the same 160 KiB as the
// posteriors: with it the longest code was n = 10,219, not the 10,235 choose_kernel's length test admits.)
__device__ __forceinline__ int block_or(int flag, int *word) {
    if (__ballot(flag) && (threadIdx.x & 63) == 0) atomicOr(word, 1);
    __syncthreads();
    return *word;
}
// The same for step `it` of a frame, over the rotating flag words misc[2..4] (as flood_lds16 and flood_pk
// do): thread 0 zeroes the next step's word before this step's barrier -- its last readers, at step
// it - 2, have passed the barrier of step it - 1 -- so a step costs one barrier.  All three words are
// zeroed at the frame pull.
__device__ __forceinline__ int step_or(int fail, int *misc, int it) {
    if (threadIdx.x == 0) misc[2 + (it + 1) % 3] = 0;
    return block_or(fail, &misc[2 + it % 3]);
}

// Register-resident variant: CPL checks per lane (check c = tid + q*kNT), c2v and the packed
// var indices of each check held in VGPRs for the lifetime of the workgroup.
template <int DC, int CPL, bool REGULAR>
__global__ void __launch_bounds__(kNT) flood_reg(KArgs a) {
    if (empty_list(a)) return;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int n = a.n;
    int *const bufs = smem;          // 3 x n posterior buffers
    int *const llr_s = smem + 3 * n; // n
    int *const misc = smem + 4 * n;  // [0] frame slot, [1] bit-error accumulator
    const int tid = threadIdx.x;

    constexpr int DP = (DC + 1) / 2;
    uint32_t vpk[CPL][DP];
    int deg[CPL];
    bool act[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        const int c = tid + q * kNT;
        act[q] = c < a.m;
        deg[q] = act[q] ? (REGULAR ? DC : (int)a.cdeg[c]) : 0;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
            uint32_t lo = 0, hi = 0;
            if (act[q]) {
                lo = a.vidx[(size_t)(2 * j) * a.m_pad + c];
                if (2 * j + 1 < DC) hi = a.vidx[(size_t)(2 * j + 1) * a.m_pad + c];
            }
            vpk[q][j] = lo | (hi << 16);
        }
    }

    for (;;) {
        __syncthreads();
        if (tid == 0) {
            misc[0] = pull_frame(a, a.work_counter);
            misc[1] = 0;
            misc[2] = misc[3] = misc[4] = 0;  // (step_or's flag words)
        }
        __syncthreads();
        const int cw = misc[0];
        if (cw < 0) break;
        frame_load(a, cw, bufs, llr_s);
        int c2v[CPL][DC];
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int k = 0; k < DC; ++k) c2v[q][k] = 0;
        __syncthreads();

        int cur = 0;
        const int *pf = nullptr;
        bool pre = false;
        int iters = 0, ok = 0;
        for (int it = 1;; ++it) {
            const bool update = it <= a.max_iter;
            const int *pc = bufs + cur * n;
            int *pn = bufs + ((cur + 1) % 3) * n;
            int *pr = bufs + ((cur + 2) % 3) * n;
            if (update)
                for (int v = tid; v < n; v += kNT) pr[v] = llr_s[v];
            int fail = 0;
#pragma unroll
            for (int q = 0; q < CPL; ++q)
                if (act[q]) fail |= check_update<DC, REGULAR>(c2v[q], vpk[q], deg[q], pc, pn, update, a.C, a.mask);
            fail = step_or(fail, misc, it);
            const int done = it - 1;
            if (done == 0 && a.precheck && !fail) {
                pf = llr_s;
                pre = true;
                iters = 0;
                ok = 1;
                break;
            }
            if ((done >= 1 && a.early_term && !fail) || done >= a.max_iter) {
                pf = pc;
                iters = done;
                ok = !fail;
                break;
            }
            cur = (cur + 1) % 3;
        }
        frame_store(a, cw, pf, !pre, iters, ok, misc);
    }
    chain_exit(a);
}

// Global-scratch variant for codes whose c2v state does not fit the register budget: checks
// strided over the lanes, c2v in a per-workgroup scratch [DC][m_pad] (coalesced per slot), var
// indices read from the [DC][m_pad] table (L1/L2 resident).
template <int DC>
__device__ __forceinline__ int check_update_gmem(int c, int deg, int m_pad, const uint16_t *vidx, int32_t *c2vs,
                                                 bool first, const int *pc, int *pn, bool update, int C, int mask) {
    int m[DC];
    int vi[DC];
    int par = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        vi[k] = vidx[(size_t)k * m_pad + c];
        const int p = pc[vi[k]];
        if (k < deg) par ^= (p <= 0) ? 1 : 0;
        m[k] = first ? p : p - c2vs[(size_t)k * m_pad + c];
    }
    if (!update) return par;
    int B[DC];
    B[DC - 1] = m[DC - 1];
#pragma unroll
    for (int k = DC - 2; k >= 1; --k) {
        const int bk = boxplus(B[k + 1], m[k], C, mask);
        B[k] = (k < deg - 1) ? bk : m[k];
    }
    int F = m[0];
    int out[DC];
    out[0] = B[1];
#pragma unroll
    for (int k = 1; k <= DC - 2; ++k) {
        const int o = boxplus(F, B[k + 1], C, mask);
        out[k] = (k < deg - 1) ? o : F;
        F = boxplus(F, m[k], C, mask);
    }
    out[DC - 1] = F;
#pragma unroll
    for (int k = 0; k < DC; ++k)
        if (k < deg) {
            c2vs[(size_t)k * m_pad + c] = out[k];
            lds_add(pn + vi[k], out[k]);
        }
    return par;
}

template <int DC>
__global__ void __launch_bounds__(kNT) flood_gmem(KArgs a) {
    if (empty_list(a)) return;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int n = a.n;
    int *const bufs = smem;
    int *const llr_s = smem + 3 * n;
    int *const misc = smem + 4 * n;
    const int tid = threadIdx.x;
    int32_t *const c2vs = a.c2v_scratch + (size_t)blockIdx.x * DC * a.m_pad;

    for (;;) {
        __syncthreads();
        if (tid == 0) {
            misc[0] = pull_frame(a, a.work_counter);
            misc[1] = 0;
            misc[2] = misc[3] = misc[4] = 0;  // (step_or's flag words)
        }
        __syncthreads();
        const int cw = misc[0];
        if (cw < 0) break;
        frame_load(a, cw, bufs, llr_s);
        __syncthreads();

        int cur = 0;
        const int *pf = nullptr;
        bool pre = false;
        int iters = 0, ok = 0;
        for (int it = 1;; ++it) {
            const bool update = it <= a.max_iter;
            const int *pc = bufs + cur * n;
            int *pn = bufs + ((cur + 1) % 3) * n;
            int *pr = bufs + ((cur + 2) % 3) * n;
            if (update)
                for (int v = tid; v < n; v += kNT) pr[v] = llr_s[v];
            int fail = 0;
            for (int c = tid; c < a.m; c += kNT)
                fail |= check_update_gmem<DC>(c, a.cdeg[c], a.m_pad, a.vidx, c2vs, it == 1, pc, pn, update, a.C, a.mask);
            fail = step_or(fail, misc, it);
            const int done = it - 1;
            if (done == 0 && a.precheck && !fail) {
                pf = llr_s;
                pre = true;
                iters = 0;
                ok = 1;
                break;
            }
            if ((done >= 1 && a.early_term && !fail) || done >= a.max_iter) {
                pf = pc;
                iters = done;
                ok = !fail;
                break;
            }
            cur = (cur + 1) % 3;
        }
        frame_store(a, cw, pf, !pre, iters, ok, misc);
    }
    chain_exit(a);
}

// ------------------------------------------------------------------------------------------
// Stateful single-frame decode: the reference's edge RAM kept across calls.  Between calls
// FP_Decoder's EdgeRAM (ArrayLDPCMacro.h:162) holds the v2c message of every edge as the last
// variable-node phase wrote it (accum - c2v, ArrayLDPC_Decoder.cpp:152, :615).  decode_general_fp,
// and decode_fixpoint in state PCV, first overwrite it with the channel values (:45-61, :462-485);
// decode_fixpoint in state C2V skips that and iterates from what the previous frame left (:488-618),
// the new LLRs entering in the variable-node phase.  `edge` is that RAM, edge[k * m + c] = slot k of
// check c (clist order, the code's own check order), owned by the caller; the first update reads its
// v2c from it (keep = 1) or from the LLRs (keep = 0), later updates from post - c2v.  The c2v of the
// last two updates sit in a global double buffer, so the RAM written back at the end is the one that
// belongs to the returned posteriors: pf[var] - c2v of update `done`.  The pre-check (:443-450) runs
// before anything touches the RAM and leaves it as it was.  One workgroup, one frame: this is the
// per-frame drop-in path (include/fpldpc_compat.hpp), not the batch kernels.
struct EdgeArgs {
    const uint16_t *vidx;  // [DC][m] var of slot k of check c (clist order)
    const uint8_t *cdeg;   // [m]
    int32_t *edge;         // [dc_max][m] edge RAM (v2c), in/out
    int32_t *c2v;          // [2][DC][m] scratch
    int keep;              // 1: iterate from `edge` (state C2V); 0: edge init from the channel values
    int dc_max;            // rows of vidx / edge (the code's largest check degree)
};

// LDS = true (when it fits, edge_lds_bytes): the c2v double buffer and the index table live in LDS
// after the posteriors instead of global memory -- A and W (R's 1128 x 47 edges do not fit).
template <int DC, bool LDS>
__global__ void __launch_bounds__(kNT) flood_edges(KArgs a, EdgeArgs e) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int n = a.n, m = a.m;
    int *const bufs = smem;
    int *const llr_s = smem + 3 * n;
    int *const misc = smem + 4 * n;
    const int tid = threadIdx.x;
    int32_t *const c2v = LDS ? smem + 4 * n + kMiscInts : e.c2v;
    const uint16_t *vidx = e.vidx;
    if constexpr (LDS) {
        uint16_t *const lv = reinterpret_cast<uint16_t *>(smem + 4 * n + kMiscInts + 2 * DC * m);
        for (int i = tid; i < e.dc_max * m; i += kNT) lv[i] = e.vidx[i];
        vidx = lv;
    }
    for (int v = tid; v < n; v += kNT) {
        const int x = load_llr(a, v);
        llr_s[v] = x;
        bufs[n + v] = x;  // posteriors of update 1: LLR + sum c2v
    }
    if (tid == 0) misc[1] = misc[2] = misc[3] = misc[4] = misc[5] = 0;  // bit errors; step_or's words; the pre-check's
    __syncthreads();
    if (a.precheck) {  // hardDecision(LLR) (:270-294): a passing channel syndrome returns 0
        int fail = 0;
        for (int c = tid; c < m; c += kNT) {
            int par = 0;
            for (int k = 0; k < e.cdeg[c]; ++k) par ^= llr_s[vidx[(size_t)k * m + c]] <= 0;
            fail |= par;
        }
        if (!block_or(fail, &misc[5])) {
            frame_store(a, 0, llr_s, false, 0, 1, misc);
            return;
        }
    }
    int cur = 0, iters = 0, ok = 0;
    const int *pf = nullptr;
    for (int it = 1;; ++it) {
        const bool update = it <= a.max_iter;
        const int *pc = bufs + cur * n;
        int *pn = bufs + ((cur + 1) % 3) * n;
        int *pr = bufs + ((cur + 2) % 3) * n;
        if (update)
            for (int v = tid; v < n; v += kNT) pr[v] = llr_s[v];
        const int32_t *c2r = c2v + (size_t)((it - 1) & 1) * DC * m;  // c2v of update it - 1
        int32_t *c2w = c2v + (size_t)(it & 1) * DC * m;               // c2v of update it
        int fail = 0;
        for (int c = tid; c < m; c += kNT) {
            const int deg = e.cdeg[c];
            int mv[DC], vi[DC];
            int par = 0;
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                vi[k] = 0;
                mv[k] = 0;
                if (k < deg) {
                    vi[k] = vidx[(size_t)k * m + c];
                    const int p = pc[vi[k]];
                    par ^= p <= 0;
                    mv[k] = it > 1 ? p - c2r[(size_t)k * m + c] : e.keep ? e.edge[(size_t)k * m + c] : llr_s[vi[k]];
                }
            }
            if (it > 1) fail |= par;  // syndrome of the posteriors after it - 1 updates (:164, :621)
            if (!update) continue;
            // forward / backward fold (:83-116), the reference's order
            int B[DC];
            B[DC - 1] = mv[DC - 1];
#pragma unroll
            for (int k = DC - 2; k >= 1; --k) B[k] = k < deg - 1 ? boxplus(B[k + 1], mv[k], a.C, a.mask) : mv[k];
            int F = mv[0];
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                if (k >= deg) continue;
                const int o = k == 0 ? B[1] : k == deg - 1 ? F : boxplus(F, B[k + 1], a.C, a.mask);
                if (k > 0) F = boxplus(F, mv[k], a.C, a.mask);
                c2w[(size_t)k * m + c] = o;
                lds_add(pn + vi[k], o);  // post' = LLR + sum c2v' (:131-144)
            }
        }
        fail = step_or(fail, misc, it);
        const int done = it - 1;
        if ((done >= 1 && a.early_term && !fail) || done >= a.max_iter) {
            pf = pc;
            iters = done;
            ok = !fail;
            break;
        }
        cur = (cur + 1) % 3;
    }
    // the edge RAM after the last variable-node phase: v2c = post - c2v of update `done`
    const int32_t *c2d = c2v + (size_t)(iters & 1) * DC * m;
    for (int c = tid; c < m; c += kNT)
        for (int k = 0; k < e.cdeg[c]; ++k)
            e.edge[(size_t)k * m + c] = pf[vidx[(size_t)k * m + c]] - c2d[(size_t)k * m + c];
    frame_store(a, 0, pf, true, iters, ok, misc);
}

// ------------------------------------------------------------------------------------------
// Sign/magnitude kernels.  Box-plus splits exactly into a magnitude chain and a sign parity:
//   |x [+] y| = bp_mag(|x|, |y|), sign = XOR of the (v <= 0) flags,
// because a zero magnitude absorbs (bp_mag(0, b) = 0, so the sgn(0) = -1 rule of
// ArrayLDPCMacro.h:222-224 can only ever multiply a zero).  The serial fold ORDER of the
// magnitudes is kept exactly as the reference's (ArrayLDPC_Decoder.cpp:83-116); only the sign
// bookkeeping leaves the chain: one parity S per check, c2v_k sign = S ^ neg(m_k).
// tests/test_oracle.py::test_sign_split checks this against the reference's sxor fold: pairs
// exhaustively on [-1024, 1024]^2, whole checks of degree 47 and 8 on random v2c, bp_mag2's packed
// arithmetic per half, for every mask 2^w - 1 (w = 2..16) the packed kernels accept.
__device__ __forceinline__ uint32_t bp_mag(uint32_t a, uint32_t b, uint32_t C, uint32_t w) {
    const uint32_t mn = min(a, b);
    const uint32_t mx = max(a, b);
    const uint32_t t1 = __builtin_amdgcn_ubfe(a + b, 2, w);   // ((a+b) & mask) >> 2
    const uint32_t t2 = __builtin_amdgcn_ubfe(mx - mn, 2, w);  // (|a-b| & mask) >> 2
    // min + max(0, C - t1) - max(0, C - t2) = min + min(C, t2) - min(C, t1)
    return mn + min(C, t2) - min(C, t1);
}

__device__ __forceinline__ uint32_t iabs(int x) { return (uint32_t)(x < 0 ? -x : x); }

// Array codes (ROM::CirShift = (i*k) mod p, ArrayLDPCMacro.h:57; H_array_p*_forward.txt): check
// (i, j) = i*P + j connects var k*P + (j + i*k) mod P, k = 0..P-1, so the gather address is
// computed (one add + one min per edge, the k*P part folds into the LDS instruction offset) and no
// index table is read.  One lane per check (m = r*P <= 256), c2v state in VGPRs.
template <int P>
__global__ void __launch_bounds__(kNT, 4) flood_array(KArgs a) {
    if (empty_list(a)) return;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int n = a.n;
    int *const bufs = smem;
    int *const llr_s = smem + 3 * n;
    int *const misc = smem + 4 * n;
    const int tid = threadIdx.x;
    const bool act = tid < a.m;
    const uint32_t row = act ? (uint32_t)(tid / P) : 0u, col = act ? (uint32_t)(tid % P) : 0u;
    const uint32_t C = (uint32_t)a.C, w = a.bfe_w;

    for (;;) {
        __syncthreads();
        if (tid == 0) {
            misc[0] = pull_frame(a, a.work_counter);
            misc[1] = 0;
            misc[2] = misc[3] = misc[4] = 0;  // (step_or's flag words)
        }
        __syncthreads();
        const int cw = misc[0];
        if (cw < 0) break;
        frame_load(a, cw, bufs, llr_s);
        int st[P];  // c2v between iterations; v2c (m) inside the update
#pragma unroll
        for (int k = 0; k < P; ++k) st[k] = 0;
        __syncthreads();

        int cur = 0;
        const int *pf = nullptr;
        bool pre = false;
        int iters = 0, ok = 0;
        for (int it = 1;; ++it) {
            const bool update = it <= a.max_iter;
            const int *pc = bufs + cur * n;
            int *pn = bufs + ((cur + 1) % 3) * n;
            int *pr = bufs + ((cur + 2) % 3) * n;
            if (update)
                for (int v = tid; v < n; v += kNT) pr[v] = llr_s[v];
            int fail = 0;
            if (act) {
                // gather posteriors; v2c = post - c2v (ArrayLDPC_Decoder.cpp:143-152); syndrome
                // parity of the hard decisions post > 0 ? 0 : 1 (:305-308); sign parity S
                // (opaque start: the compiler would otherwise hoist all P loop-invariant
                // addresses out of the iteration loop and keep them in registers)
                uint32_t t = col;
                asm volatile("" : "+v"(t));
                bool par = false, S = false;
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const int p = pc[k * P + t];
                    par ^= p <= 0;
                    st[k] = p - st[k];
                    S ^= st[k] <= 0;
                    t += row;
                    t = min(t, t - (uint32_t)P);
                }
                fail = par;
                if (update) {
                    // backward magnitudes B[k] = B[k+1] [+] m[k] (:84-89)
                    uint32_t B[P];
                    B[P - 1] = iabs(st[P - 1]);
#pragma unroll
                    for (int k = P - 2; k >= 1; --k) B[k] = bp_mag(B[k + 1], iabs(st[k]), C, w);
                    // Recompute |m| and neg(m) below instead of keeping 2 x 47 values live across
                    // the passes (the opaque moves stop the compiler from CSE-ing them).
#pragma unroll
                    for (int k = 0; k < P; ++k) asm volatile("" : "+v"(st[k]));
                    // forward pass fused with the extrinsic outputs (:83-116)
                    uint32_t F = iabs(st[0]);
                    st[0] = (S ^ (st[0] <= 0)) ? -(int)B[1] : (int)B[1];
#pragma unroll
                    for (int k = 1; k <= P - 2; ++k) {
                        const bool nk = st[k] <= 0;
                        const uint32_t ak = iabs(st[k]);
                        const uint32_t o = bp_mag(F, B[k + 1], C, w);
                        st[k] = (S ^ nk) ? -(int)o : (int)o;
                        F = bp_mag(F, ak, C, w);
                    }
                    st[P - 1] = (S ^ (st[P - 1] <= 0)) ? -(int)F : (int)F;
                    // post' = LLR + sum c2v' (:131-144), order-free integer adds in LDS
                    t = col;
                    asm volatile("" : "+v"(t));
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        lds_add(pn + k * P + t, st[k]);
                        t += row;
                        t = min(t, t - (uint32_t)P);
                    }
                } else {
                    // restore the c2v state (unused after the final syndrome, kept for clarity)
                }
            }
            fail = step_or(fail, misc, it);
            const int done = it - 1;
            if (done == 0 && a.precheck && !fail) {
                pf = llr_s;
                pre = true;
                iters = 0;
                ok = 1;
                break;
            }
            if ((done >= 1 && a.early_term && !fail) || done >= a.max_iter) {
                pf = pc;
                iters = done;
                ok = !fail;
                break;
            }
            cur = (cur + 1) % 3;
        }
        frame_store(a, cw, pf, !pre, iters, ok, misc);
    }
    chain_exit(a);
}

}  // namespace
}  // namespace fpldpc
