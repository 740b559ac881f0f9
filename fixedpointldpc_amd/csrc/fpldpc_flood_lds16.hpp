// fpldpc_flood_lds16.hpp -- flood_lds16, the one-frame kernel with its c2v state as int16 in LDS: the
// middle link of R's fallback chain (packed -> flood_lds16 -> flood_gmem).  Included by
// fpldpc_kernels.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"

namespace fpldpc {
namespace {

// LDS-state kernel for array codes whose c2v state does not fit registers (p47/r24: 1128 checks x
// 47 edges).  One frame per 1024-thread workgroup; each lane owns check tid and, for m > 1024,
// check tid + 1024.  The c2v state lives in LDS as int16 ([check][slot]); the
// posteriors stay int32.  Magnitude chains use 16-bit min (full rate on gfx950) and 32-bit
// add/sub/shift/and.  Exact while every |v2c| < 2^14 (then every chain value, a + b and c2v fit
// 16 bits); a frame that leaves that range stops and is re-decoded by the int32 kernel.
constexpr int kNT16 = 1024;  // 16 waves: 4 per SIMD (checks tid, tid + 1024)

__device__ __forceinline__ uint32_t bp_mag16(uint32_t a, uint32_t b, unsigned short C, uint32_t M) {
    const uint32_t mn = __builtin_elementwise_min((unsigned short)a, (unsigned short)b);
    const uint32_t s = a + b;
    const uint32_t d = sub2x(s, mn);  // max - min
    const uint32_t q1 = __builtin_elementwise_min((unsigned short)((s >> 2) & M), C);
    const uint32_t q2 = __builtin_elementwise_min((unsigned short)((d >> 2) & M), C);
    return mn + q2 - q1;
}

// Edge k of a check in the LDS-state kernel: posterior p (int32 LDS) and stored c2v (int16 LDS)
// give v2c m = p - c2v (:143-152); returns |m| and folds the flags into S (sign parity, bit 31 of
// the XOR) and par (hard-decision parity, bit 31: post <= 0, :305-308).
__device__ __forceinline__ uint32_t edge16(const char *pcb, unsigned short t4, int koff, int c2v, uint32_t &S,
                                           uint32_t &par, uint32_t &ovor) {
    const int p = *reinterpret_cast<const int *>(pcb + koff + t4);
    par ^= (uint32_t)(p - 1);
    const int mm = p - c2v;
    const uint32_t sg = (uint32_t)(mm >> 31);
    const uint32_t av = ((uint32_t)mm ^ sg) - sg;
    ovor |= av;
    S ^= sg;
    return av;
}

// c2v = sign * o (sign in bit 31 of sb) into the next posterior and the check's state
__device__ __forceinline__ void put16(char *pn_addr, int16_t *st, uint32_t o, uint32_t sb) {
    const uint32_t nm = 0u - (sb >> 31);
    const int v = (int)((o ^ nm) - nm);
    lds_add(reinterpret_cast<int *>(pn_addr), v);
    *st = (int16_t)v;
}

__device__ __forceinline__ unsigned short wrap_up(unsigned short t, unsigned short step, unsigned short wrap) {
    t = (unsigned short)(t + step);
    return __builtin_elementwise_min(t, (unsigned short)(t - wrap));
}
__device__ __forceinline__ unsigned short wrap_down(unsigned short t, unsigned short step, unsigned short wrap) {
    t = (unsigned short)(t - step);
    return __builtin_elementwise_min(t, (unsigned short)(t + wrap));
}

// Compiler-only fence between the steps of check_lds16's passes: keeps the scheduler from hoisting
// every edge load of a pass to its top (2 x 47 live VGPRs -> spills / fewer resident waves).
__device__ __forceinline__ void lds16_step_fence() { asm volatile("" ::: "memory"); }

// One check of the LDS-state kernel; returns the syndrome parity of pc over the check.  Nothing per
// edge is kept in registers across the two passes: pass 1 reads every edge once (building the
// middle-out chains F_0..F_{L-1}, B_{L+1}..B_{P-1} and the parities), pass 2 re-reads each edge
// (LDS is cheap next to VGPRs here) to extend the chains and emit c2v_k = F_{k-1} [+] B_{k+1}.
template <int P>
__device__ __forceinline__ int check_lds16(int c, const int *pc, int *pn, int16_t *st16, bool update,
                                           unsigned short C, uint32_t M, uint32_t &ovor) {
    constexpr int L = (P - 1) / 2;
    const unsigned short row = (unsigned short)(c / P), col = (unsigned short)(c % P);
    const unsigned short step4 = (unsigned short)(4 * row), wrap4 = (unsigned short)(4 * P);
    const char *pcb = reinterpret_cast<const char *>(pc);
    int16_t *const stc = st16 + c * P;  // this check's c2v state ([check][slot]: constant offsets)
    uint32_t par = 0, S = 0, dummy = 0;
    // byte offsets (within a block column) of slot 0 and slot P-1: (col + row*k) mod P
    unsigned short tl = (unsigned short)(4 * col);
    unsigned short tr = (unsigned short)(4 * ((col + (uint32_t)row * (P - 1)) % P));
    asm volatile("" : "+v"(tl), "+v"(tr));
    uint32_t FB[P];
    FB[0] = edge16(pcb, tl, 0, stc[0], S, par, ovor);
    FB[P - 1] = edge16(pcb, tr, (P - 1) * P * 4, stc[P - 1], S, par, ovor);
#pragma unroll
    for (int j = 1; j < P - 1 - L; ++j) {
        lds16_step_fence();
        if (j < L) {
            tl = wrap_up(tl, step4, wrap4);
            FB[j] = bp_mag16(FB[j - 1], edge16(pcb, tl, j * P * 4, stc[j], S, par, ovor), C, M);
        }
        tr = wrap_down(tr, step4, wrap4);
        FB[P - 1 - j] = bp_mag16(FB[P - j], edge16(pcb, tr, (P - 1 - j) * P * 4, stc[P - 1 - j], S, par, ovor), C, M);
        // fold the flags now: left to itself the compiler sinks the par / ovor / S chains past pass 2
        // and keeps all 2 x 47 posteriors and magnitudes live (93 VGPRs of spills at 1024 threads)
        asm volatile("" : "+v"(par), "+v"(ovor), "+v"(S));
    }
    tl = wrap_up(tl, step4, wrap4);  // slot L
    const unsigned short tL = tl;
    const uint32_t aL = edge16(pcb, tL, L * P * 4, stc[L], S, par, ovor);
    if (!update) return (int)(par >> 31);
    // memory clobber: pass 2 re-reads the LDS state instead of the compiler keeping the 47 values
    // of pass 1 live in registers
    asm volatile("" ::: "memory");
    // pass 2: outputs from the middle outwards; the sign of c2v_k is S ^ sign(m_k)
    char *pnb = reinterpret_cast<char *>(pn);
    uint32_t F, B;
    {
        uint32_t S2 = 0;
        const int p = *reinterpret_cast<const int *>(pcb + L * P * 4 + tL);
        S2 = (uint32_t)((p - (int)stc[L]) >> 31);
        const uint32_t o = bp_mag16(FB[L - 1], FB[L + 1], C, M);
        F = bp_mag16(FB[L - 1], aL, C, M);
        B = bp_mag16(FB[L + 1], aL, C, M);
        put16(pnb + L * P * 4 + tL, stc + L, o, S ^ S2);
    }
    unsigned short uf = tL, ub = tL;
#pragma unroll
    for (int j = 1; j <= (L > P - 1 - L ? L : P - 1 - L); ++j) {
        const int kf = L + j, kb = L - j;
        lds16_step_fence();
        if (kf <= P - 1) {
            uf = wrap_up(uf, step4, wrap4);
            uint32_t sgk = 0;
            const uint32_t ak = edge16(pcb, uf, kf * P * 4, stc[kf], sgk, dummy, dummy);
            uint32_t o = F;  // c2v_{P-1} = F_{P-2}
            if (kf <= P - 2) {
                o = bp_mag16(F, FB[kf + 1], C, M);
                F = bp_mag16(F, ak, C, M);
            }
            put16(pnb + kf * P * 4 + uf, stc + kf, o, S ^ sgk);
        }
        if (kb >= 0) {
            ub = wrap_down(ub, step4, wrap4);
            uint32_t sgk = 0;
            const uint32_t ak = edge16(pcb, ub, kb * P * 4, stc[kb], sgk, dummy, dummy);
            uint32_t o = B;  // c2v_0 = B_1
            if (kb >= 1) {
                o = bp_mag16(FB[kb - 1], B, C, M);
                B = bp_mag16(B, ak, C, M);
            }
            put16(pnb + kb * P * 4 + ub, stc + kb, o, S ^ sgk);
        }
    }
    return (int)(par >> 31);
}

template <int P, int NT = kNT16>
__global__ void __launch_bounds__(NT, NT / 256) flood_lds16(KArgs a) {
    if (empty_list(a)) return;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    constexpr int n = P * P;
    int *const bufs = smem;
    int *const llr_s = smem + 3 * n;
    int *const misc = smem + 4 * n;  // [0] frame [1] bit errors [2..4] flag words
    int16_t *const st16 = reinterpret_cast<int16_t *>(smem + 4 * n + 16);
    const int tid = threadIdx.x, m = a.m;
    const unsigned short C = (unsigned short)a.C;
    const uint32_t M = (1u << a.bfe_w) - 1u;

    for (;;) {
        __syncthreads();
        if (tid == 0) {
            misc[0] = pull_frame(a, a.work_counter);
            misc[1] = 0;
            misc[2] = misc[3] = misc[4] = 0;
        }
        __syncthreads();
        const int cw = misc[0];
        if (cw < 0) break;
        frame_load<NT>(a, cw, bufs, llr_s);
        for (int e = tid; e < m * P; e += NT) st16[e] = 0;
        __syncthreads();
        int cur = 0;
        const int *pf = nullptr;
        bool pre = false, taint = false;
        int iters = 0, ok = 0;
        for (int it = 1;; ++it) {
            const bool update = it <= a.max_iter;
            const int *pc = bufs + cur * n;
            int *pn = bufs + ((cur + 1) % 3) * n;
            int *pr = bufs + ((cur + 2) % 3) * n;
            if (update)
                for (int v = tid; v < n; v += NT) pr[v] = llr_s[v];
            if (tid == 0) misc[2 + (it + 1) % 3] = 0;  // flag word of step it+1 (see flood_pk)
            int fail = 0;
            uint32_t ovor = 0;
            for (int c = tid; c < m; c += NT) fail |= check_lds16<P>(c, pc, pn, st16, update, C, M, ovor);
            {
                const uint32_t bits = (uint32_t)fail | (ovor >= (1u << 14) ? 2u : 0u);
                uint32_t wb = (__ballot(bits & 1u) ? 1u : 0u) | (__ballot(bits & 2u) ? 2u : 0u);
                if ((tid & 63) == 0 && wb) atomicOr(&misc[2 + it % 3], (int)wb);
            }
            __syncthreads();
            const int flags = misc[2 + it % 3];
            if (flags & 2) {  // left the exact 16-bit range: hand the frame to the int32 kernel
                taint = true;
                break;
            }
            fail = flags & 1;
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
        if (taint) {
            if (tid == 0) a.fb_list[atomicAdd(a.fb_count, 1)] = cw;
            continue;
        }
        frame_store<NT>(a, cw, pf, !pre, iters, ok, misc);
    }
    chain_exit(a);
}

}  // namespace
}  // namespace fpldpc
