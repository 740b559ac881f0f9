// fpldpc_flood_device.hpp -- the frame framework every flooding kernel is built on: the kernel argument
// block (KArgs), the counter block's reset on the way out of a call's last kernel, the frame pull, the
// reference's box-plus and its serial check update, the frame prologue and epilogue.  Included by the
// other fpldpc_flood_*.hpp headers, and through them by fpldpc_kernels.hip, fpldpc_kernels_a1.hip and
// fpldpc_kernels_w1.hip.
//
// Reference semantics (tyc85/FixedPointLDPC): FP_Decoder::decode_general_fp
// (ArrayLDPC_Decoder.cpp:18-171) with the box-plus FP_Decoder::sxor (:677-694), the syndrome
// test checkPost_fp_general (:296-333), and decode_fixpoint's channel pre-check (:443-450).
//
// Design (DESIGN.md "Kernels"):
//   * One workgroup decodes one frame at a time and pulls the next frame from a device work
//     counter (persistent grid, per-frame early termination, no frozen lanes).
//   * One lane per check node.  The check's c2v messages live in VGPRs across iterations (or in a
//     per-workgroup global scratch for codes too large for registers); the posterior vector lives
//     in LDS.  The reference's variable-node phase (:121-156) is folded into the check pass:
//     v2c = post - c2v (:143-152), and the next posterior post' = LLR + sum(c2v') is accumulated
//     with LDS integer atomics (order-free, exact).  Three rotating posterior buffers give one
//     barrier per iteration.
//   * The check update keeps the reference's SERIAL forward/backward fold (:83-116): box-plus is
//     not associative, so no tree/shuffle reduction is used for it.
//   * The syndrome of iteration t is computed while gathering the posteriors of iteration t+1
//     (hard = post > 0 ? 0 : 1, :305-308); the pre-check is the same test on the channel LLRs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpldpc_internal.hpp"

namespace fpldpc {
namespace {

constexpr int kNT = 256;  // threads per workgroup (4 waves)
// per-workgroup control words after the posterior buffers in LDS (flood_pk's misc[])
constexpr int kTotW = 16;  // flood_pk: the workgroup's 4 totals counters misc[kTotW..+3]
constexpr int kMiscInts = kTotW + 4;

struct KArgs {
    const void *llr;
    int llr_i16;
    int n, m, m_pad, batch, max_iter, C, mask, early_term, precheck;
    const uint16_t *vidx;
    const uint8_t *cdeg;
    uint32_t *hard;
    int hard_words;
    int32_t *iters;
    uint8_t *syn_ok;
    int32_t *post;
    int32_t *bit_errors;
    unsigned long long *totals;
    const int32_t *info_idx;
    const uint8_t *info_bits;
    int k_info;
    const uint32_t *info_mask;  // [2][hard_words] packed: info positions, reference bits (distinct indices) or null
    int *work_counter;
    int32_t *c2v_scratch;  // global-state kernels: [grid][dc][m_pad]; the A kernel: [grid][47][256] words for the
                           // stationary exit's verification, null = exit off (flood_pk)
    uint32_t bfe_w;  // width_mask = 2^(bfe_w + 2) - 1 (contiguous-mask kernels only)
    // frame-list mode (fallback pass): work item i decodes frame frame_list[i], i < *frame_count
    const int *frame_list;
    const int *frame_count;
    // packed kernels: frames whose int16 range check failed are appended here for the int32 pass
    int *fb_list;
    int *fb_count;
    uint32_t cmax;  // largest c2v magnitude for which int16 posteriors / v2c cannot overflow
    unsigned long long *probe;  // diagnostic (FPLDPC_CLOCK_PROBE): workgroup 0's s_memtime/s_memrealtime
    unsigned long long *wgtrace;  // diagnostic (FPLDPC_WG_TRACE): per workgroup {xcc<<32 | hw_id, start, end, frames, stamps[4]}
    int *counters;       // the decoder's counter block (fpldpc_internal.hpp kCounterInts)
    int last_in_chain;   // 1: this launch is the call's last kernel and resets the counter block
    int split_tail;      // packed array kernels: a lone frame continues in the split form (flood_pk); bit 1: the A
                         // kernel's cycle exit in that form is on
};

__device__ __forceinline__ void clock_probe(const KArgs &a, int slot) {
    if (a.probe && blockIdx.x == 0 && threadIdx.x == 0) {
        a.probe[slot] = __builtin_amdgcn_s_memtime();
        a.probe[slot + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// Every workgroup calls chain_exit as it exits (all threads, uniform).  The last workgroup out of the
// call's LAST kernel resets the decoder's counter block for the next call: every workgroup of this
// kernel has made its last counter access before counting itself out, and the chain's earlier
// kernels have completed (stream order).  So no hipMemsetAsync precedes a decode call; the block
// is zeroed once at decoder creation.  The fallback-list sizes are kept for
// fpldpc_decoder_fallback_counts.
// (No fences: every counter access a workgroup makes before counting itself out is a returning
// atomic or a load whose value it has used, so it has been performed; the next call's kernels see
// the reset at the kernel boundary.)
__device__ __forceinline__ void chain_reset(int *c) {
    c[kCountFb0Last] = __hip_atomic_load(&c[kCountFb0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c[kCountFb1Last] = __hip_atomic_load(&c[kCountFb1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = 0; i <= kCountExit; ++i) c[i] = 0;
}
__device__ __forceinline__ void chain_exit(const KArgs &a) {
    if (!a.last_in_chain || threadIdx.x != 0) return;
    if (atomicAdd(&a.counters[kCountExit], 1) == (int)gridDim.x - 1) chain_reset(a.counters);
}
// A fallback kernel whose frame list came out empty (the common case) leaves at once, uncounted:
// no workgroup of it touches a counter, and the list size it reads is already 0, so workgroup 0
// alone can reset the block (the last kernel of the chain) without waiting for the others --
// counting 256 workgroups out through one atomic cost ~7 us per call.
__device__ __forceinline__ bool empty_list(const KArgs &a) {
    if (!a.frame_list || *a.frame_count != 0) return false;
    if (a.last_in_chain && blockIdx.x == 0 && threadIdx.x == 0) chain_reset(a.counters);
    return true;
}

// Next frame for this workgroup (thread 0 only): the work counter indexes the batch, or the
// fallback list in frame-list mode.  Returns -1 when the work is exhausted.
__device__ __forceinline__ int pull_frame(const KArgs &a, int *counter) {
    const int wi = atomicAdd(counter, 1);
    if (a.frame_list) return wi < *a.frame_count ? a.frame_list[wi] : -1;
    return wi < a.batch ? wi : -1;
}

// x [+] y = sgn(x) sgn(y) (min(|x|,|y|) + max(0, C - ((|x|+|y|) & mask) >> 2)
//                                      - max(0, C - (||x|-|y|| & mask) >> 2)),  sgn(0) = -1.
// ArrayLDPC_Decoder.cpp:677-694, ArrayLDPCMacro.h:222-224.  The magnitude term r is never
// negative (tests/test_oracle.py::test_sign_split: exhaustively wherever min(|x|,|y|) < C, for
// every mask 2^w - 1, w = 2..16, FRAC 3/4/6), so the sign of the result is + iff
// (x > 0) == (y > 0), and r == 0 gives 0 either way.
__device__ __forceinline__ int boxplus(int x, int y, int C, int mask) {
    const int a = x < 0 ? -x : x;
    const int b = y < 0 ? -y : y;
    const int s = ((a + b) & mask) >> 2;
    const int d = ((a > b ? a - b : b - a) & mask) >> 2;
    const int p1 = max(C - s, 0);
    const int p2 = max(C - d, 0);
    const int r = min(a, b) + p1 - p2;
    return ((x > 0) == (y > 0)) ? r : -r;
}

__device__ __forceinline__ void lds_add(int *p, int v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int DC>
__device__ __forceinline__ int slot_var(const uint32_t (&vpk)[(DC + 1) / 2], int k) {
    return (k & 1) ? (int)(vpk[k >> 1] >> 16) : (int)(vpk[k >> 1] & 0xffffu);
}

// One check: gather posteriors, syndrome parity, serial forward/backward fold, scatter-add.
// c2v: in = previous c2v (0 before the first iteration), out = new c2v.  Returns the parity of
// the hard decisions of pc over the check (1 = unsatisfied).
template <int DC, bool REGULAR>
__device__ __forceinline__ int check_update(int (&c2v)[DC], const uint32_t (&vpk)[(DC + 1) / 2], int deg,
                                            const int *pc, int *pn, bool update, int C, int mask) {
    int m[DC];
    int par = 0;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
        const int p = pc[slot_var<DC>(vpk, k)];
        if (REGULAR || k < deg) par ^= (p <= 0) ? 1 : 0;
        m[k] = p - c2v[k];  // v2c = post - c2v (ArrayLDPC_Decoder.cpp:143-152)
    }
    if (!update) return par;
    // Backward[k] = Backward[k+1] [+] m[k], Backward[deg-1] = m[deg-1]   (:84-89)
    int B[DC];
    B[DC - 1] = m[DC - 1];
#pragma unroll
    for (int k = DC - 2; k >= 1; --k) {
        const int bk = boxplus(B[k + 1], m[k], C, mask);
        B[k] = (REGULAR || k < deg - 1) ? bk : m[k];
    }
    // Forward[k] = Forward[k-1] [+] m[k]; out[0] = B[1], out[k] = F[k-1] [+] B[k+1],
    // out[deg-1] = F[deg-2]   (:83-116)
    int F = m[0];
    c2v[0] = B[1];
#pragma unroll
    for (int k = 1; k <= DC - 2; ++k) {
        const int o = boxplus(F, B[k + 1], C, mask);
        c2v[k] = (REGULAR || k < deg - 1) ? o : F;
        F = boxplus(F, m[k], C, mask);
    }
    c2v[DC - 1] = F;
    // post' = LLR + sum c2v' (:131-144), accumulated order-free in LDS.
#pragma unroll
    for (int k = 0; k < DC; ++k)
        if (REGULAR || k < deg) lds_add(pn + slot_var<DC>(vpk, k), c2v[k]);
    return par;
}

__device__ __forceinline__ int load_llr(const KArgs &a, size_t i) {
    return a.llr_i16 ? (int)static_cast<const int16_t *>(a.llr)[i] : static_cast<const int32_t *>(a.llr)[i];
}

// Frame prologue: LLR -> LDS (int32) and the first two posterior buffers.
template <int NT = kNT>
__device__ __forceinline__ void frame_load(const KArgs &a, int cw, int *bufs, int *llr_s) {
    const int n = a.n;
    const size_t base = (size_t)cw * n;
    for (int v = threadIdx.x; v < n; v += NT) {
        const int x = load_llr(a, base + v);
        llr_s[v] = x;
        bufs[v] = x;
        bufs[n + v] = x;
    }
}

// Frame epilogue: posteriors, packed hard decisions, per-frame BER and totals.
template <int NT = kNT>
__device__ __forceinline__ void frame_store(const KArgs &a, int cw, const int *pf, bool write_post, int iters,
                                            int ok, int *misc) {
    const int n = a.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.post && write_post)
        for (int v = tid; v < n; v += NT) a.post[(size_t)cw * n + v] = pf[v];
    if (a.hard) {
        uint32_t *h = a.hard + (size_t)cw * a.hard_words;
        for (int base = wave * 64; base < n; base += NT) {
            const int v = base + lane;
            const unsigned long long b = __ballot(v < n && pf[v] <= 0);
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
        for (int i = tid; i < a.k_info; i += NT) e += ((pf[a.info_idx[i]] <= 0) ? 1 : 0) != a.info_bits[i];
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
