// fpldpc_minsum_device.hpp -- the min-sum check rule with compressed check state, defined once for the two
// kernels that run it (fpldpc_layered_minsum.hip: layered schedule; fpldpc_minsum.hip: flooding schedule) and
// their forms with the state in global memory (fpldpc_minsum_global.hip).  Included by those three
// translation units only.
//
// Normalised / offset min-sum: with f(x) = max(((x * scale_16) >> 4) - offset, 0), for a check c with
// slots k on variables v_k,
//     t[k] = clamp(post[v_k] - c2v[c][k], S_m);  s[k] = t[k] <= 0
//     m1 = min |t|, k1 the first slot attaining it, m2 = min over the other slots
//     new[k] = (parity of s over j != k) ? -f(k == k1 ? m2 : m1) : f(k == k1 ? m2 : m1)
//     c2v[c][k] = new[k]
// A check's messages take only two magnitudes, so its state is 16 bytes whatever the degree,
//     { int16 f(m1), int16 f(m2), int32 k1, uint64 sign word (bit k = s[k]) }
// Message k is rebuilt as magnitude k == k1 ? f(m2) : f(m1) with sign parity(sign word) ^ s[k]; an all-zero
// entry rebuilds every message to 0, the frame's initial state.
//
// Everything here is loop-free and per slot: the unrolled slot loops stay in the kernels (unrolling a loop
// inside an inlined helper moved the register allocation of the wide instantiations a long way).
// Signs are arithmetic (0 / -1 words, bit-field extracts), not lane masks: the unrolled slots would
// otherwise hold one scalar register pair each.
#pragma once
#include "fpldpc_layered_device.hpp"

namespace fpldpc {
namespace {

struct MinsumArgs {
    LayeredArgs a;  // as the other layered kernels read it (C, mask and c2v_scratch unused; flooding: L, layers too)
    int scale_16 = 16, offset = 0;
};

constexpr size_t kMsStateBytes = 16;  // per check

__device__ __forceinline__ int ms_correct(int x, int scale_16, int offset) { return max(((x * scale_16) >> 4) - offset, 0); }

// (x ^ neg) - neg: x for neg = 0, -x for neg = -1
__device__ __forceinline__ int ms_signed(int x, int neg) { return (x ^ neg) - neg; }
// -(bit k of the 64-bit word hi:lo) for a constant k: one signed bit-field extract
__device__ __forceinline__ int ms_neg_bit(uint32_t lo, uint32_t hi, int k) {
    return (int)((k < 32 ? lo : hi) << (31 - (k & 31))) >> 31;
}

// A check's messages, decoded: the two magnitudes, k1, and the sign word flipped by the check's parity
// (bit k of hi:lo: message k is negative).
struct MsMessages {
    int M1, M2, k1;
    uint32_t lo, hi;
    // from corrected magnitudes and the sign word (bit k = s[k])
    __device__ __forceinline__ MsMessages(int M1_, int M2_, int k1_, uint32_t slo, uint32_t shi) : M1(M1_), M2(M2_), k1(k1_) {
        const uint32_t flip = 0u - (uint32_t)((__popc(slo) + __popc(shi)) & 1);
        lo = slo ^ flip;
        hi = shi ^ flip;
    }
    // from a stored entry: x = f(m1) | f(m2) << 16, y = k1, (z, w) = sign word
    __device__ __forceinline__ explicit MsMessages(uint4 st)
        : MsMessages((int)(st.x & 0xffff), (int)(st.x >> 16), (int)st.y, st.z, st.w) {}
    // message k, for a constant k
    __device__ __forceinline__ int operator()(int k) const { return ms_signed(k == k1 ? M2 : M1, ms_neg_bit(lo, hi, k)); }
};

// The variables of check c, slot by slot in rising k.  COMPUTED: forward array code, v = k*p + (j + i*k) mod p
// for c = i*p + j; else the slot-major index table vidx [dc_max][m] (global memory or LDS).
template <bool COMPUTED>
struct MsSlots {
    const uint16_t *vidx;
    int m, p, c, ci = 0, col = 0;
    __device__ __forceinline__ MsSlots(const uint16_t *vidx_, int m_, int p_, int c_) : vidx(vidx_), m(m_), p(p_), c(c_) {
        if constexpr (COMPUTED) {
            ci = c / p;
            col = c - ci * p;
        }
    }
    __device__ __forceinline__ uint32_t next(int k) {
        if constexpr (COMPUTED) {
            const uint32_t v = (uint32_t)(k * p + col);
            col += ci;
            col = (int)min((uint32_t)col, (uint32_t)(col - p));  // mod p (col < 2p)
            return v;
        } else {
            return vidx[(size_t)k * m + c];
        }
    }
};

// Pass 1 of a check: the minima, k1 and the sign word over its t[k].  The member order and the shape of
// add() are the ones with which the predicated layered kernels compile to the code of the hand-inlined
// form and the others to a reordering of it (profiles/r12/minsum_refactor/).
struct MsTrack {
    uint32_t lo = 0, hi = 0;
    int m1 = 0x7fff, m2 = 0x7fff, k1 = 0;
    // slot k (a constant) with t[k] = t, |t| <= S_m < 2^15
    __device__ __forceinline__ void add(int k, int t) {
        const int mag = max(t, -t);
        const uint32_t s = (uint32_t)(t - 1) >> 31;  // t <= 0
        // (selects on the constant k, not a branch)
        lo |= (k < 32 ? s : 0u) << (k & 31);
        hi |= (k < 32 ? 0u : s) << (k & 31);
        m2 = min(m2, max(mag, m1));
        k1 = mag < m1 ? k : k1;
        m1 = min(m1, mag);
    }
    // applies f, stores the check's entry and returns its new messages
    __device__ __forceinline__ MsMessages finish(uint4 *entry, const MinsumArgs &ma) const {
        const int M1 = ms_correct(m1, ma.scale_16, ma.offset), M2 = ms_correct(m2, ma.scale_16, ma.offset);
        *entry = make_uint4((uint32_t)M1 | (uint32_t)M2 << 16, (uint32_t)k1, lo, hi);
        return MsMessages(M1, M2, k1, lo, hi);
    }
};

}  // namespace
}  // namespace fpldpc
