// fpldpc_flood_checks_table.hpp -- the check policy of the packed kernel (flood_pk) for any code with
// small check degrees, its slots read from the var-index table: TableChecks (W: degrees 7 and 8).
// Included by fpldpc_kernels_w1.hip (the degree-sorted W kernel) and fpldpc_kernels.hip (the unsorted
// one).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"

namespace fpldpc {
namespace {

// Check side of the packed kernel, any code with check degree <= DC (irregular allowed, e.g. the
// 802.11n code: degrees 7 and 8): CPL checks per lane (check c = tid + q*256), per-slot gather
// byte offsets packed two per VGPR (from the [DC][m_pad] var-index table), c2v state (carry form)
// in VGPRs.  The fold follows the reference's serial schedule; slots k >= deg are masked (DMIN:
// the smallest check degree the variant accepts, so slots below it need no masks).
// QLO > 0: the decoder's table lists the checks by ascending degree and the first QLO passes
// (checks [0, QLO*256)) all have degree DMIN exactly (choose_kernel checks it), so those passes fold
// DMIN slots with no masks and no gather, box-plus or emission for slot DMIN..DC-1 -- W: 768 of its
// 972 checks are degree 7, and a degree-7 check in an 8-slot pass pays for the 8th slot.  Check
// order is free: each check's fold is its own, and the posterior sums are integer adds (atomics
// from many waves already arrive in any order).
template <int DC, int CPL, int DMIN, int QLO = 0, int TNT = kNT>
struct TableChecks {
    static_assert(QLO >= 0 && QLO <= CPL && DMIN <= DC, "bad pass split");
    // The tail's split form (round 6): one frame in half 0 of the LDS words, and a lane's four checks
    // fold two at a time -- q0 in the low half with q2 in the high half, then q1 with q3 -- so a lone
    // frame's step is two passes instead of four.  Needs the degree-sorted layout with QLO = 3 (q0..q2
    // all of degree DMIN; q3 DMIN..DC or absent).  W @ 2 dB +4.5 %, W at 30 iterations +0.3 %, with W's
    // translation unit compiled without the post-RA scheduler (profiles/r6/ab/w_split_options.txt;
    // round 5's version in the shared unit: +3 % / -2 to -5 %, the packed loop's registers reallocated).
    static constexpr bool kSplit = CPL == 4 && QLO == 3 && DC == DMIN + 1;
    static __device__ __forceinline__ uint32_t rot16(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 16); }
    static constexpr int kRefillBatch = 4;
    static constexpr bool kStationary = false;  // (flood_pk's stationary exit: the A policy's only)
    static constexpr int kTabWords = 0;
    static constexpr int kN = 0;  // code length at run time
    // posteriors as biased pairs with the array policy's borrow-chain sign/magnitude (W +1.0 % over
    // carry form, profiles/r2/ab/tab_biased.txt; round 1's biased variant without the borrow chain
    // measured the same, profiles/r1/ab/w_biased.jsonl)
    static constexpr int DP = (DC + 1) / 2;
    uint32_t st[CPL][DC];
    uint32_t off[CPL][DP];  // byte offsets 4*var of slots 2j (low 16 bits) and 2j+1 (high)
    int deg[CPL];
    // slots folded by pass Q, and its degree (a compile-time DMIN in the QLO passes)
    template <int Q>
    static constexpr int slots() { return Q < QLO ? DMIN : DC; }
    template <int Q>
    __device__ __forceinline__ int degree() const { return Q < QLO ? DMIN : deg[Q]; }
    __device__ __forceinline__ void init(const KArgs &a, int tid, uint32_t * = nullptr) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = tid + q * TNT;
            const bool act = c < a.m;
            deg[q] = act ? (int)a.cdeg[c] : 0;
#pragma unroll
            for (int j = 0; j < DP; ++j) {
                uint32_t lo = 0, hi = 0;
                if (act) {
                    lo = 4u * a.vidx[(size_t)(2 * j) * a.m_pad + c];
                    if (2 * j + 1 < DC) hi = 4u * a.vidx[(size_t)(2 * j + 1) * a.m_pad + c];
                }
                off[q][j] = lo | (hi << 16);
            }
#pragma unroll
            for (int k = 0; k < DC; ++k) st[q][k] = 0;
        }
    }
    __device__ __forceinline__ uint32_t o16(int q, int k) const {
        return (k & 1) ? off[q][k >> 1] >> 16 : off[q][k >> 1] & 0xffffu;
    }
    template <int Q>
    __device__ __forceinline__ void step_q(const char *pcb, char *pnb, u16x2 C2, uint32_t M2, uint32_t &fail,
                                           uint32_t &ovor) {
        constexpr uint32_t MAG = 0x7fff7fffu;
        constexpr int D = slots<Q>();
        const int d = degree<Q>();
        if (Q >= QLO && d == 0) return;
        uint32_t sm[D];
        uint32_t S = 0, px = 0;
        // bits 15 / 31 of a biased pair: NOT hard (:305-308)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const uint32_t V = *reinterpret_cast<const uint32_t *>(pcb + o16(Q, k));
            px ^= (k < DMIN || k < d) ? V : 0u;
            sm[k] = V - st[Q][k];  // biased v2c = post - c2v (:143-152)
        }
        if constexpr (D == 8) {
            sign_mag_b_x(sm);
        } else if constexpr (D == 7 || D == 6 || D == 4) {
            sign_mag_b_xg<D>(sm);
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) sm[k] = sign_mag_b(sm[k]);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) S ^= (k < DMIN || k < d) ? sm[k] : 0u;
        fail |= (px ^ ((d & 1) ? 0x80008000u : 0u)) & 0x80008000u;
        // serial forward/backward fold (:83-116) over the first d slots
        uint32_t B[D];
        B[D - 1] = sm[D - 1] & MAG;
#pragma unroll
        for (int k = D - 2; k >= 1; --k) {
            const uint32_t b = bp_mag2<kBpMany>(B[k + 1], sm[k] & MAG, C2, M2);
            B[k] = (k < DMIN - 1 || k < d - 1) ? b : sm[k] & MAG;
        }
        uint32_t F = sm[0] & MAG;
        uint32_t o0 = B[1];
        ovor |= o0;
        emit_c2v(sm[0], o0, S, ovor);
#pragma unroll
        for (int k = 1; k <= D - 2; ++k) {
            const uint32_t ak = sm[k] & MAG;
            const uint32_t ob = bp_mag2<kBpMany>(F, B[k + 1], C2, M2);
            const uint32_t o = (k < DMIN - 1 || k < d - 1) ? ob : F;
            if (k < DMIN || k < d) ovor |= o;
            uint32_t t = sm[k];
            emit_c2v(t, o, S, dummy_);
            sm[k] = t;
            F = bp_mag2<kBpMany>(F, ak, C2, M2);
        }
        if (d == D) ovor |= F;
        emit_c2v(sm[D - 1], F, S, dummy_);
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (k < DMIN || k < d) {
                st[Q][k] = sm[k];
                lds_add(reinterpret_cast<int *>(pnb + o16(Q, k)), (int)sm[k]);
            }
        }
    }
    template <int... Qs>
    __device__ __forceinline__ void step_all(std::integer_sequence<int, Qs...>, const char *pcb, char *pnb, u16x2 C2,
                                             uint32_t M2, uint32_t &fail, uint32_t &ovor) {
        (step_q<Qs>(pcb, pnb, C2, M2, fail, ovor), ...);
    }
    __device__ __forceinline__ void step(const KArgs &a, const uint32_t *pc, uint32_t *pn, uint32_t, uint32_t, u16x2 C2,
                                         uint32_t M2, uint32_t &par, uint32_t &ovor) {
        uint32_t fail = 0;  // OR over this lane's checks of each check's parity (not their XOR)
        step_all(std::make_integer_sequence<int, CPL>{}, reinterpret_cast<const char *>(pc), reinterpret_cast<char *>(pn),
                 C2, M2, fail, ovor);
        par = fail;
    }
    template <int Q>
    __device__ __forceinline__ void syndrome_q(const char *pcb, uint32_t &fail) const {
        constexpr int D = slots<Q>();
        const int d = degree<Q>();
        if (Q >= QLO && d == 0) return;
        uint32_t px = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {  // unrolled: off[] stays in registers
            const uint32_t V = *reinterpret_cast<const uint32_t *>(pcb + o16(Q, k));
            px ^= (k < DMIN || k < d) ? V : 0u;
        }
        fail |= (px ^ ((d & 1) ? 0x80008000u : 0u)) & 0x80008000u;
    }
    template <int... Qs>
    __device__ __forceinline__ void syndrome_all(std::integer_sequence<int, Qs...>, const char *pcb, uint32_t &fail) const {
        (syndrome_q<Qs>(pcb, fail), ...);
    }
    __device__ __forceinline__ uint32_t syndrome(const uint32_t *pc, uint32_t) const {
        uint32_t fail = 0;
        syndrome_all(std::make_integer_sequence<int, CPL>{}, reinterpret_cast<const char *>(pc), fail);
        return fail;
    }
    __device__ __forceinline__ void clear(int finished) {
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                if (q < QLO && k >= DMIN) continue;  // slots the QLO passes never use
                if (finished & 1) st[q][k] -= (uint32_t)carry_lo(st[q][k]);
                if (finished & 2) st[q][k] = (uint32_t)carry_lo(st[q][k]);
            }
    }

    // ---- split form (kSplit) ----
    // state of the frame in half h -> pairs st[p][k] = (c2v of check p, of check p + 2) in carry form
    __device__ __forceinline__ void split_enter(int h) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int k = 0; k < DC; ++k) {
                const uint32_t a = st[p][k], b = st[p + 2][k];
                const int ca = h ? (int)(a - (uint32_t)carry_lo(a)) >> 16 : carry_lo(a);
                const int cb = h ? (int)(b - (uint32_t)carry_lo(b)) >> 16 : carry_lo(b);
                st[p][k] = (uint32_t)ca + ((uint32_t)cb << 16);
                st[p + 2][k] = 0;
            }
    }
    // One split pass: check PS in the low half, check PS + 2 in the high half, both of the frame in
    // half 0 of the posterior words.  The low check has degree DMIN (a QLO pass); the high one DMIN
    // (PS = 0) or its own degree dh in {0, DMIN, DC} (PS = 1): the DC-th slot, and every slot of an
    // absent check, is masked per half.  The same chains in the same order as step_q.
    template <int PS>
    __device__ __forceinline__ void split_pass(const char *pcb, char *pnb, u16x2 C2, uint32_t M2, uint32_t &fail,
                                               uint32_t &ovor) {
        constexpr uint32_t MAG = 0x7fff7fffu;
        constexpr int D = PS == 0 ? DMIN : DC;
        const int dh = PS == 0 ? DMIN : deg[3];
        // per-half validity of slot k: low k < DMIN, high k < dh
        auto vm = [&](int k) -> uint32_t { return (k < DMIN ? 0x0000ffffu : 0u) | (k < dh ? 0xffff0000u : 0u); };
        uint32_t sm[D];
        uint32_t S = 0, px = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const uint32_t Vl = *reinterpret_cast<const uint32_t *>(pcb + o16(PS, k));
            const uint32_t Vh = *reinterpret_cast<const uint32_t *>(pcb + o16(PS + 2, k));
            const uint32_t V = __builtin_amdgcn_perm(Vh, Vl, 0x05040100u);  // (half 0 of Vl, half 0 of Vh)
            px ^= PS == 0 ? V : V & vm(k);
            sm[k] = V - st[PS][k];
        }
        if constexpr (D == 8) sign_mag_b_x(sm); else sign_mag_b_xg<D>(sm);
#pragma unroll
        for (int k = 0; k < D; ++k) S ^= PS == 0 ? sm[k] : sm[k] & vm(k);
        fail |= (px ^ ((DMIN & 1) ? 0x8000u : 0u) ^ ((dh & 1) ? 0x80000000u : 0u)) & 0x80008000u;
        uint32_t o[D];
        if constexpr (PS == 0) {  // both halves DMIN slots: the plain fold
            uint32_t B[D];
            B[D - 1] = sm[D - 1] & MAG;
#pragma unroll
            for (int k = D - 2; k >= 1; --k) B[k] = bp_mag2<kBpMany>(B[k + 1], sm[k] & MAG, C2, M2);
            uint32_t F = sm[0] & MAG;
            o[0] = B[1];
#pragma unroll
            for (int k = 1; k <= D - 2; ++k) {
                o[k] = bp_mag2<kBpMany>(F, B[k + 1], C2, M2);
                F = bp_mag2<kBpMany>(F, sm[k] & MAG, C2, M2);
            }
            o[D - 1] = F;
        } else {  // low DMIN = DC - 1 slots; high DC slots when dh == DC
            const uint32_t h8 = dh == DC ? 0xffff0000u : 0u;
            uint32_t B[D];
            B[D - 1] = sm[D - 1] & MAG;
            {
                const uint32_t b = bp_mag2<kBpMany>(B[D - 1], sm[D - 2] & MAG, C2, M2);
                B[D - 2] = (b & h8) | (sm[D - 2] & MAG & ~h8);
            }
#pragma unroll
            for (int k = D - 3; k >= 1; --k) B[k] = bp_mag2<kBpMany>(B[k + 1], sm[k] & MAG, C2, M2);
            uint32_t F = sm[0] & MAG;
            o[0] = B[1];
#pragma unroll
            for (int k = 1; k <= D - 3; ++k) {
                o[k] = bp_mag2<kBpMany>(F, B[k + 1], C2, M2);
                F = bp_mag2<kBpMany>(F, sm[k] & MAG, C2, M2);
            }
            {  // slot D - 2: the last slot of a DMIN check (F), an inner one of a DC check
                const uint32_t b = bp_mag2<kBpMany>(F, B[D - 1], C2, M2);
                o[D - 2] = (b & h8) | (F & ~h8);
                F = bp_mag2<kBpMany>(F, sm[D - 2] & MAG, C2, M2);
            }
            o[D - 1] = F;  // (high half only)
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const uint32_t ok = PS == 0 ? o[k] : o[k] & vm(k);  // (an absent high check: dh = 0)
            ovor |= ok;
            uint32_t t = sm[k];
            emit_c2v(t, ok, S, dummy_);
            st[PS][k] = t;
            const int lo = carry_lo(t);
            if (k < DMIN) lds_add(reinterpret_cast<int *>(pnb + o16(PS, k)), lo);
            if (PS == 0 || k < dh) lds_add(reinterpret_cast<int *>(pnb + o16(PS + 2, k)), (int)(t - (uint32_t)lo) >> 16);
        }
    }
    __device__ __forceinline__ void split_step(const uint32_t *pc, uint32_t *pn, uint32_t, uint32_t, u16x2 C2,
                                               uint32_t M2, uint32_t &par, uint32_t &ovor) {
        uint32_t fail = 0;
        split_pass<0>(reinterpret_cast<const char *>(pc), reinterpret_cast<char *>(pn), C2, M2, fail, ovor);
        split_pass<1>(reinterpret_cast<const char *>(pc), reinterpret_cast<char *>(pn), C2, M2, fail, ovor);
        par = (fail | fail >> 16) & 0x8000u;  // the one frame fails if either half's check does
    }
    uint32_t dummy_ = 0;
};

}  // namespace
}  // namespace fpldpc
