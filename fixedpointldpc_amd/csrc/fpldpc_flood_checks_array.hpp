// fpldpc_flood_checks_array.hpp -- the check policies of the packed kernel (flood_pk) for the p = 47
// array codes: ArrayChecks (A: one check per lane; R's earlier forms: two), ArrayChecksOutGuard (A with
// the per-output range guard), SplitCore (two lanes per check) and MixChecks (R: both in one
// workgroup).  Included by fpldpc_kernels_a1.hip (the A kernel) and fpldpc_kernels.hip (the R kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"

namespace fpldpc {
namespace {

// Check side of the packed kernel, array codes: c2v state (carry form) in VGPRs; CPL checks per
// lane (c = tid + q*NT).  Slot k of check (row i, column j) reads variable k*P + (j + i*k) mod P.
// With one check per lane (A) the 16-bit byte offsets 4*((j + i*k) mod P) are computed once and
// kept two per VGPR (P/2 VGPRs), so a gather or scatter address costs one SDWA add with a word
// select (lds_at; round 2: v_add_u16 for the low half, shift + add for the high one); with several
// checks per lane (R: no VGPRs to spare) they come from an LDS table or are walked per step.
// With several checks per lane (R) the offsets do not fit VGPRs; LDS_OFFS keeps them in an LDS
// table instead (kTabW words per check, the same packing as `offs`, a word = two slots), so a
// slot costs one table read per two slots plus the same one or two address ops as with VGPR
// offsets -- against three walk ops per slot and pass.  The table's row pitch kTabW is odd, so each
// 32-lane half of a wave (consecutive checks) reads 32 different banks (ds_read_b32: dword mod 32).
template <int P, int CPL = 1, int NT = kNT, bool STORE_OFFS = true, bool LDS_OFFS = false>
struct ArrayChecks {
    static constexpr int kN = P * P;  // code length, known at compile time
    static constexpr bool kStoreOffs = CPL == 1 && STORE_OFFS;
    static constexpr bool kLdsOffs = LDS_OFFS && !kStoreOffs;
    static constexpr bool kSdwa = kStoreOffs;  // slot-address form (lds_at)
    static constexpr int kOW = kStoreOffs ? (P + 1) / 2 : 1;
    static constexpr int kBp = CPL == 1 ? kBpArray1 : kBpMany;  // bp_mag2 form
    // flood_pk's refill batch and LDS-staged stores (two checks per lane: none, R's kernel spills
    // with the batch; its frames run 50 iterations, so the per-frame work weighs 1 %)
    static constexpr int kRefillBatch = CPL == 1 ? 4 : 0;
    static constexpr int kTabW = ((P + 1) / 2) | 1;  // LDS table words per check (odd pitch)
    static constexpr int kTabWords = kLdsOffs ? kTabW : 0;  // per check, for variant_lds
    uint32_t st[CPL][P];
    uint32_t row[CPL], col[CPL];
    uint32_t offs[kOW];  // kStoreOffs: slot 2w's byte offset in bits 0-15, slot 2w+1's in bits 16-31
    uint32_t tabq[kLdsOffs ? CPL : 1];  // kLdsOffs: LDS byte address of check q's table row
    bool act[CPL];
    uint32_t pxp;  // kStationary: the XOR of the check's posterior words at the step before (the exit's trigger)
    // LDS byte address of stored-offset slot k in the buffer at base
    __device__ __forceinline__ uint32_t soff(int k, uint32_t base) const {
        return lds_at<kSdwa>(offs[kStoreOffs ? k >> 1 : 0], k & 1, base);
    }
    // table word w of check q (slots 2w, 2w+1)
    __device__ __forceinline__ uint32_t tword(int q, int w) const {
        return reinterpret_cast<const lds_u32 *>((size_t)tabq[q])[w];
    }
    __device__ __forceinline__ void init(const KArgs &a, int tid, uint32_t *tab = nullptr) {
        if (kLdsOffs) {
            // the table: every check's kTabW words, built once per workgroup (a barrier follows init)
            for (int c = tid; c < a.m; c += NT) {
                const uint32_t r = (uint32_t)(c / P);
                uint32_t x = (uint32_t)(c % P);
                for (int w = 0; w < (P + 1) / 2; ++w) {
                    uint32_t word = 4u * x;
                    x += r;
                    x = x >= (uint32_t)P ? x - P : x;
                    if (2 * w + 1 < P) {
                        word |= (4u * x) << 16;
                        x += r;
                        x = x >= (uint32_t)P ? x - P : x;
                    }
                    tab[c * kTabW + w] = word;
                }
            }
#pragma unroll
            for (int q = 0; q < (kLdsOffs ? CPL : 1); ++q) tabq[q] = lds_addr(tab + (tid + q * NT) * kTabW);
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = tid + q * NT;  // this lane's checks
            act[q] = c < a.m;
            if (kStationary) pxp = 0;
            row[q] = act[q] ? (uint32_t)(c / P) : 0u;
            col[q] = act[q] ? (uint32_t)(c % P) : 0u;
#pragma unroll
            for (int k = 0; k < P; ++k) st[q][k] = 0;
        }
        if (kStoreOffs) {
#pragma unroll
            for (int w = 0; w < kOW; ++w) offs[w] = 0;
            uint32_t x = col[0];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                offs[k >> 1] |= (4u * x) << (16 * (k & 1));
                x += row[0];
                x = x >= (uint32_t)P ? x - P : x;
            }
        }
    }
    // One flooding step for this lane's checks: gather from buffer pc, update, scatter-add into
    // buffer pn (LDS byte addresses).  par: bit 15 / 31 = OR over the lane's checks
    // of each check's syndrome parity for the low / high frame; ovor |= every c2v magnitude, or
    // (kChainGuard) a bound on them all.  kStationary: par's other bits are non-zero in a half when the
    // XOR of the check's posterior words differs, below the sign, from the step before's -- the
    // stationary exit's trigger, a hash: unchanged posteriors leave it zero.
    //
    // The chain guard.  bp_mag(a, b) <= min(a, b) + C (packed_cmax), so along the fold
    //   F_j <= F_{j-1} + C,  B_j <= B_{j+1} + C,  c2v_k = F_{k-1} [+] B_{k+1} <= min(F_{k-1}, B_{k+1}) + C,
    // and with the middle slot L = (P-1)/2: c2v_k <= F_{L-1} + (k-L+1) C for k >= L (k = P-1: c2v =
    // F_{P-2} <= F_{L-1} + (P-1-L) C) and c2v_k <= B_{L+1} + (L-k+1) C for 1 <= k <= L (k = 0: c2v =
    // B_1 <= B_{L+1} + L C).  Every output magnitude of the check is therefore at most
    //   max(F_{L-1}, B_{L+1}) + G,  G = (L+1) C,
    // and ovor |= (F_{L-1} + G) | (B_{L+1} + G) has a bit at or above 2^b (cmax = 2^b - 1) whenever
    // some c2v does: the deferred range test flags every frame the per-output OR would, and possibly a
    // few more (max(F, B) within G of the threshold), which the int32 kernel then decodes -- exactly, as
    // any flagged frame.  Both sums stay inside their 16-bit halves (chain values < 2^15, G <= 2^12).
    // choose_kernel takes this form only while G <= (cmax + 1) / 8; the per-output form is
    // ArrayChecksOutGuard's kernel.
    static constexpr bool kChainGuard = kStoreOffs;
    __device__ __forceinline__ void step(const KArgs &a, const uint32_t *pcp, uint32_t *pnp, uint32_t pc, uint32_t pn,
                                         u16x2 C2, uint32_t M2, uint32_t &par, uint32_t &ovor) {
        step_g<kChainGuard>(a, pcp, pnp, pc, pn, C2, M2, par, ovor);
    }
    template <bool CHAIN>
    __device__ __forceinline__ void step_g(const KArgs &a, const uint32_t *, uint32_t *, uint32_t pc, uint32_t pn, u16x2 C2,
                                           uint32_t M2, uint32_t &par, uint32_t &ovor) {
        uint32_t fail = 0;  // OR over the lane's checks of each check's parity (not their XOR)
        [[maybe_unused]] uint32_t trig = 0;
        // (literal operands: the same mask constants in VGPRs measured the same, profiles/r2/ab/bp_form.txt)
        constexpr uint32_t SGN = 0x80008000u, MAG = 0x7fff7fffu;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            if (!act[q]) continue;
            uint32_t(&stq)[P] = st[q];
            // Gather.  State stq[k] = c2v of the previous step in carry form; becomes the v2c
            // message in sign-magnitude halves (|m| in bits 0-14, m <= 0 in bit 15).
            unsigned short t4 = (unsigned short)(4 * col[q]);  // walked offset (!kStoreOffs)
            if (!kStoreOffs && !kLdsOffs) asm volatile("" : "+v"(t4));
            const unsigned short step4 = (unsigned short)(4 * row[q]), wrap4 = (unsigned short)(4 * P);
            uint32_t px = 0, S = 0;
            [[maybe_unused]] unsigned short tL = 0;  // walked offset of slot L
            // loads in batches of G, issued back to back, so G LDS reads are in flight per wave
            // instead of the compiler's one or two (each waited on a few instructions later)
            constexpr int G = 8;
            if constexpr (kLdsOffs) {
                // software-pipelined like the VGPR-offset gather: batches of 4 slots (2 table
                // words); batch b+1's 4 reads are issued before batch b is processed, and the table
                // words two batches ahead are read before that
                constexpr int G4 = 4, NB = (P + G4 - 1) / G4, NW = (P + 1) / 2;
                uint32_t ow[3][2], Vb[2][G4];
                auto words = [&](int b) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        if (2 * b + i < NW) ow[b % 3][i] = tword(q, 2 * b + i);
                };
                auto issue = [&](int b) {
#pragma unroll
                    for (int g = 0; g < G4; ++g) {
                        const int k = b * G4 + g;
                        if (k >= P) break;
                        const uint32_t o = lds_at<kSdwa>(ow[b % 3][g >> 1], k & 1, pc);
                        Vb[b & 1][g] = reinterpret_cast<const lds_u32 *>((size_t)o)[k * P];
                    }
                };
                words(0);
                words(1);
                issue(0);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b + 2 < NB) words(b + 2);
                    if (b + 1 < NB) issue(b + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    const int k0 = b * G4;
                    if (k0 + G4 <= P) {
                        uint32_t u[G4];
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            px ^= Vb[b & 1][g];
                            u[g] = Vb[b & 1][g] - stq[k0 + g];
                        }
                        sign_mag_b_xg<G4>(u);
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            S ^= u[g];
                            stq[k0 + g] = u[g];
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            const int k = k0 + g;
                            if (k >= P) break;
                            px ^= Vb[b & 1][g];
                            const uint32_t sm = sign_mag_b(Vb[b & 1][g] - stq[k], SGN);
                            S ^= sm;
                            stq[k] = sm;
                        }
                    }
                }
            } else if constexpr (kStoreOffs) {
                // slots per gather batch: 4, 6, 7 and 8 measured the same; without the batch's
                // scheduling barrier the kernel spills (profiles/r5/ab/post_ra.txt run 9)
                constexpr int G4 = 4, NB = (P + G4 - 1) / G4;
                uint32_t Vb[2][G4];
                auto issue = [&](int b) {
#pragma unroll
                    for (int g = 0; g < G4; ++g) {
                        const int k = b * G4 + g;
                        if (k >= P) break;
                        if (!kStoreOffs && k == (P - 1) / 2) tL = t4;
                        const uint32_t o = kStoreOffs ? soff(k, pc) : pc + t4;
                        Vb[b & 1][g] = reinterpret_cast<const lds_u32 *>((size_t)o)[k * P];
                        if (!kStoreOffs) {
                            t4 = (unsigned short)(t4 + step4);
                            t4 = __builtin_elementwise_min(t4, (unsigned short)(t4 - wrap4));
                        }
                    }
                };
                issue(0);
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (b + 1 < NB) issue(b + 1);
                    __builtin_amdgcn_sched_barrier(0);
                    const int k0 = b * G4;
                    if (k0 + G4 <= P) {
                        uint32_t u[G4];
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            px ^= Vb[b & 1][g];
                            u[g] = Vb[b & 1][g] - stq[k0 + g];
                        }
                        if constexpr (G4 == 8) sign_mag_b_x(u); else sign_mag_b_xg<G4>(u);
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            S ^= u[g];
                            stq[k0 + g] = u[g];
                        }
                    } else {
#pragma unroll
                        for (int g = 0; g < G4; ++g) {
                            const int k = k0 + g;
                            if (k >= P) break;
                            px ^= Vb[b & 1][g];
                            const uint32_t sm = sign_mag_b(Vb[b & 1][g] - stq[k], SGN);
                            S ^= sm;
                            stq[k] = sm;
                        }
                    }
                }
            } else
#pragma unroll
            for (int k0 = 0; k0 < P; k0 += G) {
                uint32_t V[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int k = k0 + g;
                    if (k >= P) break;
                    if (!kStoreOffs && k == (P - 1) / 2) tL = t4;
                    const uint32_t o = kStoreOffs ? soff(k, pc) : pc + t4;
                    V[g] = reinterpret_cast<const lds_u32 *>((size_t)o)[k * P];
                    if (!kStoreOffs) {
                        t4 = (unsigned short)(t4 + step4);
                        t4 = __builtin_elementwise_min(t4, (unsigned short)(t4 - wrap4));
                    }
                }
                if (G > 1) __builtin_amdgcn_sched_barrier(0);
                if (k0 + G <= P) {  // whole batch: the last step of sign_mag_b as a borrow chain
                    uint32_t u[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        px ^= V[g];
                        u[g] = V[g] - stq[k0 + g];
                    }
                    sign_mag_b_x(u);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        S ^= u[g];
                        stq[k0 + g] = u[g];
                    }
                    continue;
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int k = k0 + g;
                    if (k >= P) break;
                    px ^= V[g];                                      // bits 15 / 31: NOT hard (:305-308)
                    const uint32_t sm = sign_mag_b(V[g] - stq[k], SGN);  // v2c = post - c2v (:143-152)
                    S ^= sm;
                    stq[k] = sm;
                }
            }
            // parity of the hard bits = parity of the NOT-hard bits, inverted for an odd degree
            fail |= (px ^ ((P & 1) ? 0x80008000u : 0u)) & 0x80008000u;
            if constexpr (kStationary) {
                trig = (px ^ pxp) & 0x7fff7fffu;
                pxp = px;
            }
            // Middle-out schedule of the reference's fold (:83-116): the forward chain F and the
            // backward chain B run side by side (two independent dependency chains per lane):
            // phase 1 builds F_0..F_{L-1} and B_{L+1}..B_{P-1}; phase 2 extends F rightwards and B
            // leftwards from the middle, emitting c2v_k = F_{k-1} [+] B_{k+1} on both sides.  Every
            // chain and every output is the same fold, in the same order, as the serial schedule.
            constexpr int L = (P - 1) / 2;
            uint32_t FB[P];  // FB[k] = F_k for k < L, B_k for k > L
            FB[0] = stq[0] & MAG;
            FB[P - 1] = stq[P - 1] & MAG;
#pragma unroll
            for (int j = 1; j < P - 1 - L; ++j) {
                if (j < L) FB[j] = bp_mag2<kBp>(FB[j - 1], stq[j] & MAG, C2, M2);
                FB[P - 1 - j] = bp_mag2<kBp>(FB[P - j], stq[P - 1 - j] & MAG, C2, M2);
            }
            if constexpr (CHAIN) {  // the range guard: a bound on every output from F_{L-1} and B_{L+1}
                const uint32_t G = W(C2) * (uint32_t)(L + 1);  // (L+1) C in both halves
                ovor |= (FB[L - 1] + G) | (FB[L + 1] + G);
            }
            // opaque: recompute st & MAG below instead of keeping 46 masked copies live
#pragma unroll
            for (int k = 0; k < P; ++k) asm volatile("" : "+v"(stq[k]));
            // output k: magnitude o, sign = parity of the other inputs' flags = (S ^ flag_k);
            // written back as carry-form c2v o - 2*(o & signmask) (state and scatter value), and
            // scattered into pn as soon as it is emitted (spreads the LDS atomics over phase 2)
            uint32_t F, B;  // running F_{kf-1}, B_{kb+1}
            {
                const uint32_t aL = stq[L] & MAG;
                const uint32_t o = bp_mag2<kBp>(FB[L - 1], FB[L + 1], C2, M2);
                F = bp_mag2<kBp>(FB[L - 1], aL, C2, M2);
                B = bp_mag2<kBp>(FB[L + 1], aL, C2, M2);
                emit_c2v<true, !CHAIN>(stq[L], o, S, ovor);
            }
            unsigned short uf = tL, ub = tL;
            if (!kStoreOffs && !kLdsOffs) asm volatile("" : "+v"(uf), "+v"(ub));
            // kLdsOffs: the table words of the forward / backward side's current slot pair, read one
            // pair ahead (wf_n / wb_n) so the read has a whole emission to complete
            uint32_t wf = 0, wb = 0, wf_n = 0, wb_n = 0;
            if (kLdsOffs) {  // the pair holding slot L, and the next pair on each side
                wf = wb = tword(q, L >> 1);
                if ((L >> 1) + 1 < (P + 1) / 2) wf_n = tword(q, (L >> 1) + 1);
                if ((L >> 1) >= 1) wb_n = tword(q, (L >> 1) - 1);
            }
            auto addr = [&](int k, uint32_t w, unsigned short t, uint32_t base) -> uint32_t {
                if (kStoreOffs) return soff(k, base);
                if (kLdsOffs) return lds_at<kSdwa>(w, k & 1, base);
                return base + t;
            };
            lds_add_at(addr(L, wf, tL, pn) + L * P * 4, (int)stq[L]);
#pragma unroll
            for (int j = 1; j <= (L > P - 1 - L ? L : P - 1 - L); ++j) {
                const int kf = L + j, kb = L - j;
                if (kf <= P - 1) {
                    uint32_t o = F;  // c2v_{P-1} = F_{P-2}
                    if (kf <= P - 2) {
                        o = bp_mag2<kBp>(F, FB[kf + 1], C2, M2);
                        F = bp_mag2<kBp>(F, stq[kf] & MAG, C2, M2);
                    }
                    emit_c2v<true, !CHAIN>(stq[kf], o, S, ovor);
                    if (!kStoreOffs && !kLdsOffs) {
                        uf = (unsigned short)(uf + step4);
                        uf = __builtin_elementwise_min(uf, (unsigned short)(uf - wrap4));
                    }
                    if (kLdsOffs && (kf >> 1) != ((kf - 1) >> 1)) {  // a new slot pair on this side
                        wf = wf_n;
                        if ((kf >> 1) + 1 < (P + 1) / 2) wf_n = tword(q, (kf >> 1) + 1);
                    }
                    lds_add_at(addr(kf, wf, uf, pn) + kf * P * 4, (int)stq[kf]);
                }
                if (kb >= 0) {
                    uint32_t o = B;  // c2v_0 = B_1
                    if (kb >= 1) {
                        o = bp_mag2<kBp>(FB[kb - 1], B, C2, M2);
                        B = bp_mag2<kBp>(B, stq[kb] & MAG, C2, M2);
                    }
                    emit_c2v<true, !CHAIN>(stq[kb], o, S, ovor);
                    if (!kStoreOffs && !kLdsOffs) {
                        ub = (unsigned short)(ub - step4);
                        ub = __builtin_elementwise_min(ub, (unsigned short)(ub + wrap4));
                    }
                    if (kLdsOffs && (kb >> 1) != ((kb + 1) >> 1)) {  // a new slot pair on this side
                        wb = wb_n;
                        if ((kb >> 1) >= 1) wb_n = tword(q, (kb >> 1) - 1);
                    }
                    lds_add_at(addr(kb, wb, ub, pn) + kb * P * 4, (int)stq[kb]);
                }
            }
        }
        par = fail;
        if constexpr (kStationary) par |= trig;
    }
    // Syndrome of buffer pc only (no update): bits 15 / 31 of par as in step().  The c2v state is
    // left as it is; every frame in flight ends at this step and is refilled (state cleared) or idle.
    __device__ __forceinline__ uint32_t syndrome(const uint32_t *, uint32_t pc) const {
        uint32_t fail = 0;
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            if (!act[q]) continue;
            uint32_t px = 0;
            if (kStoreOffs) {
#pragma unroll
                for (int k = 0; k < P; ++k)
                    px ^= reinterpret_cast<const lds_u32 *>((size_t)soff(k, pc))[k * P];
            } else if (kLdsOffs) {
#pragma unroll
                for (int w = 0; w < (P + 1) / 2; ++w) {
                    const uint32_t ow = tword(q, w);
                    px ^= reinterpret_cast<const lds_u32 *>((size_t)lds_at<kSdwa>(ow, 0, pc))[2 * w * P];
                    if (2 * w + 1 < P) px ^= reinterpret_cast<const lds_u32 *>((size_t)lds_at<kSdwa>(ow, 1, pc))[(2 * w + 1) * P];
                }
            } else {  // walked offsets, as in step()
                unsigned short t4 = (unsigned short)(4 * col[q]);
                const unsigned short step4 = (unsigned short)(4 * row[q]), wrap4 = (unsigned short)(4 * P);
#pragma nounroll
                for (int k = 0; k < P; ++k) {
                    px ^= reinterpret_cast<const lds_u32 *>((size_t)(pc + t4))[k * P];
                    t4 = (unsigned short)(t4 + step4);
                    t4 = __builtin_elementwise_min(t4, (unsigned short)(t4 - wrap4));
                }
            }
            fail |= (px ^ ((P & 1) ? 0x80008000u : 0u)) & 0x80008000u;
        }
        return fail;
    }
    // zero the refilled half(s) of the carry-form c2v state
    __device__ __forceinline__ void clear(int finished) {
#pragma unroll
        for (int q = 0; q < CPL; ++q)
#pragma unroll
            for (int k = 0; k < P; ++k) {
                if (finished & 1) st[q][k] -= (uint32_t)carry_lo(st[q][k]);
                if (finished & 2) st[q][k] = (uint32_t)carry_lo(st[q][k]);
            }
    }

    // ---- The stationary exit's verification (flood_pk, DESIGN.md "Stationary exit (round 15)") ----
    // After a step the state st[0][k] is the c2v of the update just made.  stat_verify leaves it in this
    // workgroup's slice of global scratch ([P][NT] words: slot k of every lane is one coalesced row) and,
    // with `compare` (wave-uniform), first reads what the call of the step before left there.  It
    // returns the OR over the slots of old ^ new, both with the carry form's borrow undone (x + 2 (x &
    // 0x8000): the high half alone), so bits 0-15 / 16-31 are zero iff every c2v of the lane's check in
    // the low / high frame is what it was one update earlier.  In the split form (one frame, state word
    // j the pair c2v_j, c2v_{P-1-j}) the same over SLOTS = SL + 1 words, and any set bit is a change.
    // One instruction stream with a branch round each batch's loads: as two instantiations hipcc merged
    // the arms' common prefix, all P borrow terms at once, and the kernel spilled.  The slice address (the
    // caller's) and the lane index are opaque, or the P / G row addresses are hoisted out of the step
    // loop and held in registers across the check step; the scheduling barriers keep the unit's max-ILP
    // scheduler from issuing every load first, and the change word is pinned after each batch, or its
    // XORs sink to the end and every old and new word stays live till then.
    static constexpr bool kStationary = CPL == 1 && kStoreOffs;
    static constexpr int kStatWords = P * NT;  // scratch words per workgroup
    static constexpr int kStatSlots = P;       // state words compared in the packed form
    static constexpr int kStatSplitSlots = (P - 1) / 2 + 1;  // in the split form (the pairs S[0..SL])
    // HOLD (the split tail's cycle exit, DESIGN.md "Cycle exit (round 21)"): with `keep` (wave-uniform) the
    // rows are compared and left as they are -- a snapshot held over several steps -- through a branch
    // round each batch's stores, in the same one instruction stream; the split form has the registers
    // for eight loads in flight.  Without HOLD the code is what it was.
    template <int SLOTS, bool HOLD = false>
    __device__ __forceinline__ uint32_t stat_verify(uint32_t *slice, int tid, bool compare, bool keep = false) const {
        uint32_t chg = 0;
        constexpr int G = HOLD ? 8 : 4;  // loads in flight per lane
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int k0 = 0; k0 < SLOTS; k0 += G) {
            uint32_t *const p = slice + k0 * NT;
            uint32_t old[G] = {};
            if (compare) {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (k0 + g < SLOTS) old[g] = p[g * NT + tid];
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (HOLD) {
                uint32_t nw[G] = {};
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int k = k0 + g;
                    if (k >= SLOTS) break;
                    const uint32_t x = st[0][k];
                    nw[g] = x + ((x & 0x8000u) << 1);
                    chg |= old[g] ^ nw[g];
                }
                if (!keep) {
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        if (k0 + g < SLOTS) p[g * NT + tid] = nw[g];
                }
            } else {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int k = k0 + g;
                    if (k >= SLOTS) break;
                    const uint32_t x = st[0][k], nw = x + ((x & 0x8000u) << 1);
                    chg |= old[g] ^ nw;
                    p[g * NT + tid] = nw;
                }
            }
            asm volatile("" : "+v"(chg));  // (this batch's words are dead from here on)
            __builtin_amdgcn_sched_barrier(0);
        }
        return compare ? chg : 0u;
    }

    // ---- The tail: one frame, its check split over the lane's two halves (flood_pk) ----
    // Once the work queue is empty a workgroup whose partner half has gone idle carries ONE frame,
    // and its packed lanes would spend every instruction's second half on nothing -- the launch then
    // waits on such frames, each at a lone workgroup's step latency.  In the split form the frame sits
    // in half 0 of the LDS words and lane halves fold the two ends of the same check: the low half
    // owns slots j = 0..L-1 (the forward chain F_0..F_{L-1}), the high half slots P-1-j (the backward
    // chain B_{P-1}..B_{L+1}), both the middle slot L -- SplitCore's middle-out schedule with the two
    // sides in the halves of one lane instead of in lanes l and l + 32, the exchange a 16-bit rotate.
    // The same chains and outputs in the same order (:83-116); L + 1 state words per lane, and about
    // 55 % of the packed step's instructions for the one frame.
    static constexpr bool kSplit = CPL == 1 && kStoreOffs;
    static constexpr int SL = (P - 1) / 2;
    static __device__ __forceinline__ uint32_t rot16(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 16); }
    // state of the frame in half h (the other half's c2v is zero) -> split pairs (c2v_j, c2v_{P-1-j})
    __device__ __forceinline__ void split_enter(int h) {
        uint32_t(&S)[P] = st[0];
#pragma unroll
        for (int j = 0; j <= SL; ++j) {
            const uint32_t a = S[j], b = S[P - 1 - j];
            const int ca = h ? (int)(a - (uint32_t)carry_lo(a)) >> 16 : carry_lo(a);
            const int cb = h ? (int)(b - (uint32_t)carry_lo(b)) >> 16 : carry_lo(b);
            S[j] = (uint32_t)ca + ((uint32_t)cb << 16);  // carry form lo + 65536 hi (j = L: both c2v_L)
        }
#pragma unroll
        for (int j = SL + 1; j < P; ++j) S[j] = 0;
    }
    __device__ __forceinline__ void split_step(const uint32_t *, uint32_t *, uint32_t pc, uint32_t pn, u16x2 C2,
                                               uint32_t M2, uint32_t &par, uint32_t &ovor) {
        constexpr uint32_t SGN = 0x80008000u, MAG = 0x7fff7fffu;
        constexpr int L = SL, J = L + 1;
        par = 0;
        if (!act[0]) return;
        uint32_t(&S)[P] = st[0];
        // Gather, software-pipelined in batches of 4 pairs as the packed step: own slot j's posterior
        // word and slot P-1-j's, combined into (half 0 of j, half 0 of P-1-j); v2c = that - c2v.
        constexpr int G4 = 4, NB = (J + G4 - 1) / G4;
        uint32_t Va[2][G4], Vc[2][G4];
        auto issue = [&](int b) {
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int j = b * G4 + g;
                if (j >= J) break;
                Va[b & 1][g] = reinterpret_cast<const lds_u32 *>((size_t)soff(j, pc))[j * P];
                if (j < L) Vc[b & 1][g] = reinterpret_cast<const lds_u32 *>((size_t)soff(P - 1 - j, pc))[(P - 1 - j) * P];
            }
        };
        uint32_t px = 0, Sg = 0, VL = 0;
        issue(0);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) issue(b + 1);
            __builtin_amdgcn_sched_barrier(0);
            const int j0 = b * G4;
            uint32_t u[G4];
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int j = j0 + g;
                if (j >= J) break;
                const uint32_t a = Va[b & 1][g];
                const uint32_t V = __builtin_amdgcn_perm(j < L ? Vc[b & 1][g] : a, a, 0x05040100u);
                if (j < L) px ^= V;  // bits 15 / 31: NOT hard of slots j / P-1-j (:305-308)
                else VL = a;
                u[g] = V - S[j];
            }
            if (j0 + G4 <= J) {
                sign_mag_b_xg<G4>(u);
            } else {
#pragma unroll
                for (int g = 0; g < G4; ++g)
                    if (j0 + g < J) u[g] = sign_mag_b(u[g], SGN);
            }
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int j = j0 + g;
                if (j >= J) break;
                if (j < L) Sg ^= u[g];
                S[j] = u[g];
            }
        }
        // the whole check's sign and syndrome parities (each half holds one side's), in both halves
        Sg ^= rot16(Sg) ^ S[L];
        px ^= rot16(px) ^ VL;
        par = (px ^ ((P & 1) ? 0x80008000u : 0u)) & 0x8000u;
        if constexpr (kStationary) {  // the trigger, as in step_g (the whole check's XOR is in both halves)
            par |= (px ^ pxp) & 0x7fffu;
            pxp = px;
        }
        // phase 1: each half's chain over its own slots
        uint32_t X[L];
        X[0] = S[0] & MAG;
#pragma unroll
        for (int j = 1; j < L; ++j) X[j] = bp_mag2<kBp>(X[j - 1], S[j] & MAG, C2, M2);
#pragma unroll
        for (int j = 0; j < J; ++j) asm volatile("" : "+v"(S[j]));  // recompute S & MAG below
        // phase 2: the other half's chain end, the middle output, then that chain extended outwards
        // through own slots (low half: B_L..B_1, high half: F_L..F_{P-2}), emitting as it goes
        const uint32_t R = rot16(X[L - 1]);
        {
            const uint32_t o = bp_mag2<kBp>(X[L - 1], R, C2, M2);
            uint32_t Y = bp_mag2<kBp>(R, S[L] & MAG, C2, M2);
            emit_c2v<true>(S[L], o, Sg, ovor);
            lds_add_at(soff(L, pn) + L * P * 4, carry_lo(S[L]));
#pragma unroll
            for (int j = L - 1; j >= 0; --j) {
                uint32_t oj = Y;  // own slot 0 / P-1: the extended chain itself
                if (j >= 1) {
                    oj = bp_mag2<kBp>(X[j - 1], Y, C2, M2);
                    Y = bp_mag2<kBp>(Y, S[j] & MAG, C2, M2);
                }
                emit_c2v<true>(S[j], oj, Sg, ovor);
                const int lo = carry_lo(S[j]);
                lds_add_at(soff(j, pn) + j * P * 4, lo);
                lds_add_at(soff(P - 1 - j, pn) + (P - 1 - j) * P * 4, (int)(S[j] - (uint32_t)lo) >> 16);
            }
        }
    }
};

// The A policy with the per-output range guard (every c2v magnitude OR-ed into ovor): the same
// kernel for parameter sets whose G = (L+1) C is too large a share of cmax for the chain guard
// (large FRAC_WIDTH; choose_kernel).
template <int P>
struct ArrayChecksOutGuard : ArrayChecks<P> {
    __device__ __forceinline__ void step(const KArgs &a, const uint32_t *pcp, uint32_t *pnp, uint32_t pc, uint32_t pn,
                                         u16x2 C2, uint32_t M2, uint32_t &par, uint32_t &ovor) {
        this->template step_g<false>(a, pcp, pnp, pc, pn, C2, M2, par, ovor);
    }
};

// Exchange of one value between lanes l and l + 32 of a wave (gfx950 v_permlane32_swap): the
// builtin swaps the upper half of its first operand with the lower half of its second, so with both
// operands x, r[0] ^ r[1] ^ x is the partner's x in every lane (two full-rate XORs, no select).
__device__ __forceinline__ uint32_t partner32(uint32_t x) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return r[0] ^ r[1] ^ x;
}

// Check side of the packed kernel, array codes, TWO lanes per check: lanes l and l + 32 of a wave
// hold check c = 32 * wave + (l & 31).  Side 0 (l < 32) owns slots 0..L-1, side 1 slots P-1..L+1
// (stored in that order, so both sides run the same instruction stream), and both hold the middle
// slot L (P = 2L + 1).  Each side folds its own slots into its chain (side 0 the forward chain
// F_0..F_{L-1}, side 1 the backward chain B_{P-1}..B_{L+1}), the two chain ends are exchanged once
// (v_permlane32_swap), and each side then extends the OTHER side's chain through its own slots --
// from the middle outwards -- emitting c2v_k = F_{k-1} [+] B_{k+1} for its own k.  These are the
// middle-out schedule's chains and outputs (ArrayChecks, :83-116) split between two lanes: the same
// box-plus operations in the same order per chain, L + 1 fold steps per lane instead of 2L + 1, so a
// frame pair's check step has half the latency on a lone workgroup and twice the waves per frame.
// (sxor is commutative -- min, |x|+|y| and ||x|-|y|| are symmetric -- though not associative, so a
// side 1 operand order such as B_{L+1} [+] F_{L-1} gives the reference's F_{L-1} [+] B_{L+1}.)
// The middle output is computed by both sides (identical) and scattered by side 0 only; the sign
// parity S and the syndrome parity are combined over both sides with one exchange each.
// Offsets: own slot j of side s is slot k = s ? P-1-j : j, at byte offset 4 * (P*k + (col + row*k)
// mod P) (< 64 KiB), two per VGPR.
template <int P>
struct SplitCore {
    static_assert(P % 2 == 1, "odd P");
    static constexpr int L = (P - 1) / 2;  // the middle slot; own slots j = 0..L-1, the middle at j = L
    static constexpr int J = L + 1;        // state words S[0..J)
    static constexpr int OW = (J + 1) / 2; // offset words S[J..J+OW), two 16-bit slot offsets each
    static constexpr int NS = J + OW;
    static constexpr bool kSdwa = true;
    template <int N>
    static __device__ __forceinline__ uint32_t soff(const uint32_t (&S)[N], int j, uint32_t base) {
        return lds_at<kSdwa>(S[J + (j >> 1)], j & 1, base);
    }
    // state zero, offsets of check (row, col) on this side
    template <int N>
    static __device__ __forceinline__ void init(uint32_t (&S)[N], bool act, uint32_t row, uint32_t col, int side) {
        static_assert(N >= NS, "state array too small");
#pragma unroll
        for (int i = 0; i < NS; ++i) S[i] = 0;
        if (act) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const uint32_t k = side ? (uint32_t)(P - 1 - j) : (uint32_t)j;
                const uint32_t o = 4u * (P * k + (col + row * k) % P);
                S[J + (j >> 1)] |= o << (16 * (j & 1));
            }
        }
    }
    template <int N>
    static __device__ __forceinline__ void step(uint32_t (&S)[N], bool act, uint32_t keepL, uint32_t pc, uint32_t pn, u16x2 C2,
                                                uint32_t M2, uint32_t &par, uint32_t &ovor) {
        constexpr uint32_t SGN = 0x80008000u, MAG = 0x7fff7fffu;
        par = 0;
        if (!act) return;
        // Gather (software-pipelined in batches of 4, as ArrayChecks): S[j] = v2c in sign-magnitude
        constexpr int G4 = 4, NB = (J + G4 - 1) / G4;
        uint32_t Vb[2][G4];
        uint32_t px = 0, Sg = 0, VL = 0;
        auto issue = [&](int b) {
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int j = b * G4 + g;
                if (j >= J) break;
                Vb[b & 1][g] = *reinterpret_cast<const lds_u32 *>((size_t)soff(S, j, pc));
            }
        };
        issue(0);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) issue(b + 1);
            __builtin_amdgcn_sched_barrier(0);
            const int j0 = b * G4;
            if (j0 + G4 <= J) {
                uint32_t u[G4];
#pragma unroll
                for (int g = 0; g < G4; ++g) u[g] = Vb[b & 1][g] - S[j0 + g];
                sign_mag_b_xg<G4>(u);
#pragma unroll
                for (int g = 0; g < G4; ++g) S[j0 + g] = u[g];
            } else {
#pragma unroll
                for (int g = 0; g < G4; ++g) {
                    const int j = j0 + g;
                    if (j >= J) break;
                    S[j] = sign_mag_b(Vb[b & 1][g] - S[j], SGN);
                }
            }
#pragma unroll
            for (int g = 0; g < G4; ++g) {
                const int j = j0 + g;
                if (j >= J) break;
                if (j < L) {
                    px ^= Vb[b & 1][g];  // bits 15 / 31: NOT hard (:305-308)
                    Sg ^= S[j];
                } else {
                    VL = Vb[b & 1][g];
                }
            }
        }
        // Phase 1: this side's chain over its own slots
        uint32_t X[L];
        X[0] = S[0] & MAG;
#pragma unroll
        for (int j = 1; j < L; ++j) X[j] = bp_mag2<kBpMany>(X[j - 1], S[j] & MAG, C2, M2);
#pragma unroll
        for (int j = 0; j < J; ++j) asm volatile("" : "+v"(S[j]));  // recompute S & MAG below
        // the exchange: the partner's chain end, sign parity and syndrome parity
        const uint32_t R = partner32(X[L - 1]);
        Sg ^= partner32(Sg) ^ S[L];
        px ^= partner32(px) ^ VL;
        par = (px ^ ((P & 1) ? 0x80008000u : 0u)) & 0x80008000u;
        // Phase 2: the middle output, then the partner's chain extended outwards through own slots
        {
            const uint32_t o = bp_mag2<kBpMany>(X[L - 1], R, C2, M2);
            const uint32_t aL = S[L] & MAG;
            uint32_t Y = bp_mag2<kBpMany>(R, aL, C2, M2);
            emit_c2v<true>(S[L], o, Sg, ovor);
            lds_add_at(soff(S, L, pn), (int)(S[L] & keepL));
#pragma unroll
            for (int j = L - 1; j >= 0; --j) {
                uint32_t oj = Y;  // own slot 0's output: the extended chain itself
                if (j >= 1) {
                    oj = bp_mag2<kBpMany>(X[j - 1], Y, C2, M2);
                    Y = bp_mag2<kBpMany>(Y, S[j] & MAG, C2, M2);
                }
                emit_c2v<true>(S[j], oj, Sg, ovor);
                lds_add_at(soff(S, j, pn), (int)S[j]);
            }
        }
    }
    // Syndrome of buffer pc only (no update), bits 15 / 31 as in step()
    template <int N>
    static __device__ __forceinline__ uint32_t syndrome(const uint32_t (&S)[N], bool act, uint32_t pc) {
        if (!act) return 0;
        uint32_t px = 0;
#pragma unroll
        for (int j = 0; j < L; ++j) px ^= *reinterpret_cast<const lds_u32 *>((size_t)soff(S, j, pc));
        const uint32_t VL = *reinterpret_cast<const lds_u32 *>((size_t)soff(S, L, pc));
        px ^= partner32(px) ^ VL;
        return (px ^ ((P & 1) ? 0x80008000u : 0u)) & 0x80008000u;
    }
    // zero the refilled half(s) of the state words (the offset words are left alone)
    template <int N>
    static __device__ __forceinline__ void clear(uint32_t (&S)[N], int finished) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (finished & 1) S[j] -= (uint32_t)carry_lo(S[j]);
            if (finished & 2) S[j] = (uint32_t)carry_lo(S[j]);
        }
    }
};

// R-sized array codes (1024 < m <= NT + 256 + 128): the LDS-offset-table policy with 2 checks per lane
// for checks [0, NT + 256) -- the second check on threads [0, 256) only -- and the remaining checks
// (R: 104) two lanes per check (SplitCore) on threads [256, 512), their state and offsets in the
// words of the second-check state those lanes do not use.  R's 1128 checks are 17.6 wave-units of
// one check per lane: as 2 checks per lane they load the SIMDs 5 / 5 / 4 / 4 per step (some SIMD
// carries two second-pass units); here every SIMD carries 3 + 1 whole units and one split unit of
// half the work, 4.5.
template <int P, int NT = 768>
struct MixChecks {
    static constexpr bool kSplit = false;
    static constexpr bool kStationary = false;
    static constexpr int kRefillBatch = 0;
    using Reg = ArrayChecks<P, 2, NT, true, true>;
    using Sp = SplitCore<P>;
    static_assert(Sp::NS <= P, "split state must fit a check's state words");
    static constexpr int kN = P * P;
    static constexpr int kTabWords = Reg::kTabWords;
    static constexpr int kSplitBase = NT + 256;  // first split check
    Reg reg;
    uint32_t keepL;
    bool split_lane, sact;
    __device__ __forceinline__ void init(const KArgs &a, int tid_in, uint32_t *tab) {
        // Roles of the three 256-thread blocks of waves (one wave of each per SIMD): the oldest block
        // (threads 0..255) takes one whole check + the split units, the middle block the two whole
        // checks, the youngest one whole check.  Round 6's per-wave stamps (FPLDPC_WAIT_TRACE) showed
        // the hardware's age-ordered issue finishing the oldest, heaviest waves first and parking them
        // at the step barrier for 36 % of their time; of the six role orders measured
        // (profiles/r6/ab/r_roles.txt) this one ran fastest, and with wave priorities 1 / 0 / 2 on top
        // R went 666 -> 677 Mb/s (r_prio.txt, r_prio2.txt).  Since the quick exit between steps the
        // priorities cost 0.3-0.4 % (profiles/r6/ab/r_prio_quick.txt) and are gone.  `u` is the lane's
        // check index as before (the same 32-lane pairs for the split units: u & 63 == tid & 63).
        // (roles as hex digits, block b in digit b)
        constexpr int kRoles = 0x201;
        const int tid = ((kRoles >> (4 * (tid_in >> 8))) & 0xf) * 256 + (tid_in & 255);
        reg.init(a, tid, tab);
        reg.act[1] = reg.act[1] && tid < 256;
        split_lane = tid >= 256 && tid < 512;
        const int l = tid & 63, side = l >> 5;
        const int c = kSplitBase + ((tid - 256) >> 6) * 32 + (l & 31);
        sact = split_lane && c < a.m;
        keepL = side ? 0u : ~0u;
        if (split_lane) Sp::init(reg.st[1], sact, sact ? (uint32_t)(c / P) : 0u, sact ? (uint32_t)(c % P) : 0u, side);
    }
    __device__ __forceinline__ void step(const KArgs &a, const uint32_t *pcp, uint32_t *pnp, uint32_t pc, uint32_t pn, u16x2 C2,
                                         uint32_t M2, uint32_t &par, uint32_t &ovor) {
        reg.step(a, pcp, pnp, pc, pn, C2, M2, par, ovor);
        if (split_lane) {
            uint32_t p2 = 0;
            Sp::step(reg.st[1], sact, keepL, pc, pn, C2, M2, p2, ovor);
            par |= p2;
        }
    }
    __device__ __forceinline__ uint32_t syndrome(const uint32_t *pcp, uint32_t pc) const {
        uint32_t f = reg.syndrome(pcp, pc);
        if (split_lane) f |= Sp::syndrome(reg.st[1], sact, pc);
        return f;
    }
    __device__ __forceinline__ void clear(int finished) {
        // the second check's words beyond the split state hold the split offsets on split lanes
        uint32_t keep[Sp::OW];
#pragma unroll
        for (int w = 0; w < Sp::OW; ++w) keep[w] = reg.st[1][Sp::J + w];
        reg.clear(finished);
        if (split_lane) {
#pragma unroll
            for (int w = 0; w < Sp::OW; ++w) reg.st[1][Sp::J + w] = keep[w];
        }
    }
};

}  // namespace
}  // namespace fpldpc
