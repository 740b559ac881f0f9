// fpldpc_flood_pk.hpp -- flood_pk, the packed flooding kernel: two frames per lane (one per 16-bit
// half), the halves refilled independently, a lone last frame continued in the policy's split form.
// The check side is the policy CK (fpldpc_flood_checks_array.hpp, fpldpc_flood_checks_table.hpp), which
// the including unit brings itself.  Included by fpldpc_kernels.hip, fpldpc_kernels_a1.hip and
// fpldpc_kernels_w1.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "fpldpc_flood_device.hpp"
#include "fpldpc_flood_packed.hpp"

// flood_pk's diagnostic builds (-DFPLDPC_PHASE_TRACE, -DFPLDPC_WAIT_TRACE: tools/wait_trace.py,
// -DFPLDPC_TAIL_TRACE: tools/tail_trace.py; read with tools/wg_trace.py).  The shipped build defines
// none of them, and the macros below expand to nothing or to a plain barrier.
// FPLDPC_PHASE_TRACE: thread 0's s_memrealtime ticks between PH_T0(v) and PH_ADD(acc, v).
#if FPLDPC_PHASE_TRACE
#define PH_T0(v) const unsigned long long v = (tid == 0) ? __builtin_amdgcn_s_memrealtime() : 0ull
#define PH_ADD(acc, v) if (tid == 0) acc += __builtin_amdgcn_s_memrealtime() - v
#else
#define PH_T0(v)
#define PH_ADD(acc, v)
#endif
// FPLDPC_WAIT_TRACE = 1: PK_SYNC, the barriers of the packed loop other than the per-step one (refills,
// stores, the final-update syndrome pass, the range check), adds its wait to wt_bar2.
// FPLDPC_WAIT_TRACE = 2: word 4 holds the per-step LLR copy instead; 3: everything after the per-step
// barrier (decisions, stores, refills).
#if FPLDPC_WAIT_TRACE
#if FPLDPC_WAIT_TRACE >= 2
#define PK_SYNC() __syncthreads()
#else
#define PK_SYNC()                                                         \
    do {                                                                  \
        const unsigned long long pk_t = __builtin_amdgcn_s_memtime();     \
        __syncthreads();                                                  \
        wt_bar2 += __builtin_amdgcn_s_memtime() - pk_t;                   \
    } while (0)
#endif
#else
#define PK_SYNC() __syncthreads()
#endif

namespace fpldpc {
namespace {

// (the tail's split step, for the policies that have one)
template <class CK>
__device__ __forceinline__ void split_step_of(CK &ck, const uint32_t *pcp, uint32_t *pnp, uint32_t pc, uint32_t pn,
                                              u16x2 C2, uint32_t M2, uint32_t &par, uint32_t &ovor) {
    if constexpr (CK::kSplit) ck.split_step(pcp, pnp, pc, pn, C2, M2, par, ovor);
}

// flood_pk's stationary-exit control words (wave-uniform), for the policies that have the exit
template <bool ON>
struct StatCtl {};
template <>
struct StatCtl<true> {
    int stat, sexit;  // a step's decisions: halves verified stationary / ending by that alone
    int vsk;          // (across set_quick at a refill: the on-bits, and the other half's state << 16)
    // The exit's state between steps rides in flood_pk's q_live word, which the step loop holds in a
    // register anyway (every SGPR more that lives across the check step costs spills in it):
    //   bits 0-1   the live halves, whose fail flags the quick exit wants set (as without the exit)
    //   bits 2-3   the same halves' `changed` flags, wanted too -- set only while the exit is on
    //   bits 16-19 the verification state vs, two bits per half (1: the coming step stores, 2: it
    //              compares); no flag word has these bits, so the quick exit is not taken meanwhile
    // A flag word (misc[6..8]) only ever carries bits 0-6: fail (0, 1), changed (2, 3), the compare's
    // result (4, 5) and, in the split loop only, the cycle exit's arming bit (6: some live check lane's
    // posterior hash did not change).  Bits 16-19 of q_live must stay outside that set (kFlagBits), and
    // both loops read the state through on() / vs() only.
    static constexpr int kFlagBits = 0x7f;
    static_assert((kFlagBits & 0xf0000) == 0, "the verification state must lie outside the flag bits");
    static __device__ __forceinline__ int word(int live, bool on, int vs) { return live * (on ? 5 : 1) | vs << 16; }
    static __device__ __forceinline__ bool on(int q_live) { return (q_live & 0xc) != 0; }
    static __device__ __forceinline__ int vs(int q_live) { return q_live >> 16; }
};

template <class CK, int WAVES, int NT = kNT>
__global__ void __launch_bounds__(NT, WAVES) flood_pk(KArgs a) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int n = CK::kN ? CK::kN : a.n;
    uint32_t *const bufs = reinterpret_cast<uint32_t *>(smem);  // 3 x n posteriors, biased pairs
    uint32_t *const llrc = bufs + 3 * n;                          // n channel LLRs, biased pairs
    int *const misc = smem + 4 * n;
    // misc: [0,1] frame of half h (-1 idle)  [2,3] start step  [4,5] load taint  [6..8] flag words
    //       [12] final-pass syndrome word  [13] deferred range-check word
    //       [9,10] bit-error accumulators  [14] frames this workgroup ended by the stationary exit
    //       [15] frames it ended by the cycle exit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u16x2 C2 = (u16x2)(unsigned short)a.C;
    uint32_t M2 = ((1u << a.bfe_w) - 1u) * 0x10001u;
    {  // box-plus constants in VGPRs, not SGPRs (bp_mag2)
        uint32_t c2w = W(C2);
        asm volatile("" : "+v"(c2w), "+v"(M2));
        C2 = U2(c2w);
    }

    for (int v = tid; v < 4 * n; v += NT) bufs[v] = 0x7fff7fffu;  // zero posteriors (biased pairs)
    if (tid < kMiscInts) misc[tid] = tid < 2 ? -1 : 0;
    CK ck;
    ck.init(a, tid, reinterpret_cast<uint32_t *>(smem + 4 * n + kMiscInts));  // (array LDS-offset table)
    constexpr int kRB = CK::kRefillBatch;  // refill: LLR words per thread in flight (0: one at a time)
    // kRB > 0: the masked-BER info positions / reference bits ([2][hard_words], the same for every
    // frame of the call) staged in LDS after the check table, so a frame's store reads no global
    // memory on its critical path (variant_lds reserves the words)
    uint32_t *const lmask = reinterpret_cast<uint32_t *>(smem + 4 * n + kMiscInts) + (size_t)a.m * CK::kTabWords;
    if (kRB > 0 && a.info_mask && a.k_info > 0)
        for (int i = tid; i < 2 * a.hard_words; i += NT) lmask[i] = a.info_mask[i];
    uint32_t ovf = 0;
    bool taint[2] = {false, false};
    __syncthreads();

    unsigned long long trace_t0 = 0;
    int trace_frames = 0;  // thread 0: frames pulled (diagnostic trace)
#if FPLDPC_PHASE_TRACE
    // diagnostic build only: thread 0's s_memrealtime ticks in the refills, the frame pulls inside
    // them (FPLDPC_PHASE_TRACE=2: the stores' ballot loops instead; 3: the refills' part up to the
    // second barrier) and the stores, and the steps run (3: the refills' load loops) (trace words 4..7)
    unsigned long long ph_refill = 0, ph_pull = 0, ph_store = 0, ph_steps = 0, ph_sloop = 0, ph_rhead = 0, ph_rload = 0;
#endif
#if FPLDPC_WAIT_TRACE
    // diagnostic build only (tools/wait_trace.py): per wave, s_memtime cycles in the packed loop's
    // check step, at its per-step barrier, and in the whole packed loop, written after the
    // [grid][8] trace words as [grid][64]: wave w's {step, barrier, loop, steps, other barriers} at
    // 5w..5w+4 (up to 12 waves)
    unsigned long long wt_step = 0, wt_bar = 0, wt_loop0 = __builtin_amdgcn_s_memtime(), wt_steps = 0, wt_bar2 = 0;
#endif
#if FPLDPC_TAIL_TRACE
    // diagnostic build only (tools/tail_trace.py): thread 0's s_memrealtime when a pull first found
    // the queue empty and when the workgroup entered the split tail, and the steps it then ran with
    // two live frames, one live frame (packed) and in the split form (trace words 4..7)
    unsigned long long tt_empty = 0, tt_split = 0, tt_two = 0, tt_one = 0, tt_splits = 0;
    int tt_frame = -1;  // the frame the workgroup carried into the split form (word 3, bits 32-63: id + 1)
#endif
    // (Re)fill the halves in `mask` before step s: new frames' LLRs into llrc, into the buffer
    // read at step s (pc) and the one accumulated at step s (pn); c2v state and overflow trackers
    // of the half cleared.  Uniform control flow (every thread calls it with the same arguments).
    auto refill = [&](int mask, int s, int cur_next) {
        PH_T0(ph_r0);
        // kRB > 0: one atomic for every refilled half, issued before the barrier so that its round
        // trip overlaps the wait (frames wi, wi + 1 in half order, as two pulls in a row would give)
        int got[2] = {-1, -1};
        if (kRB > 0 && tid == 0) {
            const int wi = atomicAdd(a.work_counter, (mask & 1) + (mask >> 1));
            const int lim = a.frame_list ? *a.frame_count : a.batch;
            const int w1 = wi + (mask & 1);
            if ((mask & 1) && wi < lim) got[0] = a.frame_list ? a.frame_list[wi] : wi;
            if ((mask & 2) && w1 < lim) got[1] = a.frame_list ? a.frame_list[w1] : w1;
        }
        // every wave has finished reading misc[0..3] (finish decision, store) before thread 0
        // replaces the frame ids and start steps
        PK_SYNC();
        if (tid == 0) {
            misc[13] = 0;  // deferred range-check word (read by every wave before the barrier above)
            for (int h = 0; h < 2; ++h)
                if (mask >> h & 1) {
                    PH_T0(ph_p0);
                    misc[h] = kRB > 0 ? got[h] : pull_frame(a, a.work_counter);
                    PH_ADD(ph_pull, ph_p0);
#if FPLDPC_TAIL_TRACE
                    if (misc[h] < 0 && !tt_empty) tt_empty = __builtin_amdgcn_s_memrealtime();
#endif
                    trace_frames += misc[h] >= 0;
                    misc[2 + h] = s;
                    misc[4 + h] = 0;
                    misc[9 + h] = 0;
                }
        }
        PK_SYNC();
        PH_ADD(ph_rhead, ph_r0);
        PH_T0(ph_l0);
        uint32_t *pc = bufs + cur_next * n;
        uint32_t *pn = bufs + ((cur_next + 1) % 3) * n;
        if constexpr (kRB > 0) {
            // both refilled halves at once, kRB words per thread with their loads in flight
            // together, one read-modify-write of each LDS word for both halves
            constexpr int KB = kRB > 0 ? kRB : 1;
            const int f0 = (mask & 1) ? misc[0] : -1, f1 = (mask & 2) ? misc[1] : -1;
            bool big0 = false, big1 = false;
            int v0 = tid;
            asm volatile("" : "+v"(v0));
            auto ld = [&](int f, int v) -> int {
                const size_t i = (size_t)f * n + v;
                return a.llr_i16 ? (int)static_cast<const int16_t *>(a.llr)[i] : static_cast<const int32_t *>(a.llr)[i];
            };
            for (int vb = v0; vb < n; vb += KB * NT) {
                int x0[KB], x1[KB];
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int v = vb + j * NT;
                    x0[j] = (v < n && f0 >= 0) ? ld(f0, v) : 0;
                    x1[j] = (v < n && f1 >= 0) ? ld(f1, v) : 0;
                }
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int v = vb + j * NT;
                    if (v < n) {
                        if (x0[j] > kLlrMax || x0[j] < -kLlrMax) {
                            big0 = true;
                            x0[j] = 0;
                        }
                        if (x1[j] > kLlrMax || x1[j] < -kLlrMax) {
                            big1 = true;
                            x1[j] = 0;
                        }
                        uint32_t L = llrc[v], C = pc[v], N = pn[v];
                        if (mask & 1) {
                            L = bias_set(L, 0, x0[j]);
                            C = bias_set(C, 0, x0[j]);
                            N = bias_set(N, 0, x0[j]);
                        }
                        if (mask & 2) {
                            L = bias_set(L, 1, x1[j]);
                            C = bias_set(C, 1, x1[j]);
                            N = bias_set(N, 1, x1[j]);
                        }
                        llrc[v] = L;
                        pc[v] = C;
                        pn[v] = N;
                    }
                }
            }
            if (big0) atomicOr(&misc[4], 1);
            if (big1) atomicOr(&misc[5], 1);
        }
        for (int h = 0; h < 2 && kRB == 0; ++h) {
            if (!(mask >> h & 1)) continue;
            const int f = misc[h];
            bool big = false;
            // (an opaque start, so the loop's per-lane bounds are not hoisted out of the step loop
            // and held in VGPRs across it -- A 163 -> 142 VGPRs, +4.7 %; R's spills gone,
            // profiles/r3/ab/opaque_loops*.txt)
            int v0 = tid;
            asm volatile("" : "+v"(v0));
            for (int v = v0; v < n; v += NT) {
                int x = 0;
                if (f >= 0) {
                    const size_t i = (size_t)f * n + v;
                    x = a.llr_i16 ? (int)static_cast<const int16_t *>(a.llr)[i] : static_cast<const int32_t *>(a.llr)[i];
                    if (x > kLlrMax || x < -kLlrMax) {
                        big = true;
                        x = 0;
                    }
                }
                llrc[v] = bias_set(llrc[v], h, x);
                pc[v] = bias_set(pc[v], h, x);
                pn[v] = bias_set(pn[v], h, x);
            }
            if (big) atomicOr(&misc[4 + h], 1);
        }
        PH_ADD(ph_rload, ph_l0);
        PK_SYNC();
        PH_ADD(ph_refill, ph_r0);
    };

    // Outputs of the frame in half h: posteriors / hard decisions from buffer pf (biased pairs),
    // or the channel decision on a pre-check pass (posteriors left untouched).
    // calculateBER (ArrayLDPC_Decoder.cpp:707-722) with distinct info positions (a.info_mask) comes
    // out of the hard-decision ballots: errors = popcount((hard ^ ref) & mask) per 32 variables,
    // instead of a gather of k_info scattered posteriors and their index / bit tables per frame.
    // The workgroup's totals are summed in LDS and added to a.totals once, at exit.
    auto store = [&](int h, const uint32_t *pf, bool pre, int iters, int ok) {
        PH_T0(ph_s0);
        const int f = misc[h];
        int v0 = tid, b0 = wave * 64;  // opaque loop starts (see refill)
        asm volatile("" : "+v"(v0), "+v"(b0));
        if (a.post && !pre)
            for (int v = v0; v < n; v += NT) a.post[(size_t)f * n + v] = bias_half(pf[v], h);
        const bool masked = a.k_info > 0 && a.info_mask;
        if (kRB > 0 && (a.hard || masked)) {
            // kRB > 0: the posterior words of four ballots read together, the info masks from LDS
            uint32_t *hd = a.hard ? a.hard + (size_t)f * a.hard_words : nullptr;
            int e = 0;
            for (int base = b0; base < n; base += 4 * NT) {
                uint32_t pv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = base + j * NT + lane;
                    pv[j] = v < n ? pf[v] : 0u;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int bj = base + j * NT;
                    if (bj >= n) break;
                    const unsigned long long b = __ballot(bj + lane < n && bias_half(pv[j], h) <= 0);
                    if (lane == 0) {
                        const int w = bj >> 5;
                        const bool two = w + 1 < a.hard_words;
                        if (hd) {
                            hd[w] = (uint32_t)b;
                            if (two) hd[w + 1] = (uint32_t)(b >> 32);
                        }
                        if (masked) {
                            const uint32_t *mk = lmask, *rf = lmask + a.hard_words;
                            e += __popc(((uint32_t)b ^ rf[w]) & mk[w]);
                            if (two) e += __popc(((uint32_t)(b >> 32) ^ rf[w + 1]) & mk[w + 1]);
                        }
                    }
                }
            }
            if (masked && e) atomicAdd(&misc[9 + h], e);
            PH_ADD(ph_sloop, ph_s0);
        } else if (a.hard || masked) {
            uint32_t *hd = a.hard ? a.hard + (size_t)f * a.hard_words : nullptr;
            int e = 0;
            for (int base = b0; base < n; base += NT) {
                const int v = base + lane;
                const unsigned long long b = __ballot(v < n && bias_half(pf[v], h) <= 0);
                if (lane == 0) {
                    const int w = base >> 5;
                    const bool two = w + 1 < a.hard_words;
                    if (hd) {
                        hd[w] = (uint32_t)b;
                        if (two) hd[w + 1] = (uint32_t)(b >> 32);
                    }
                    if (masked) {
                        const uint32_t *mk = a.info_mask, *rf = a.info_mask + a.hard_words;
                        e += __popc(((uint32_t)b ^ rf[w]) & mk[w]);
                        if (two) e += __popc(((uint32_t)(b >> 32) ^ rf[w + 1]) & mk[w + 1]);
                    }
                }
            }
            if (masked && e) atomicAdd(&misc[9 + h], e);
        }
        int errors = 0;
        if (a.k_info > 0) {
            if (!masked) {
                int e = 0;
                for (int i = v0; i < a.k_info; i += NT) e += ((bias_half(pf[a.info_idx[i]], h) <= 0) ? 1 : 0) != a.info_bits[i];
                if (e) atomicAdd(&misc[9 + h], e);
            }
            PK_SYNC();
            errors = misc[9 + h];
        }
        if (tid == 0) {
            if (a.iters) a.iters[f] = iters;
            if (a.syn_ok) a.syn_ok[f] = (uint8_t)ok;
            if (a.bit_errors) a.bit_errors[f] = errors;
            if (a.totals) {
                misc[kTotW] += errors;
                misc[kTotW + 1] += errors > 0;
                misc[kTotW + 2] += 1;
                misc[kTotW + 3] += iters;
            }
        }
        PH_ADD(ph_store, ph_s0);
    };

    clock_probe(a, 0);
    if (a.wgtrace) trace_t0 = __builtin_amdgcn_s_memrealtime();  // every lane: a wave-uniform (SGPR) value
    refill(3, 1, 0);
    taint[0] = misc[4] != 0;
    taint[1] = misc[5] != 0;
    // Frame ids and start steps of the two halves in (wave-uniform) registers, so the per-step
    // decisions need one LDS read (the flag word) instead of a chain of dependent ones (A +1.5 %; W
    // +13.5 % together with the final-update syndrome pass below, profiles/r4/ab/w_regctl.txt --
    // round 3's table-policy build lost 4 % with it to SGPR spills).
    int frm_r[2], sst_r[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        frm_r[h] = __builtin_amdgcn_readfirstlane(misc[h]);
        sst_r[h] = __builtin_amdgcn_readfirstlane(misc[2 + h]);
    }
    auto frm = [&](int h) { return frm_r[h]; };
    auto sst = [&](int h) { return sst_r[h]; };
    // The steps after whose barrier nothing can happen -- every live half's fail flag set (no
    // pre-check or early-termination end) and s < q_until (no half at max_iter or one short of it)
    // -- skip the end decisions: 60-odd scalar instructions per wave and step, which R's twelve
    // waves (one workgroup per CU) issue one after another on the CU's scalar unit between two
    // steps (A +2.1 %, A @ 4.5 dB +3.1 %, W +2.8 %, W @ 2 dB +2.0 %, R +1.4 %,
    // profiles/r6/ab/quick_exit.txt).  q_live: the live halves (bit h), whose fail flags must be set.
    int q_live = 0, q_until = 0;
    // The stationary exit (CK::kStationary, DESIGN.md "Stationary exit (round 15)"): a frame whose c2v
    // messages are the same after two consecutive updates has reached a fixed point of the iteration --
    // every later update reproduces them, the posteriors and the syndrome -- so it ends there, reported
    // with max_iter iterations and the outputs max_iter updates give.  Per half:
    //   trigger  the check step's XOR over each check's posterior words (it has it for the syndrome) is
    //            what it was at the step before in every lane (flag bits 2 / 3: the hash of half 0 / 1
    //            changed somewhere); equal posteriors give equal hashes, and neither proves anything
    //            about the messages: the trigger only arms
    //   verify   the two steps after it run ck.stat_verify after the check step: the first stores the
    //            c2v words, the second compares (flag bits 4 / 5: some c2v of the half changed)
    //   end      no change: the half ends through the end-of-frame path below
    // On when the launch passes a scratch slice per workgroup (a.c2v_scratch; FPLDPC_STATIONARY_EXIT=0
    // passes none).  With this policy q_live carries the exit's state too (StatCtl); it is still zero
    // only when both halves are idle.
    // (StatCtl is empty for the other policies: their kernels carry no trace of it)
    [[maybe_unused]] StatCtl<CK::kStationary> sc;
    auto set_quick = [&]() {
        q_live = (frm(0) >= 0 ? 1 : 0) | (frm(1) >= 0 ? 2 : 0);
        q_until = 0x7fffffff;
        for (int h = 0; h < 2; ++h)
            if (frm(h) >= 0) q_until = min(q_until, sst(h) + a.max_iter - 1);
    };
    set_quick();
    if constexpr (CK::kStationary) q_live = sc.word(q_live, a.c2v_scratch != nullptr, 0);
    // The stationary exit's decisions after the barrier of step s, per live half; d = its completed
    // updates in pc.  A compare that found no change: the update this step made (d + 1 <= max_iter, one
    // the reference makes) reproduced the c2v of update d, so pn = pc and every later posterior equals
    // pc -- the half ends on pc (sc.stat).  Armed when the posterior hashes of updates d - 1 and d are
    // equal (d >= 1: at d = 0 the hash before was another frame's) and the compare, two steps on, still
    // comes before the last update of either half (s + 2 <= q_until, the smaller of the halves' bounds and
    // a value the loop holds anyway: the half's own a.max_iter bound cost five more SGPR spills).
    [[maybe_unused]] auto stat_decide = [&](uint32_t flags, int s) {
        if constexpr (CK::kStationary) {
            sc.stat = 0;
            sc.sexit = 0;
            if (!sc.on(q_live)) return;
            int vs = sc.vs(q_live);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (frm(h) < 0) continue;
                const int d = s - sst(h);
                int st = vs >> (2 * h) & 3;
                if (st == 2) {
                    if (!(flags >> (4 + h) & 1u)) sc.stat |= 1 << h;
                    st = 0;
                } else if (st == 1) {
                    st = 2;
                }
                if (st == 0 && !(sc.stat >> h & 1) && !(flags >> (2 + h) & 1u) && d >= 1 && s + 2 <= q_until) st = 1;
                vs = (vs & ~(3 << (2 * h))) | st << (2 * h);
            }
            q_live = (q_live & 0xffff) | vs << 16;
        }
    };
    // the verification of the step just made, while one is pending: the c2v words (the packed state's
    // P, the split form's SL + 1) against the step before's, or stored for the next; flag bits 4 / 5
    [[maybe_unused]] auto stat_check = [&](auto words_c, int s) {
        if constexpr (CK::kStationary) {
            if (!sc.vs(q_live)) return;
            unsigned wg = blockIdx.x;  // (opaque: see stat_verify)
            asm volatile("" : "+s"(wg));
            uint32_t *const slice = reinterpret_cast<uint32_t *>(a.c2v_scratch) + (size_t)wg * CK::kStatWords;
            // (split form: both halves of a state word are the one frame's, in half 0 of the control words, and
            // half 1's state bits are the cycle exit's part: 2 compares as well, and keeps the rows)
            constexpr bool kPacked = decltype(words_c)::value == CK::kStatSlots;
            const uint32_t chg = ck.template stat_verify<decltype(words_c)::value, !kPacked>(slice, tid, (sc.vs(q_live) & 0xa) != 0,
                                                                                             !kPacked && (sc.vs(q_live) & 8) != 0);
            const uint32_t lo = kPacked ? chg & 0xffffu : chg, hi = kPacked ? chg >> 16 : 0u;
            const uint32_t cb = (__ballot(lo != 0u) ? 0x10u : 0u) | (__ballot(hi != 0u) ? 0x20u : 0u);
            if (cb) atomicOr(&misc[6 + s % 3], (int)cb);
        }
    };
    int cur = 0;
    int s = 1;
    bool more = true;
    // (a half goes idle only at a refill: the tail check runs there, and once before the first step)
    bool tail = CK::kSplit && a.split_tail && (frm(0) < 0) != (frm(1) < 0);
    for (; !tail; ++s) {
        if (q_live == 0) {  // both halves idle
            clock_probe(a, 2);
            if (a.wgtrace && tid == 0) {
                unsigned long long *t = a.wgtrace + 8 * (size_t)blockIdx.x;
                t[0] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                       (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_XCC_ID, HW_REG_HW_ID
                t[1] = trace_t0;
                t[2] = __builtin_amdgcn_s_memrealtime();
                t[3] = (unsigned long long)trace_frames;
#if FPLDPC_PHASE_TRACE
                t[4] = ph_refill;
                t[5] = FPLDPC_PHASE_TRACE == 3 ? ph_rhead : FPLDPC_PHASE_TRACE == 2 ? ph_sloop : ph_pull;
                t[6] = ph_store;
                t[7] = FPLDPC_PHASE_TRACE == 3 ? ph_rload : ph_steps;
#endif
#if FPLDPC_TAIL_TRACE
                t[4] = tt_empty;
                t[5] = tt_split;
                t[6] = tt_two | tt_one << 32;
                t[7] = tt_splits;
#endif
            }
#if FPLDPC_WAIT_TRACE
            if (a.wgtrace && lane == 0) {
                unsigned long long *w = a.wgtrace + 8 * (size_t)gridDim.x + 64 * (size_t)blockIdx.x + 5 * wave;
                w[0] = wt_step;
                w[1] = wt_bar;
                w[2] = __builtin_amdgcn_s_memtime() - wt_loop0;
                w[3] = wt_steps;
                w[4] = wt_bar2;
            }
#endif
            more = false;
            break;
        }
        const uint32_t *pc = bufs + cur * n;
        uint32_t *pn = bufs + ((cur + 1) % 3) * n;
        uint32_t *pr = bufs + ((cur + 2) % 3) * n;
#if FPLDPC_WAIT_TRACE == 2
        const unsigned long long wc0 = __builtin_amdgcn_s_memtime();
#endif
        {
            int v0 = tid;  // opaque: keeps the compiler from hoisting 3 x 9 addresses across steps
            asm volatile("" : "+v"(v0));
            if (CK::kN) {
#pragma unroll
                for (int v = v0, j = 0; j < (CK::kN + NT - 1) / NT; ++j, v += NT)
                    if (j < CK::kN / NT || v < CK::kN) pr[v] = llrc[v];
            } else if ((n & 3) == 0) {  // 16-byte chunks, every buffer 16-byte aligned (W +1.3-1.4 %, W @ 2 dB +2.0 %, profiles/r6/ab/w_copy16.txt)
                const int n4 = n >> 2;
                const uint4 *l4 = reinterpret_cast<const uint4 *>(llrc);
                uint4 *p4 = reinterpret_cast<uint4 *>(pr);
                for (int vb = v0; vb < n4; vb += 2 * NT) {
                    const uint4 t0 = l4[vb];
                    uint4 t1 = {};
                    if (vb + NT < n4) t1 = l4[vb + NT];
                    p4[vb] = t0;
                    if (vb + NT < n4) p4[vb + NT] = t1;
                }
            } else {  // 8 loads in flight per thread, then 8 stores
                for (int vb = v0; vb < n; vb += 8 * NT) {
                    uint32_t t[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] = vb + j * NT < n ? llrc[vb + j * NT] : 0u;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (vb + j * NT < n) pr[vb + j * NT] = t[j];
                }
            }
        }
#if FPLDPC_WAIT_TRACE == 2
        wt_bar2 += __builtin_amdgcn_s_memtime() - wc0;
#endif
        // flag word of step s+1: last read at step s-2, and every thread has passed the barrier of
        // step s-1 since; it is next written after this step's barrier
        if (tid == 0) {
#if FPLDPC_PHASE_TRACE
            ++ph_steps;
#endif
#if FPLDPC_TAIL_TRACE
            if (tt_empty) {
                if (frm(0) >= 0 && frm(1) >= 0) ++tt_two;
                else ++tt_one;
            }
#endif
            misc[6 + (s + 1) % 3] = 0;
            misc[12] = 0;  // flag word of a final-update syndrome pass (below), read after this step's barrier
        }
        uint32_t par = 0, ovor = 0;
        // (The check step always runs: a frame's last update is checked by the final-update syndrome pass
        // below, not by one more step.)
#if FPLDPC_WAIT_TRACE
        const unsigned long long wt0 = __builtin_amdgcn_s_memtime();
#endif
        ck.step(a, pc, pn, lds_addr(pc), lds_addr(pn), C2, M2, par, ovor);
        ovf |= ovor;
        if constexpr (CK::kStationary) stat_check(std::integral_constant<int, CK::kStatSlots>{}, s);
        // per-step flags: fail (syndrome) for each half, OR over the block.  The int16 range flags
        // (ovf, sticky per lane until the half is refilled) are reduced only when a frame ends,
        // below: an overflow taints every frame in flight, and no frame is stored before that check
        // (two ballots per step instead of four: W +0.6 %, R +0.3 %, A within noise; profiles/r2/ab/flags.txt).
        {
            const uint32_t bits = (par >> 15 & 1u) | (par >> 30 & 2u);
            uint32_t wb = 0;
#pragma unroll
            for (int b = 0; b < 2; ++b) wb |= __ballot((bits >> b) & 1u) ? (1u << b) : 0u;
            if constexpr (CK::kStationary)  // the trigger: par's other bits, the halves' posterior hashes changed
                wb |= (__ballot((par & 0x7fffu) != 0u) ? 4u : 0u) | (__ballot((par & 0x7fff0000u) != 0u) ? 8u : 0u);
            if (wb) atomicOr(&misc[6 + s % 3], (int)wb);  // (wave-uniform: the atomic optimizer elects one lane)
        }
#if FPLDPC_WAIT_TRACE
        const unsigned long long wt1 = __builtin_amdgcn_s_memtime();
        wt_step += wt1 - wt0;
        ++wt_steps;
#endif
        __syncthreads();
#if FPLDPC_WAIT_TRACE
        wt_bar += __builtin_amdgcn_s_memtime() - wt1;
#endif
#if FPLDPC_WAIT_TRACE == 3
        const unsigned long long wd0 = __builtin_amdgcn_s_memtime();
#endif
        uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane(misc[6 + s % 3]);
        int finished = 0;
        if (!((flags & (uint32_t)q_live) == (uint32_t)q_live && s < q_until)) {
            if constexpr (CK::kStationary) stat_decide(flags, s);
            // When no frame ends on pc's syndrome but every frame still running has just made its last
            // update (max_iter) into pn, check pn now (one syndrome pass after the barrier) instead of in
            // the next step's gather: a frame then costs max_iter check updates, not max_iter + 1.
            const uint32_t *pf = pc;
            int dadj = 0;
            {
                bool any = false, last = true, ends = false;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (frm(h) < 0) continue;
                    const int d = s - sst(h);
                    const bool fail = flags >> h & 1u;
                    ends = ends || (d == 0 && a.precheck && !fail) || (d >= 1 && a.early_term && !fail) || d >= a.max_iter;
                    if constexpr (CK::kStationary) ends = ends || (sc.stat >> h & 1);
                    any = true;
                    last = last && d + 1 == a.max_iter;
                }
                if (any && last && !ends) {
                    const uint32_t p2 = ck.syndrome(pn, lds_addr(pn));
                    const uint32_t b2 = (p2 >> 15 & 1u) | (p2 >> 30 & 2u);
                    uint32_t w2 = 0;
                    for (int b = 0; b < 2; ++b) w2 |= __ballot((b2 >> b) & 1u) ? (1u << b) : 0u;
                    if (lane == 0 && w2) atomicOr(&misc[12], (int)w2);
                    PK_SYNC();
                    flags = (flags & ~3u) | (uint32_t)__builtin_amdgcn_readfirstlane(misc[12]);
                    pf = pn;
                    dadj = 1;
                }
            }
            int ending = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (frm(h) < 0) continue;
                const int d = s - sst(h) + dadj;
                const bool fail = flags >> h & 1u;
                if ((d == 0 && a.precheck && !fail) || (d >= 1 && a.early_term && !fail) || d >= a.max_iter) ending |= 1 << h;
            }
            if constexpr (CK::kStationary) {  // sexit: the halves that end by the stationary exit and by nothing else
                sc.sexit = sc.stat & ~ending;
                ending |= sc.sexit;
            }
            if (ending) {
                // the deferred int16 range check: a c2v at or above 2^b (a.cmax = 2^b - 1) in either half
                // since that half's refill corrupts both halves' posterior words, so it taints every
                // frame in flight (misc[13] is cleared again by the refill that follows)
                const uint32_t hi_bits = ~(a.cmax * 0x10001u);
                if (__ballot((ovf & hi_bits) != 0u) && lane == 0) atomicOr(&misc[13], 1);
                PK_SYNC();
                if (__builtin_amdgcn_readfirstlane(misc[13])) {
                    taint[0] = taint[0] || frm(0) >= 0;
                    taint[1] = taint[1] || frm(1) >= 0;
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!(ending >> h & 1)) continue;
                // completed updates in pf for this frame; a stationary frame reports the max_iter updates
                // whose result pf (= pc, with pc's syndrome in flags: no final-update pass ran) holds
                int d = s - sst(h) + dadj;
                if constexpr (CK::kStationary)
                    if (sc.sexit >> h & 1) d = a.max_iter;
                const bool fail = flags >> h & 1u;
                const bool pre = d == 0 && a.precheck && !fail;
                finished |= 1 << h;
                if (taint[h]) {
                    if (tid == 0) a.fb_list[atomicAdd(a.fb_count, 1)] = frm(h);
                } else {
                    store(h, pre ? llrc : pf, pre, pre ? 0 : d, pre ? 1 : !fail);
                    if constexpr (CK::kStationary)
                        if ((sc.sexit >> h & 1) && tid == 0) misc[14] += 1;
                }
            }
        }
        cur = (cur + 1) % 3;
        if (finished) {
            refill(finished, s + 1, cur);
            // the refilled half starts from zero c2v state and a fresh range tracker
            const uint32_t keep = (finished & 1 ? 0xffff0000u : 0xffffffffu) & (finished & 2 ? 0x0000ffffu : 0xffffffffu);
            ck.clear(finished);
            ovf &= keep;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (finished >> h & 1) taint[h] = misc[4 + h] != 0;
                frm_r[h] = __builtin_amdgcn_readfirstlane(misc[h]);
                sst_r[h] = __builtin_amdgcn_readfirstlane(misc[2 + h]);
            }
            if constexpr (CK::kSplit) tail = a.split_tail && (frm(0) < 0) != (frm(1) < 0);
            // (the exit's word rebuilt from the old one here, after the refill: the same value carried across
            // the refill made the allocator copy the 47 state registers to a second set and back at every
            // step -- 96 v_mov on the quick path, 3-4 % at points without stationary frames)
            if constexpr (CK::kStationary) sc.vsk = (q_live & 0xc) | (sc.vs(q_live) & ~((finished & 1 ? 3 : 0) | (finished & 2 ? 12 : 0))) << 16;
            set_quick();
            if constexpr (CK::kStationary) q_live = sc.word(q_live, (sc.vsk & 0xc) != 0, sc.vsk >> 16);
        }
#if FPLDPC_WAIT_TRACE == 3
        wt_bar2 += __builtin_amdgcn_s_memtime() - wd0;
#endif
    }
    // The cycle exit (split loop only, DESIGN.md "Cycle exit (round 21)").  The c2v messages are the whole
    // state of the iteration (posterior = LLR + sum c2v, v2c = posterior - c2v), so a frame whose c2v after
    // update u + P equal those after update u repeats from there with period P: update max_iter gives what
    // update u + P + rem gives, rem = (max_iter - u - P) mod P.  The frame's start step is moved back by the
    // whole periods left, and it ends through the max_iter path as if it had run them.
    //   arm      some live check lane's posterior hash did not change (flag bit 6), more than 8 updates
    //            are left, and no stationary verification is pending
    //   snapshot the step after stores the c2v words in the scratch slice (the rows the stationary
    //            verification uses: its trigger drops a held snapshot, so the two are never pending together)
    //   hold     the 8 steps after that compare with the snapshot and store nothing (flag bit 4, as the
    //            stationary compare); then a new snapshot, if still armed
    // Its state rides in q_live too, in the split loop's own reading of the word (the lone frame is in half
    // 0, so half 1's bits are free there; a new scalar alive in this loop, or one more branch on its quick
    // path, cost the packed loop 20 VGPRs and spills):
    //   bit 2      the exits are on for the frame (sc.on)      bit 3      the cycle exit is on
    //   bits 18-19 the coming step's part, where half 1's verification state would be (1: it stores the
    //              snapshot, 2: it compares and keeps it), so sc.vs and stat_check's compare flag cover it
    //   bits 20-23 the steps since the snapshot while it is held
    // The cycle exit's decisions after the barrier of step s, after stat_decide's; d = the frame's completed
    // updates in pc, and the state compared is that of update d + 1.
    [[maybe_unused]] auto cyc_decide = [&](uint32_t flags, int s) {
        if constexpr (CK::kStationary) {
            if (!(q_live & 8) || frm(0) < 0) return;
            const int part = q_live >> 18 & 3, age = q_live >> 20 & 15, d = s - sst(0);
            int nc = 0;
            if (part == 1) {
                nc = 2 << 18;  // this step stored the snapshot
            } else if (part == 2) {
                const int period = age + 1;
                if (!(flags & 0x10u)) {
                    if (period == 1) {
                        // the stationary proof itself: update d + 1 reproduced the c2v of update d
                        sc.stat |= 1;
                    } else if ((flags & 1u) || !a.early_term) {  // (a satisfied syndrome ends the frame by itself)
                        int rem = a.max_iter - (d + 1);
                        const int left = rem;
                        while (rem >= period) rem -= period;
                        if (left > rem) {
                            sst_r[0] -= left - rem;
                            q_until = sst_r[0] + a.max_iter - 1;
                            q_live &= 0xfff3;  // the exits are off for the rest of this frame
                            if (tid == 0) misc[15] += 1;
                            return;
                        }
                    }
                } else if (period < 8) {
                    nc = 2 << 18 | period << 20;
                }
            }
            if (nc == 0 && (flags & 0x40u) && a.max_iter - d > 8) nc = 1 << 18;
            if ((sc.vs(q_live) & 3) || (sc.stat & 1)) nc = 0;  // the stationary exit keeps precedence (and the rows)
            q_live = (q_live & 0x3ffff) | nc;
        }
    };
    // (the split loop's step)
    auto step_body = [&](int s, auto split_c) -> bool {
        constexpr bool SPLIT = decltype(split_c)::value;
        if (frm(0) < 0 && frm(1) < 0) {
            clock_probe(a, 2);
            if (a.wgtrace && tid == 0) {
                unsigned long long *t = a.wgtrace + 8 * (size_t)blockIdx.x;
                t[0] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |
                       (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);  // HW_REG_XCC_ID, HW_REG_HW_ID
                t[1] = trace_t0;
                t[2] = __builtin_amdgcn_s_memrealtime();
                t[3] = (unsigned long long)trace_frames;
#if FPLDPC_PHASE_TRACE
                t[4] = ph_refill;
                t[5] = FPLDPC_PHASE_TRACE == 3 ? ph_rhead : FPLDPC_PHASE_TRACE == 2 ? ph_sloop : ph_pull;
                t[6] = ph_store;
                t[7] = FPLDPC_PHASE_TRACE == 3 ? ph_rload : ph_steps;
#endif
#if FPLDPC_TAIL_TRACE
                t[3] |= (unsigned long long)(unsigned)(tt_frame + 1) << 32;
                t[4] = tt_empty;
                t[5] = tt_split;
                t[6] = tt_two | tt_one << 32;
                t[7] = tt_splits;
#endif
            }
            return false;
        }
        const uint32_t *pc = bufs + cur * n;
        uint32_t *pn = bufs + ((cur + 1) % 3) * n;
        uint32_t *pr = bufs + ((cur + 2) % 3) * n;
        {
            int v0 = tid;  // opaque: keeps the compiler from hoisting 3 x 9 addresses across steps
            asm volatile("" : "+v"(v0));
            if (CK::kN) {
#pragma unroll
                for (int v = v0, j = 0; j < (CK::kN + NT - 1) / NT; ++j, v += NT)
                    if (j < CK::kN / NT || v < CK::kN) pr[v] = llrc[v];
            } else if ((n & 3) == 0) {  // 16-byte chunks, every buffer 16-byte aligned (W +1.3-1.4 %, W @ 2 dB +2.0 %, profiles/r6/ab/w_copy16.txt)
                const int n4 = n >> 2;
                const uint4 *l4 = reinterpret_cast<const uint4 *>(llrc);
                uint4 *p4 = reinterpret_cast<uint4 *>(pr);
                for (int vb = v0; vb < n4; vb += 2 * NT) {
                    const uint4 t0 = l4[vb];
                    uint4 t1 = {};
                    if (vb + NT < n4) t1 = l4[vb + NT];
                    p4[vb] = t0;
                    if (vb + NT < n4) p4[vb + NT] = t1;
                }
            } else {  // 8 loads in flight per thread, then 8 stores
                for (int vb = v0; vb < n; vb += 8 * NT) {
                    uint32_t t[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) t[j] = vb + j * NT < n ? llrc[vb + j * NT] : 0u;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (vb + j * NT < n) pr[vb + j * NT] = t[j];
                }
            }
        }
        // flag word of step s+1: last read at step s-2, and every thread has passed the barrier of
        // step s-1 since; it is next written after this step's barrier
        if (tid == 0) {
#if FPLDPC_PHASE_TRACE
            ++ph_steps;
#endif
#if FPLDPC_TAIL_TRACE
            ++tt_splits;
#endif
            misc[6 + (s + 1) % 3] = 0;
            misc[12] = 0;  // flag word of a final-update syndrome pass (below), read after this step's barrier
        }
        uint32_t par = 0, ovor = 0;
        // (The check step always runs: a frame's last update is checked by the final-update syndrome pass
        // below, not by one more step.)
        if constexpr (SPLIT)
            split_step_of(ck, pc, pn, lds_addr(pc), lds_addr(pn), C2, M2, par, ovor);
        else
            ck.step(a, pc, pn, lds_addr(pc), lds_addr(pn), C2, M2, par, ovor);
        ovf |= ovor;
        if constexpr (CK::kStationary) {  // (nested: the outer condition does not depend on the lambda's parameter)
            // (the stationary verification, or the cycle exit's snapshot / compare)
            if constexpr (SPLIT) stat_check(std::integral_constant<int, CK::kStatSplitSlots>{}, s);
        }
        // per-step flags: fail (syndrome) for each half, OR over the block.  The int16 range flags
        // (ovf, sticky per lane until the half is refilled) are reduced only when a frame ends,
        // below: an overflow taints every frame in flight, and no frame is stored before that check
        // (two ballots per step instead of four: W +0.6 %, R +0.3 %, A within noise; profiles/r2/ab/flags.txt).
        {
            const uint32_t bits = (par >> 15 & 1u) | (par >> 30 & 2u);
            uint32_t wb = 0;
#pragma unroll
            for (int b = 0; b < 2; ++b) wb |= __ballot((bits >> b) & 1u) ? (1u << b) : 0u;
            if constexpr (CK::kStationary) {  // (the trigger, as in the packed loop; the frame is in half 0)
                wb |= __ballot((par & 0x7fffu) != 0u) ? 4u : 0u;
                // the cycle exit's arming bit, while it is on: the hashes of kCycArm live check lanes of one wave
                // did not change.  (One lane is not enough: the posteriors are small numbers, and the 15-bit XOR
                // of a check's 47 stays the same by chance in about one check in a hundred per update, at 2 dB
                // in some check at nearly every step; a cycling frame leaves 11 and more lanes of a wave unchanged.)
                constexpr int kCycArm = 8;
                wb |= __popcll(__ballot(tid < a.m && (par & 0x7fffu) == 0u)) >= kCycArm ? (uint32_t)(q_live & 8) << 3 : 0u;
            }
            if (lane == 0 && wb) atomicOr(&misc[6 + s % 3], (int)wb);
        }
        __syncthreads();
        uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane(misc[6 + s % 3]);
        {  // the packed loop's quick exit (from the control words: q_live / q_until are the packed loop's)
            bool q = true;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (frm(h) >= 0) q = q && (flags >> h & 1u) && s < sst(h) + a.max_iter - 1;
            // (the stationary exit: the frame's posteriors changed, and no verification is pending)
            if constexpr (CK::kStationary)
                if (sc.on(q_live)) q = q && (flags & 0x44u) == 4u && !sc.vs(q_live);
            if (q) {
                cur = (cur + 1) % 3;
                return true;
            }
        }
        // (the stationary exit as in the packed loop; the frame is in half 0, and of the posterior words
        // only that half is the frame's: half 1's `changed` and compare bits are never looked at)
        if constexpr (CK::kStationary) stat_decide(flags, s);
        // (the cycle exit, before the end decisions: a frame it leaves no update to ends in this step)
        if constexpr (CK::kStationary) cyc_decide(flags, s);
        // When no frame ends on pc's syndrome but every frame still running has just made its last
        // update (max_iter) into pn, check pn now (one syndrome pass after the barrier) instead of in
        // the next step's gather: a frame then costs max_iter check updates, not max_iter + 1.
        const uint32_t *pf = pc;
        int dadj = 0;
        {
            bool any = false, last = true, ends = false;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (frm(h) < 0) continue;
                const int d = s - sst(h);
                const bool fail = flags >> h & 1u;
                ends = ends || (d == 0 && a.precheck && !fail) || (d >= 1 && a.early_term && !fail) || d >= a.max_iter;
                if constexpr (CK::kStationary) ends = ends || (sc.stat >> h & 1);
                any = true;
                last = last && d + 1 == a.max_iter;
            }
            if (any && last && !ends) {
                const uint32_t p2 = ck.syndrome(pn, lds_addr(pn));
                const uint32_t b2 = (p2 >> 15 & 1u) | (p2 >> 30 & 2u);
                uint32_t w2 = 0;
                for (int b = 0; b < 2; ++b) w2 |= __ballot((b2 >> b) & 1u) ? (1u << b) : 0u;
                if (lane == 0 && w2) atomicOr(&misc[12], (int)w2);
                __syncthreads();
                flags = (flags & ~3u) | (uint32_t)__builtin_amdgcn_readfirstlane(misc[12]);
                pf = pn;
                dadj = 1;
            }
        }
        int ending = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (frm(h) < 0) continue;
            const int d = s - sst(h) + dadj;
            const bool fail = flags >> h & 1u;
            if ((d == 0 && a.precheck && !fail) || (d >= 1 && a.early_term && !fail) || d >= a.max_iter) ending |= 1 << h;
        }
        if constexpr (CK::kStationary) {
            sc.sexit = sc.stat & ~ending;
            ending |= sc.sexit;
        }
        if (ending) {
            // the deferred int16 range check: a c2v at or above 2^b (a.cmax = 2^b - 1) in either half
            // since that half's refill corrupts both halves' posterior words, so it taints every
            // frame in flight (misc[13] is cleared again by the refill that follows)
            const uint32_t hi_bits = ~(a.cmax * 0x10001u);
            if (__ballot((ovf & hi_bits) != 0u) && lane == 0) atomicOr(&misc[13], 1);
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane(misc[13])) {
                taint[0] = taint[0] || frm(0) >= 0;
                taint[1] = taint[1] || frm(1) >= 0;
            }
        }
        int finished = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (!(ending >> h & 1)) continue;
            int d = s - sst(h) + dadj;  // completed updates in pf for this frame (stationary: as in the packed loop)
            if constexpr (CK::kStationary)
                if (sc.sexit >> h & 1) d = a.max_iter;
            const bool fail = flags >> h & 1u;
            const bool pre = d == 0 && a.precheck && !fail;
            finished |= 1 << h;
            if (taint[h]) {
                if (tid == 0) a.fb_list[atomicAdd(a.fb_count, 1)] = frm(h);
            } else {
                store(h, pre ? llrc : pf, pre, pre ? 0 : d, pre ? 1 : !fail);
                if constexpr (CK::kStationary)
                    if ((sc.sexit >> h & 1) && tid == 0) misc[14] += 1;
            }
        }
        cur = (cur + 1) % 3;
        if (finished) {
            if constexpr (CK::kStationary) q_live &= ~((finished & 1 ? 3 << 16 : 0) | (finished & 2 ? 12 << 16 : 0));
            refill(finished, s + 1, cur);
            // the refilled half starts from zero c2v state and a fresh range tracker.  (In the split
            // form the queue is empty -- a half goes idle only when a pull finds it so -- and this
            // refill finds no frame: the workgroup ends.)
            const uint32_t keep = (finished & 1 ? 0xffff0000u : 0xffffffffu) & (finished & 2 ? 0x0000ffffu : 0xffffffffu);
            ck.clear(finished);
            ovf &= keep;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (finished >> h & 1) taint[h] = misc[4 + h] != 0;
                frm_r[h] = __builtin_amdgcn_readfirstlane(misc[h]);
                sst_r[h] = __builtin_amdgcn_readfirstlane(misc[2 + h]);
            }
        }
        return true;
    };
    if constexpr (CK::kSplit) {
        if (more) {
            // The tail: this frame continues in half 0 of the LDS words with its check split over the
            // lane halves (ArrayChecks::split_step, about 55 % of the packed step's instructions), so
            // the frames the launch waits on at its end run at a shorter step latency.  A frame in half
            // 1 is moved to half 0 first: posterior, next-posterior and LLR words rotated, its control
            // words swapped.
            const int h = frm(0) < 0 ? 1 : 0;
            if (h) {
                for (int v = tid; v < 4 * n; v += NT) bufs[v] = CK::rot16(bufs[v]);
                if (tid == 0) {
                    for (int i : {0, 2, 4, 9}) {
                        const int t = misc[i];
                        misc[i] = misc[i + 1];
                        misc[i + 1] = t;
                    }
                }
                const int f0 = frm_r[0], s0 = sst_r[0];
                const bool t0 = taint[0];
                frm_r[0] = frm_r[1];
                sst_r[0] = sst_r[1];
                taint[0] = taint[1];
                frm_r[1] = f0;
                sst_r[1] = s0;
                taint[1] = t0;
                ovf >>= 16;
            } else {
                ovf &= 0xffffu;
            }
            ck.split_enter(h);
            // (the scratch words are the packed state's: a pending verification starts over from the
            // trigger, which a stationary frame sets again at every step)
            // (and the word in the split loop's reading: bit 2 the exits on, bit 3 the cycle exit on)
            if constexpr (CK::kStationary) q_live = sc.on(q_live) ? ((a.split_tail & 2) ? 12 : 4) : 0;
#if FPLDPC_TAIL_TRACE
            if (tid == 0) tt_split = __builtin_amdgcn_s_memrealtime();
            tt_frame = frm_r[0];
#endif
            __syncthreads();
            for (;; ++s)
                if (!step_body(s, std::true_type{})) break;
        }
    }
    if constexpr (CK::kStationary) {
        // the call's stationary exits, in the counter block's list-1 size: a chain of two kernels has no
        // second fallback list, and the chain's last kernel keeps that word for the host and zeroes it
        // (chain_reset).  A returning atomic whose value is used, as chain_exit asks of counter accesses.
        if (a.c2v_scratch && tid == 0 && misc[14]) {
            const int was = atomicAdd(&a.counters[kCountFb1], misc[14]);
            asm volatile("" ::"v"(was));
        }
        // the call's cycle exits, in a counter word of their own that this kernel keeps by itself (the
        // chain's last kernel knows nothing of it): every workgroup counts itself out in the word's low
        // kCycOutBits bits and adds its exits above them; the last one out leaves the sum for the host
        // and zeroes the word for the next call (plain stores, seen at the kernel boundary as chain_reset's).
        if (a.c2v_scratch && (a.split_tail & 2) && tid == 0) {
            const int was = atomicAdd(&a.counters[kCountCyc], (misc[15] << kCycOutBits) | 1);
            if ((was & ((1 << kCycOutBits) - 1)) == (int)gridDim.x - 1) {
                a.counters[kCountCycLast] = (was >> kCycOutBits) + misc[15];
                a.counters[kCountCyc] = 0;
            }
        }
    }
    if (a.totals && tid == 0) {  // this workgroup's frames (each counter < 2^31 per workgroup)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (misc[kTotW + c]) atomicAdd(&a.totals[c], (unsigned long long)(unsigned)misc[kTotW + c]);
    }
    chain_exit(a);
}

}  // namespace
}  // namespace fpldpc
