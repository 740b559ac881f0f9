// fpldpc_flood_packed.hpp -- the arithmetic of the packed (two frames per lane) kernels: the 16-bit
// pair types, box-plus on both halves (bp_mag2), biased pairs and their sign/magnitude form, the LDS
// slot addressing and the c2v emission.  Included by the check policies (fpldpc_flood_checks_array.hpp,
// fpldpc_flood_checks_table.hpp), by fpldpc_flood_pk.hpp and by fpldpc_flood_lds16.hpp (sub2x), so by
// all three flooding translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace fpldpc {
namespace {

// Packed kernel (flood_pk): two frames per lane, one in each 16-bit half (v_pk_* ops), so every VALU op,
// LDS access and address computation serves two frames.  Exact while every value fits int16:
// with |LLR| <= kLlrMax and every c2v magnitude <= a.cmax = (32767 - kLlrMax) / (dv_max + 1),
// |post| and |v2c| stay below 32768 and the u16 magnitude chain (a + b <= 65534) never wraps.
// A frame that leaves that range (or overlaps in time with a partner that does) is not written:
// it is appended to a.fb_list and decoded again by the variant's fallback kernel (kVariants) in a
// second pass, so outputs are bit-exact for every input.
//
// Posteriors live in LDS as *biased* pairs V = (lo + 0x7fff) | (hi + 0x7fff) << 16: c2v
// messages are added in carry form (lo + 65536*hi, a plain int32), so the next posterior is still
// accumulated with one ds_add_u32 per edge, and since LLR + bias + sum(c2v) is exact modulo 2^32
// the final word has both biased halves in place while |post| <= 32767, whatever the order of the
// adds.  Bits 15 / 31 are then (post >= 1) = NOT hard (:305-308), and v2c = V - c2v is again a
// biased pair (one subtraction).  The two halves run independent frames: when one finishes (own
// iteration count, early termination, pre-check) its outputs are written and the half is refilled
// with the next frame at the next step while the other half carries on.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
constexpr int kLlrMax = 8000;

__device__ __forceinline__ u16x2 U2(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ i16x2 I2(uint32_t x) { return __builtin_bit_cast(i16x2, x); }
__device__ __forceinline__ uint32_t W(u16x2 x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t W(i16x2 x) { return __builtin_bit_cast(uint32_t, x); }

// low half of a carry-form word lo + 65536*hi (the c2v state): the high half is (v - lo) >> 16
__device__ __forceinline__ int carry_lo(uint32_t v) { return (int)(short)(v & 0xffffu); }

// bp_mag on both halves: min(a,b) + min(C, ((|a-b| & M) >> 2)) - min(C, ((a+b) & M) >> 2).
// The halves are magnitudes below 2^15, so a + b and max - min never cross into the other half, a
// 32-bit right shift only pollutes bits 14-15 of the low half (cleared by M2, at most 14 bits per
// half), and mn + q2 - q1 >= 0 per half: full-rate 32-bit add/sub/shift/and give exact per-half
// results, and only the three min/max steps need the (half-rate) packed instructions.
// 2*x written as x + x: hipcc turns it into v_lshlrev_b32, which issues at half the rate of
// v_add_u32 on gfx950 (profiles/r1/ubench_valu_rate.txt)
__device__ __forceinline__ uint32_t sub2x(uint32_t a, uint32_t x) {  // a - 2x
    uint32_t r;
    asm("v_sub_u32 %0, %1, %2\n\tv_sub_u32 %0, %0, %2" : "=&v"(r) : "v"(a), "v"(x));
    return r;
}

// (The packed kernels hold C2 / M2 in VGPRs, see flood_pk: as SGPR operands, hipcc's choice for
// uniform values, the 270 v_and_b32 / v_pk_min_u16 per check-step that read them cost A 0.5-1.9 %
// and W 0.7 % (profiles/r2/ab/bp_form.txt); C = 10 / mask 0xff as immediates measured 4.6 % slower.)
// FORM 0 leaves the order to hipcc; FORM 1 is one asm block (no pk_min result read by the next
// instruction).  Measured per kernel (profiles/r5/ab/post_ra.txt): the asm block is +2.7 % on R and
// +1.3 % on W but -4 % on A, whatever its order (two other orders of the block were measured the
// same), so each check policy picks its own (kBp).  (Also measured and not kept: two independent
// box-pluses interleaved in one block with their six v_pk_min_u16 four instructions apart -- W and R
// unchanged, R's kernel spilling when its whole checks used it; W's output-range ORs kept out of
// v_or3_b32 -- W -2.7 %.)
constexpr int kBpArray1 = 0;  // A: compiler order
constexpr int kBpMany = 1;    // R (two checks per lane, split units) and W: the asm block
template <int FORM>
__device__ __forceinline__ uint32_t bp_mag2(uint32_t a, uint32_t b, u16x2 C2, uint32_t M2) {
    if constexpr (FORM == 0) {
        const uint32_t mn = W(__builtin_elementwise_min(U2(a), U2(b)));
        const uint32_t s = a + b;          // per half a + b < 2^16
        const uint32_t d = sub2x(s, mn);   // per half max - min = a + b - 2 min >= 0
        const uint32_t q1 = W(__builtin_elementwise_min(U2((s >> 2) & M2), C2));
        const uint32_t q2 = W(__builtin_elementwise_min(U2((d >> 2) & M2), C2));
        return mn + q2 - q1;
    } else {
        uint32_t mn, s, t;
        static_assert(FORM == 1, "bp_mag2: FORM 0 (compiler order) or 1 (one asm block)");
        asm("v_pk_min_u16 %0, %3, %4\n\tv_add_u32 %1, %3, %4\n\tv_lshrrev_b32 %2, 2, %1\n\t"
            "v_sub_u32 %1, %1, %0\n\tv_sub_u32 %1, %1, %0\n\tv_and_b32 %2, %2, %6\n\t"
            "v_lshrrev_b32 %1, 2, %1\n\tv_pk_min_u16 %2, %2, %5\n\tv_and_b32 %1, %1, %6\n\t"
            "v_pk_min_u16 %1, %1, %5\n\tv_sub_u32 %0, %0, %2\n\tv_add_u32 %0, %0, %1"
            : "=&v"(mn), "=&v"(s), "=&v"(t) : "v"(a), "v"(b), "v"(W(C2)), "v"(M2));
        return mn;
    }
}

// Biased pairs (posteriors, LLRs, v2c): half h holds x + 0x7fff, in [0, 0xfffe] for |x| <= 32767.
__device__ __forceinline__ int bias_half(uint32_t v, int h) { return (int)((v >> (16 * h)) & 0xffffu) - 0x7fff; }
__device__ __forceinline__ uint32_t bias_set(uint32_t v, int h, int x) {
    const uint32_t u = (uint32_t)(x + 0x7fff) & 0xffffu;
    return h ? (v & 0xffffu) | (u << 16) : (v & 0xffff0000u) | u;
}
// biased v2c pair u -> sign-magnitude halves (|x| in bits 0-14, x <= 0 in bit 15; the flag of a
// zero is irrelevant: a zero magnitude absorbs every chain through it, and output k's sign never
// uses flag k).  Per half: t = 0x8000 iff x >= 1, c = its bit-0 copy, w = t - c = 0x7fff iff
// x >= 1; ~(u ^ w) is then x - 1 (x >= 1) or 0x8000 | -x (x <= 0), and + c gives |x| without a
// carry out of the half, so the whole word is c - (u ^ w) - 1 in plain 32-bit arithmetic.  Six
// full-rate VOP2 ops: v_xnor_b32, though VOP2, issues at the slow rate in a mix
// (profiles/r1/ubench/mix_rate.txt), as hipcc's v_xad_u32 fusion would.
__device__ __forceinline__ uint32_t sign_mag_b(uint32_t u, uint32_t sgn = 0x80008000u) {
    const uint32_t t = u & sgn, c = t >> 15;
    uint32_t x = u ^ (t - c), r;
    asm("v_sub_u32 %0, %1, %2\n\tv_add_u32 %0, -1, %0" : "=&v"(r) : "v"(c), "v"(x));
    return r;
}
// sign_mag_b on 8 values with the final c - x - 1 as v_subb_co_u32 (c - x - VCC): VCC is set to all
// ones once and stays so, because c <= x in every lane and half combination (c = 1 in a half only
// when that half's x is >= 0x8000; c = 0 borrows from 0 - x - 1), so every subtraction borrows out
// again: 5 full-rate ops per value instead of 6.
template <int G>
__device__ __forceinline__ void sign_mag_b_x(uint32_t (&u)[G]) {
    static_assert(G == 8, "batch of 8");
    uint32_t t[8], c[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        t[g] = u[g] & 0x80008000u;
        c[g] = t[g] >> 15;
        u[g] ^= t[g] - c[g];
    }
    asm("s_mov_b64 vcc, -1\n\t"
        "v_subb_co_u32_e32 %0, vcc, %8, %0, vcc\n\t"
        "v_subb_co_u32_e32 %1, vcc, %9, %1, vcc\n\t"
        "v_subb_co_u32_e32 %2, vcc, %10, %2, vcc\n\t"
        "v_subb_co_u32_e32 %3, vcc, %11, %3, vcc\n\t"
        "v_subb_co_u32_e32 %4, vcc, %12, %4, vcc\n\t"
        "v_subb_co_u32_e32 %5, vcc, %13, %5, vcc\n\t"
        "v_subb_co_u32_e32 %6, vcc, %14, %6, vcc\n\t"
        "v_subb_co_u32_e32 %7, vcc, %15, %7, vcc"
        : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6]), "+v"(u[7])
        : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]), "v"(c[7])
        : "vcc");
}
// The same on G = 4, 6 or 7 values (the pipelined gather, the table policy), one asm block (split
// into blocks of two it measured 1 % slower: the block boundaries constrain the scheduler)
template <int G>
__device__ __forceinline__ void sign_mag_b_xg(uint32_t (&u)[G]) {
    static_assert(G == 4 || G == 6 || G == 7, "batch of 4, 6 or 7");
    uint32_t t[G], c[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        t[g] = u[g] & 0x80008000u;
        c[g] = t[g] >> 15;
        u[g] ^= t[g] - c[g];
    }
    if constexpr (G == 4)
        asm("s_mov_b64 vcc, -1\n\t"
            "v_subb_co_u32_e32 %0, vcc, %4, %0, vcc\n\t"
            "v_subb_co_u32_e32 %1, vcc, %5, %1, vcc\n\t"
            "v_subb_co_u32_e32 %2, vcc, %6, %2, vcc\n\t"
            "v_subb_co_u32_e32 %3, vcc, %7, %3, vcc"
            : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3])
            : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3])
            : "vcc");
    else if constexpr (G == 7)
        asm("s_mov_b64 vcc, -1\n\t"
            "v_subb_co_u32_e32 %0, vcc, %7, %0, vcc\n\t"
            "v_subb_co_u32_e32 %1, vcc, %8, %1, vcc\n\t"
            "v_subb_co_u32_e32 %2, vcc, %9, %2, vcc\n\t"
            "v_subb_co_u32_e32 %3, vcc, %10, %3, vcc\n\t"
            "v_subb_co_u32_e32 %4, vcc, %11, %4, vcc\n\t"
            "v_subb_co_u32_e32 %5, vcc, %12, %5, vcc\n\t"
            "v_subb_co_u32_e32 %6, vcc, %13, %6, vcc"
            : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5]), "+v"(u[6])
            : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6])
            : "vcc");
    else
        asm("s_mov_b64 vcc, -1\n\t"
            "v_subb_co_u32_e32 %0, vcc, %6, %0, vcc\n\t"
            "v_subb_co_u32_e32 %1, vcc, %7, %1, vcc\n\t"
            "v_subb_co_u32_e32 %2, vcc, %8, %2, vcc\n\t"
            "v_subb_co_u32_e32 %3, vcc, %9, %3, vcc\n\t"
            "v_subb_co_u32_e32 %4, vcc, %10, %4, vcc\n\t"
            "v_subb_co_u32_e32 %5, vcc, %11, %5, vcc"
            : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]), "+v"(u[3]), "+v"(u[4]), "+v"(u[5])
            : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5])
            : "vcc");
}
// LDS addressing of the packed kernels: buffers are addressed by their 32-bit LDS byte address
// (< 64 KiB within a workgroup's allocation); a slot's 16-bit byte offset, kept two per VGPR,
// plus the buffer's (wave-uniform) address costs one v_add_u16 for the low half (the result's
// high half is zeroed on gfx9) or a shift and an add for the high half, all full-rate VOP2.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) int lds_i32;
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(size_t)(const __attribute__((address_space(3))) void *)p;
}
// (base in a VGPR: a 16-bit VOP2 op with an SGPR operand issues at the slow rate)
// LDS byte address of a slot: base + the low (hi = 0) or high 16-bit offset of a packed pair.
// SDWA: one 32-bit add with a word select for either half, any LDS address -- the stored-offset
// policy (A) and the split checks (A +1.15 %; R's LDS-table policy -1.2 %, profiles/r3/ab/sdwa.txt).
// Otherwise a 16-bit add for the low half (LDS byte addresses below 64 KiB, as in flood_pk's
// one-frame-pair layouts) and shift + add for the high one.
template <bool SDWA>
__device__ __forceinline__ uint32_t lds_at(uint32_t offs2, int hi, uint32_t base) {
    uint32_t r;
    if constexpr (SDWA) {
    if (hi)
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
            : "=v"(r) : "v"(base), "v"(offs2));
    else
        asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0"
            : "=v"(r) : "v"(base), "v"(offs2));
    } else {
    if (hi)
        asm("v_lshrrev_b32 %0, 16, %1\n\tv_add_u32 %0, %2, %0" : "=&v"(r) : "v"(offs2), "v"(base));
    else
        asm("v_add_u16 %0, %1, %2" : "=v"(r) : "v"(base), "v"(offs2));
    }
    return r;
}
__device__ __forceinline__ void lds_add_at(uint32_t addr, int v) {
    __hip_atomic_fetch_add(reinterpret_cast<lds_i32 *>((size_t)addr), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Output k of a check: magnitude o, sign = parity of the other inputs' flags = (S ^ flag_k) in bits
// 15 / 31; st (the v2c in sign-magnitude) is overwritten with the carry-form c2v (o ^ neg) - neg.
// TRACK = false: the magnitude is not OR-ed into ovor (the caller bounds every output of the check
// from two chain values instead, ArrayChecks::kChainGuard).
template <bool ASM_OR = false, bool TRACK = true>
__device__ __forceinline__ void emit_c2v(uint32_t &st, uint32_t o, uint32_t S, uint32_t &ovor) {
    if (!TRACK)
        ;
    else if (ASM_OR)
        asm("v_or_b32 %0, %0, %1" : "+v"(ovor) : "v"(o));  // not fused into v_or3_b32 (VOP3)
    else
        ovor |= o;
    const uint32_t neg = W((i16x2)(I2(S ^ st) >> (i16x2)15));
    // per half neg ? -o : o, as one 32-bit word in carry form: (o ^ m) - m with m = 0xffff in a
    // negative half is (+-hi)*65536 + (+-lo) exactly (the low half's borrow is the carry form's)
    asm("v_xor_b32 %0, %1, %2\n\tv_sub_u32 %0, %0, %2" : "=&v"(st) : "v"(o), "v"(neg));
}

}  // namespace
}  // namespace fpldpc
