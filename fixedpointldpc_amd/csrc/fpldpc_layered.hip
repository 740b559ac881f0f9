// fpldpc_layered.hip -- gfx950 (CDNA4) layered (row-serial) schedule of the fixed-point decoder.
//
// No reference counterpart: tyc85/FixedPointLDPC decodes by flooding only.  The arithmetic is the
// reference's -- the box-plus FP_Decoder::sxor (ArrayLDPC_Decoder.cpp:677-694) and the serial
// forward/backward fold of a check (:66-118) -- under the schedule fixed-point LDPC hardware uses
// (DESIGN.md "Layered schedule"): per frame post[v] = LLR[v] and c2v[c][k] = 0; then, for every
// iteration and for the checks c = 0 .. m-1 in code order, one after another,
//     t[k] = post[v_k] - c2v[c][k];  new = fold(t);  c2v[c][k] = new[k];  post[v_k] = t[k] + new[k]
// and after the last check hard[v] = post[v] > 0 ? 0 : 1 and the syndrome over clist.  Nothing is
// saturated: results are defined while every intermediate fits int32 (the reference's arithmetic has
// the same limit; unsaturated posteriors roughly double per layer once a frame is converging).
//
// Layers are parallelism, not semantics: checks [l*L, (l+1)*L) share no variable (validated at
// creation, fpldpc_code_layering), so updating them at once gives what the serial order gives.
//
// Kernel (layered_generic): persistent grid, one workgroup per frame at a time, frames pulled from a
// device work counter that the last workgroup out resets.  Posteriors are int32 in LDS.  Lane j takes
// check l*L + j of the current layer (looping when L exceeds the workgroup); one __syncthreads()
// separates layers.  A check's c2v entries are only ever touched by the lane that owns the check, so
// the c2v state needs no synchronisation of its own: it lives in LDS (slot-major [dc_max][m], lanes
// on consecutive words) when it fits the CU's 160 KiB beside the posteriors,
// else in a per-workgroup global scratch; the index table joins it in LDS where that costs no resident
// workgroup, and is read from global memory otherwise.  Forward array codes compute v = k*p + (j + i*k) mod p
// instead of reading a table.  Hard decision, syndrome and error counts run once per iteration.
//
// Saturated form (fpldpc_layered_create_sat, include/fpldpc.h): the same kernel with
//     post[v] = clamp(LLR[v], S_p);  t[k] = clamp(post[v_k] - c2v[c][k], S_m);  post[v_k] = clamp(t[k] + new[k], S_p)
// which bounds every c2v by S_m + C and every posterior by S_p, for every input.  With post_bits <= 16
// the on-chip state (posteriors and c2v) is int16 -- half the LDS per frame, and R's c2v fits LDS --
// with the arithmetic in int32 registers; lanes of a layer write distinct posteriors with native
// 16-bit LDS stores, so two lanes on the halves of one word never read-modify-write it.  With
// post_bits 17..24 the state stays int32.
#include <map>
#include <mutex>
#include <utility>

#include "fpldpc_layered_host.hpp"

namespace fpldpc {
namespace {

// State of a kernel instantiation (MODE): the type of the posteriors and c2v; the clamps run in the two
// saturated modes.
template <int MODE> struct LayState { using type = int32_t; };
template <> struct LayState<kLaySat16> { using type = int16_t; };

constexpr size_t lay_state_bytes(int mode) { return mode == kLaySat16 ? sizeof(int16_t) : sizeof(int32_t); }
// 32-bit words that n posteriors take in front of the control words
__host__ __device__ constexpr size_t lay_post_words(int mode, int n) { return ((size_t)n * lay_state_bytes(mode) + 3) / 4; }

// LDS: post [n] ST (up to a whole word) | misc [kLayMisc] | (LDS_STATE) c2v [dc_max][m] ST
//      | (table_lds) vidx [dc_max][m] uint16 | (!EXACT) cdeg [m] uint8;  ST = int16 in MODE kLaySat16, else int32
// EXACT: every check has degree DC -- the slot loops are straight-line code (A and R: DC = 47, a
// quarter of the instructions of the predicated form); otherwise DC is the next of 8 / 16 / 32 / 48 /
// 64, the degrees are staged in LDS once per workgroup and the slots are predicated per lane.
// MODE: kLayUnsat (nothing saturated, int32 state), kLaySat32 / kLaySat16 (the clamps at a.sat_post / a.sat_msg).
template <int DC, bool LDS_STATE, bool EXACT, int MODE>
__global__ void __launch_bounds__(kLayMaxNT) layered_generic(LayeredArgs a) {
    using ST = typename LayState<MODE>::type;
    constexpr bool SAT = MODE != kLayUnsat;
    extern __shared__ __attribute__((aligned(16))) int lay_smem[];
    const int n = a.n, m = a.m, p = a.array_p;
    const int tid = threadIdx.x, NT = blockDim.x;
    ST *const post = reinterpret_cast<ST *>(lay_smem);
    int *const misc = lay_smem + lay_post_words(MODE, n);
    ST *const c2v = LDS_STATE ? reinterpret_cast<ST *>(misc + kLayMisc)
                              : static_cast<ST *>(a.c2v_scratch) + (size_t)blockIdx.x * a.dc_max * m;
    const uint16_t *vidx = a.vidx;  // null: computed addressing (forward array code)
    if constexpr (LDS_STATE) {
        if (a.table_lds) {
            uint16_t *const lv = reinterpret_cast<uint16_t *>(c2v + a.dc_max * m);
            for (int i = tid; i < a.dc_max * m; i += NT) lv[i] = a.vidx[i];
            vidx = lv;
        }
    }
    const uint8_t *cdeg = nullptr;
    if constexpr (!EXACT) {
        const size_t edges = (size_t)a.dc_max * m;
        uint8_t *const ld = reinterpret_cast<uint8_t *>(misc + kLayMisc) +
                            (LDS_STATE ? edges * sizeof(ST) + (a.table_lds ? edges * sizeof(uint16_t) : 0) : 0);
        for (int i = tid; i < m; i += NT) ld[i] = a.cdeg[i];
        cdeg = ld;
    }

    for (;;) {
        const int cw = lay_next_frame(a, misc);
        if (cw < 0) break;
        for (int v = tid; v < n; v += NT) {
            int x = lay_load_llr(a, (size_t)cw * n + v);
            if constexpr (SAT) x = lay_clamp(x, a.sat_post);  // (sign and zero are kept: S_p >= 1)
            post[v] = (ST)x;
        }
        __syncthreads();
        // decode_fixpoint's channel pre-check (ArrayLDPC_Decoder.cpp:443-450): 0 iterations, the
        // channel decision, posteriors left untouched
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
                    int ci = 0, col = 0;
                    if (!vidx) {
                        ci = c / p;
                        col = c - ci * p;
                    }
                    int mv[DC], vi[DC];
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        vi[k] = 0;
                        mv[k] = 0;
                        if (k < deg) {
                            vi[k] = vidx ? (int)vidx[(size_t)k * m + c] : k * p + col;
                            col += ci;
                            if (col >= p) col -= p;
                            const int old = it > 1 ? (int)c2v[(size_t)k * m + c] : 0;  // c2v = 0 before the first update
                            mv[k] = (int)post[vi[k]] - old;
                            if constexpr (SAT) mv[k] = lay_clamp(mv[k], a.sat_msg);
                        }
                    }
                    // forward / backward fold (ArrayLDPC_Decoder.cpp:83-116), the reference's order
                    int B[DC];
                    B[DC - 1] = mv[DC - 1];
#pragma unroll
                    for (int k = DC - 2; k >= 1; --k)
                        B[k] = k < deg - 1 ? lay_boxplus(B[k + 1], mv[k], a.C, a.mask) : mv[k];
                    int F = mv[0];
#pragma unroll
                    for (int k = 0; k < DC; ++k) {
                        if (k >= deg) continue;
                        const int bn = B[k + 1 < DC ? k + 1 : k];  // (unused in the last slot)
                        const int o = k == 0 ? bn : k == deg - 1 ? F : lay_boxplus(F, bn, a.C, a.mask);
                        if (k > 0) F = lay_boxplus(F, mv[k], a.C, a.mask);
                        c2v[(size_t)k * m + c] = (ST)o;  // |o| <= S_m + C: inside int16 where the state is
                        int q = mv[k] + o;
                        if constexpr (SAT) q = lay_clamp(q, a.sat_post);
                        post[vi[k]] = (ST)q;
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

using LayeredFn = void (*)(LayeredArgs);

}  // namespace

// hipFuncAttributeMaxDynamicSharedMemorySize is per kernel function and device, not per decoder: only
// ever raise it, so that a later decoder with a smaller code does not take away what an earlier one
// launches with.  Called with the decoder's device current.
hipError_t raise_dynamic_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> set;
    int dev = 0;
    hipError_t d = hipGetDevice(&dev);
    if (d != hipSuccess) return d;
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = set[{dev, fn}];
    if (bytes <= cur) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cur = bytes;
    return e;
}

namespace {

template <int MODE>
LayeredFn layered_fn_of(int dc, bool lds_state, bool exact) {
    return lay_for_dc(dc, exact, [&](auto d, auto e) -> LayeredFn {
        constexpr int DC = decltype(d)::value;
        constexpr bool EXACT = decltype(e)::value;
        return lds_state ? layered_generic<DC, true, EXACT, MODE> : layered_generic<DC, false, EXACT, MODE>;
    });
}

LayeredFn layered_fn(int dc, bool lds_state, bool exact, int mode) {
    switch (mode) {
        case kLayUnsat: return layered_fn_of<kLayUnsat>(dc, lds_state, exact);
        case kLaySat32: return layered_fn_of<kLaySat32>(dc, lds_state, exact);
        case kLaySat16: return layered_fn_of<kLaySat16>(dc, lds_state, exact);
    }
    return nullptr;
}

}  // namespace

// Envelope: check degrees 2..64; any valid layer size; the posteriors (4 B each, 2 B with int16 state),
// the control words and one byte per check (unless the kernel's DC is every check's degree) within the
// CU's 160 KiB of LDS: n <= 40956 with int32 state; with int16 state every code object's n (<= 65535:
// 128 KiB of posteriors) as long as its degree table fits beside them.
int layered_choose(const fpldpc_code &code, int L, int device, int mode, LayeredChoice *out) {
    LayeredChoice lc;
    if (int st = lay_choice_of_code(code, mode, "layered", &lc)) return st;
    const size_t state = lay_state_bytes(mode);
    if (mode != kLaySat16 && (size_t)(code.n + kLayMisc) * sizeof(int) > kLdsMax)
        return fail(FPLDPC_ERR_UNSUPPORTED, "layered decoder: code length above 40956 (int32 posteriors in 160 KiB of LDS)");
    // posteriors and control words, plus one byte per check for the degree table
    const size_t base = (lay_post_words(mode, code.n) + kLayMisc) * sizeof(int) + (lc.exact ? 0 : (size_t)code.m);
    if (base > kLdsMax)
        return fail(FPLDPC_ERR_UNSUPPORTED, "layered decoder: posteriors and check degrees do not fit 160 KiB of LDS");
    const size_t edges = (size_t)code.dc_max * code.m;
    // The index table joins c2v in LDS only where that costs no resident workgroup: the kernel is
    // bound by latency at one or two waves per SIMD, and the table's reads (consecutive lanes,
    // consecutive entries, addresses known ahead) are the ones global memory serves well.  W: 2
    // workgroups per CU with the table in LDS (55 KB each), 4 without (40 KB): 17.0 -> 9.2 ms per 8192
    // frames at 30 iterations (profiles/r7/layered/).
    // Diagnostics, read at creation (A/B runs, and tests of those paths on small codes):
    // FPLDPC_LAYERED_C2V=global keeps c2v and the index table in global memory even where they fit
    // LDS, =lds keeps c2v in LDS wherever it fits; FPLDPC_LAYERED_TABLE=global / lds places the index
    // table regardless of the rule above.
    const char *force = getenv("FPLDPC_LAYERED_C2V");
    const bool force_global = force && !strcmp(force, "global"), force_lds = force && !strcmp(force, "lds");
    const size_t c2v_bytes = edges * state, tab_bytes = lc.computed ? 0 : edges * sizeof(uint16_t);
    lc.threads = std::min(kLayMaxNT, (L + 63) / 64 * 64);
    lc.lds_state = base + c2v_bytes <= kLdsMax && !force_global;
    LayResidency<LayeredFn> resident{layered_fn(lc.dc, lc.lds_state, lc.exact, mode), lc.threads};
    // Saturated decoders: a c2v that fits LDS but leaves one workgroup per CU resident (R with int16
    // state: 110 KB) goes to the global scratch with its 4 workgroups per CU instead -- the kernel runs
    // at the latency of its dependent chain, and one wave per CU hides none of it (measured
    // on R).  The unsaturated decoder keeps its rule: LDS wherever c2v fits.
    if (mode != kLayUnsat && lc.lds_state && !force_lds) {
        const int with_lds = resident(base + c2v_bytes);
        if (resident.e != hipSuccess) return fail_hip(resident.e, "layered kernel occupancy");
        if (with_lds < 2) {
            lc.lds_state = false;
            resident.fn = layered_fn(lc.dc, false, lc.exact, mode);
        }
    }
    lc.table_lds = lc.lds_state && lay_table_in_lds("FPLDPC_LAYERED_TABLE", base + c2v_bytes, tab_bytes, resident);
    lc.lds_bytes = base + (lc.lds_state ? c2v_bytes + (lc.table_lds ? tab_bytes : 0) : 0);
    int per_cu = resident(lc.lds_bytes);
    // global c2v: at most 4 workgroups per CU, so that the scratch (R: 212 KB per workgroup, 106 KB with
    // int16 state) stays within the L2 / Infinity Cache
    if (!lc.lds_state) per_cu = std::min(per_cu, 4);
    if (int st = lay_grid(per_cu, resident.e, device, "layered", &lc.grid)) return st;
    lc.scratch_bytes = lc.lds_state ? 0 : (size_t)lc.grid * edges * state;
    snprintf(lc.name, sizeof lc.name, "%s<DC=%d,c2v=%s,addr=%s,deg=%s>", mode == kLayUnsat ? "layered_generic" : "layered_sat",
             lc.dc, lc.lds_state ? "lds" : "global", lay_addr_name(lc), lc.exact ? "exact" : "table");
    *out = lc;
    return FPLDPC_OK;
}

int layered_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream) {
    return lay_launch(layered_fn(lc.dc, lc.lds_state, lc.exact, lc.mode), lc, args, args, stream, "layered");
}

}  // namespace fpldpc
