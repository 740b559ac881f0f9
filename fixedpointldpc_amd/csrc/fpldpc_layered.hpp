// fpldpc_layered.hpp -- the layered (row-serial) decoder: declarations shared by fpldpc_code.cpp
// (layer validation), fpldpc_layered.cpp (the fpldpc_layered_* and fpldpc_minsum_* C ABI), fpldpc_layered.hip,
// fpldpc_layered_minsum.hip, fpldpc_minsum.hip, fpldpc_minsum_global.hip, fpldpc_minsum_wide.hip and fpldpc_flood_sat.hip (kernels; through
// fpldpc_layered_device.hpp, beside which fpldpc_layered_host.hpp holds their shared choice and launch steps and
// fpldpc_minsum_device.hpp the min-sum rule).
//
// The layered decoder is an object of its own, not a mode of fpldpc_decoder: its state differs (the
// c2v of every check persists across layers).  What every decoder object has is DecoderCore
// (fpldpc_internal.hpp), which this object is built on as fpldpc_decoder is; the host plumbing around it
// (creation checks, reference bits, the checks of a decode call, the staged host decode) is fpldpc_host.hpp's.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fpldpc_host.hpp"

namespace fpldpc {

// Resolves layer_checks (0 = auto: the array code's p, else qc_z when it gives valid layers, else 1)
// and validates it: L divides m and no variable occurs twice among checks [l*L, (l+1)*L).
int code_layering(const fpldpc_code &code, int layer_checks, int *L, int *layers);

// State of a layered decoder: nothing saturated (fpldpc_layered_create: int32 posteriors and c2v), or
// the clamps of fpldpc_layered_create_sat with int32 state (post_bits 17..24) or int16 state (<= 16), or
// fpldpc_layered_create_minsum (int16 posteriors, 16 bytes of state per check: fpldpc_layered_minsum.hip).
// kFloodMinsum is not a layered decoder: the flooding min-sum decoder (fpldpc_minsum_t, fpldpc_minsum.hip)
// shares this object's host plumbing (L = m, layers = 1, no meaning), and so does kFloodSat, the saturated
// flooding decoder with the sxor fold (fpldpc_flood_create_sat, fpldpc_flood_sat.hip: int16 c2v per edge).
enum { kLayUnsat = 0, kLaySat32 = 1, kLaySat16 = 2, kLayMinsum = 3, kFloodMinsum = 4, kFloodSat = 5 };

// Kernel choice of a layered decoder, made once at creation.
struct LayeredChoice {
    int mode = kLayUnsat;
    int dc = 0;              // kernel DC: 8 / 16 / 32 / 48 / 64 >= dc_max, or the exact degree (47); wide: 32 * sign words
    bool lds_state = false;  // c2v / check state (and the index table) in LDS; else per-workgroup global scratch
    bool computed = false;   // forward array code: v = k*p + (j + i*k) mod p, no index table
    bool table_lds = false;  // the index table is staged in LDS (with lds_state, table codes)
    bool exact = false;      // every check has degree dc: straight-line slot loops, no degree table
    int threads = 64;
    int grid = 0;            // resident workgroups (persistent)
    size_t lds_bytes = 0;
    size_t scratch_bytes = 0; // global c2v: grid * dc_max * m entries of the state type; min-sum: grid * slice
    bool wide = false;        // min-sum: the wide form (fpldpc_minsum_wide.hip: run-time slot loops, degrees to 255)
    int state_bytes = 16;     // min-sum: bytes of check state per check (wide: 8 + 4 * sign words)
    char name[96] = "";
};

// Counter block of a layered decoder (int32): [0] work counter, [1] workgroups out of the kernel.
// Zeroed at creation; the last workgroup out resets it, so a decode call issues kernels only.
constexpr int kLayeredCounterInts = 2;

struct LayeredArgs {
    const void *llr = nullptr;
    int llr_i16 = 0;
    int n = 0, m = 0, dc_max = 0, L = 0, layers = 0, array_p = 0, table_lds = 0;
    int batch = 0, max_iter = 30, C = 10, mask = 0xff, early_term = 1, precheck = 0;
    const uint16_t *vidx = nullptr;  // [dc_max][m] var of slot k of check c (code order); null when computed
    const uint8_t *cdeg = nullptr;   // [m]
    uint32_t *hard = nullptr;
    int hard_words = 0;
    int sat_post = 0;                // S_p of a saturated decoder (this and sat_msg sit in what was padding:
                                     // the unsaturated kernels keep their argument layout)
    int32_t *iters = nullptr;
    uint8_t *syn_ok = nullptr;
    int32_t *post = nullptr;
    int32_t *bit_errors = nullptr;
    unsigned long long *totals = nullptr;
    const int32_t *info_idx = nullptr;
    const uint8_t *info_bits = nullptr;
    int k_info = 0;
    int sat_msg = 0;                 // S_m
    int *counters = nullptr;         // kLayeredCounterInts
    void *c2v_scratch = nullptr;     // [grid][dc_max][m] of the state type when !lds_state (min-sum: [grid] slices)
};

// Envelope and kernel choice for (code, L, mode) on `device`; FPLDPC_ERR_UNSUPPORTED outside the envelope.
int layered_choose(const fpldpc_code &code, int L, int device, int mode, LayeredChoice *out);
int layered_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream);
// The same pair for the min-sum decoder (mode kLayMinsum; lds_state: the check state in LDS, no scratch).
int layered_minsum_choose(const fpldpc_code &code, int L, int device, LayeredChoice *out);
int layered_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream);
// The same pair for the flooding min-sum decoder (mode kFloodMinsum, fpldpc_minsum.hip): no layers.
int flood_minsum_choose(const fpldpc_code &code, int device, LayeredChoice *out);
int flood_minsum_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream);
// The same pair for the saturated flooding decoder (mode kFloodSat, fpldpc_flood_sat.hip): no layers.  `state` is
// fpldpc_flood_create_sat_placed's (validated by the caller): FPLDPC_STATE_LDS keeps the state in LDS only
// (lds_state; FPLDPC_ERR_UNSUPPORTED where it does not fit), _GLOBAL takes the global form, _AUTO the LDS form
// wherever it fits and the global form otherwise.
int flood_sat_choose(const fpldpc_code &code, int device, int state, LayeredChoice *out);
int flood_sat_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream);
// The global form of the saturated flooding decoder (fpldpc_flood_sat_global.hip; !lds_state), which the pair
// above delegates to.  flood_sat_global_choose completes a choice whose mode, dc, exact and threads are set: the
// int16 c2v of every edge and the three accumulators in scratch_bytes = grid * slice of global memory, passed
// as c2v_scratch.
int flood_sat_global_choose(const fpldpc_code &code, int device, LayeredChoice *lc);
int flood_sat_global_launch(const LayeredChoice &lc, const LayeredArgs &args, void *stream);
// The global form of the two min-sum decoders (fpldpc_minsum_global.hip; !lds_state), which the two pairs
// above delegate to where the LDS form does not fit or the environment variable `env` is "global".
// minsum_global_choose completes a choice whose mode, dc, exact and threads are set: the check state (and
// the flooding accumulators) in scratch_bytes = grid * slice of global memory, passed as c2v_scratch.
bool minsum_state_forced_global(const char *env);
int minsum_global_choose(const fpldpc_code &code, int device, LayeredChoice *lc);
int minsum_global_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream);
// The wide form of the two min-sum decoders (fpldpc_minsum_wide.hip; lc.wide), which the two pairs above
// delegate to for a code with check degrees above 64 and for every code under FPLDPC_MINSUM_FORM=wide (a
// diagnostic, read at creation).  minsum_wide_choose makes the whole choice for (mode, threads): check degrees
// 2..255, the state in LDS where it fits unless force_global, the index table placed under `table_env`.
bool minsum_form_forced_wide();
int minsum_wide_choose(const fpldpc_code &code, int mode, int threads, const char *table_env, bool force_global, int device,
                       LayeredChoice *out);
int minsum_wide_launch(const LayeredChoice &lc, const LayeredArgs &args, int scale_16, int offset, void *stream);
// A second layered object of src's code, parameters, L, layers, widths, scale, offset, device and LayeredChoice
// (copied, not chosen again: the environment switches read at creation may have changed since), with device
// tables, counter block, scratch and stream of its own: fpldpc_layered_ber_sim's and fpldpc_minsum_ber_sim's
// second chunk in flight.  No reference bits.  Destroyed by fpldpc_layered_destroy.
int layered_create_twin(fpldpc_layered_t src, fpldpc_layered_t *out);
// Raises a kernel's dynamic-LDS limit on the current device, never lowers it (fpldpc_layered.hip).
hipError_t raise_dynamic_lds(const void *fn, size_t bytes);

}  // namespace fpldpc

// Layered decoder object (fpldpc_layered_t).
struct fpldpc_layered : fpldpc::DecoderCore {
    int L = 0, layers = 0;
    int post_bits = 0, msg_bits = 0;  // fpldpc_layered_create_sat / _minsum; 0: unsaturated
    int scale_16 = 16, offset = 0;    // fpldpc_layered_create_minsum
    fpldpc::LayeredChoice lc;
    uint16_t *d_vidx = nullptr;
    uint8_t *d_cdeg = nullptr;
    int *d_counter = nullptr;
    void *d_scratch = nullptr;
};

// Flooding min-sum decoder object (fpldpc_minsum_t): a type of its own in the C ABI over the same plumbing.
// The saturated flooding decoder (fpldpc_flood_create_sat) is this object too.
struct fpldpc_minsum {
    fpldpc_layered *lay = nullptr;  // mode kFloodMinsum or kFloodSat, owned
};
