/*
 * fpldpc.h -- C ABI of the MI355X-native fixed-point LDPC decoder (libfpldpc.so).
 *
 * Drop-in boundary for the reference's decode path (tyc85/FixedPointLDPC).  The reference has
 * no FFI of its own: its "operator API" is the FP_Decoder class (ArrayLDPCMacro.h:121-158) and
 * the PerfTest.h free functions.  Every entry point below names the reference interface it
 * replaces.  The C++ class-level compatibility layer (FP_Decoder / PerfTest names) is in
 * fpldpc_compat.hpp and is built on this ABI.
 *
 * Conventions
 *   - Every function returns int status: FPLDPC_OK (0) or a negative FPLDPC_ERR_* code; the
 *     message of the last error on the calling thread is fpldpc_last_error().
 *   - "dev" pointers are HIP device pointers, "host" pointers are host memory.  Streams are
 *     hipStream_t passed as void* (NULL = the null stream).
 *   - Decoder objects are independent (no function-static state, unlike the reference's
 *     decode_general_fp, ArrayLDPC_Decoder.cpp:21-37); one object may be used from one thread at
 *     a time, different objects concurrently.
 *   - A decoder is single-stream: its decode calls share one device work counter and fallback
 *     list, so two calls on the same decoder must not overlap on the device (issue them on one
 *     stream, or synchronise between streams).  Use one decoder per stream for concurrency.
 */
#ifndef FPLDPC_H
#define FPLDPC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FPLDPC_OK 0
#define FPLDPC_ERR_ARG (-1)         /* invalid argument */
#define FPLDPC_ERR_IO (-2)          /* file open/read failed (reference: ignored, ReadH :646) */
#define FPLDPC_ERR_FORMAT (-3)      /* malformed / inconsistent alist */
#define FPLDPC_ERR_UNSUPPORTED (-4) /* code shape outside the kernels' envelope */
#define FPLDPC_ERR_HIP (-5)         /* HIP runtime error or no GPU / kernel image */
#define FPLDPC_ERR_NOMEM (-6)

#define FPLDPC_LLR_I32 0 /* const int32_t LLR[batch][n] (the reference's const int *LLR) */
#define FPLDPC_LLR_I16 1 /* const int16_t LLR[batch][n] (compact: |LLR_fp| <= 644 measured) */
#define FPLDPC_LLR_F64 2 /* double LLR[batch][n], unquantised (channel output for fpldpc_decode_float) */

typedef struct fpldpc_code *fpldpc_code_t;
typedef struct fpldpc_decoder *fpldpc_decoder_t;

/* Decoder parameters.  The reference fixes these at compile time (ArrayLDPCMacro.h:17-39). */
typedef struct {
    int32_t max_iter;   /* MAX_ITER, ArrayLDPCMacro.h:17 (default 30) */
    int32_t frac_bits;  /* FRAC_WIDTH, ArrayLDPCMacro.h:36; Constant = int(5/8 * 2^frac) (default 4) */
    int32_t width_mask; /* WIDTH_MASK, ArrayLDPCMacro.h:29, applied inside sxor (default 0xff) */
    int32_t early_term; /* 1 = stop at the first passing syndrome, ArrayLDPC_Decoder.cpp:164-167 (default 1) */
    int32_t precheck;   /* 1 = decode_fixpoint's channel-syndrome pre-check, ArrayLDPC_Decoder.cpp:443-450
                           (iterations 0, hard = channel decision, posteriors left untouched) (default 0) */
    int32_t device;     /* HIP device ordinal; -1 = the calling thread's current device (default -1) */
} fpldpc_params;

const char *fpldpc_last_error(void);
const char *fpldpc_version(void);
/* Content hash (16 hex digits) of the device sources and compile flags this library was built
 * from (no reference counterpart): committed profiler counters are bound to it, so that counters
 * measured on one kernel build are never reported for another.  It covers the kernels with committed
 * counters (flooding, float, generation), not the layered decoder's. */
const char *fpldpc_kernel_build_id(void);

/* ---------------------------------------------------------------- parity-check codes */
/* Replaces FP_Decoder::ReadH() (ArrayLDPC_Decoder.cpp:642-674), which hard-codes
 * "H_802.11_IndZero.txt" and ignores errors.  Alist format: N M / dv_max dc_max / vdeg[N] /
 * cdeg[M] / N vlist rows / M clist rows, 0-based.  Validated: rows ascending (the reference's
 * addr_count bank selection relies on it, :137), vlist/clist consistent, 2 <= cdeg. */
int fpldpc_code_load_alist(const char *path, fpldpc_code_t *out);
int fpldpc_code_parse_alist(const char *text, size_t len, fpldpc_code_t *out);
/* Array code, p prime, r block rows: check (i,j) <-> var k*p + (j + i*k) mod p ("forward",
 * ROM::CirShift ArrayLDPCMacro.h:57 and codes/alist_from_arraycode.m) or (j - i*k) mod p. */
int fpldpc_code_array(int32_t p, int32_t r, int32_t forward, fpldpc_code_t *out);
/* IEEE 802.11n rate-1/2 n=1944 (Z=81) code, the reference's H_802.11_IndZero.txt. */
int fpldpc_code_wifi_1944_r12(fpldpc_code_t *out);
/* dims[0..7] = n, m, dv_max, dc_max, edges, qc_z (0 if not quasi-cyclic), gf2_rank, regular_checks */
int fpldpc_code_dims(fpldpc_code_t code, int32_t dims[8]);
/* ROM::getRate (ArrayLDPCMacro.h:60) for array codes, 1 - rank/n otherwise. */
int fpldpc_code_rate(fpldpc_code_t code, double *rate);
/* Copy out degree and adjacency lists (row-padded to dv_max / dc_max with -1).  Any may be NULL. */
int fpldpc_code_lists(fpldpc_code_t code, int32_t *vdeg, int32_t *cdeg, int32_t *vlist, int32_t *clist);
/* Serialise to alist text; *len receives the size needed (excluding NUL). */
int fpldpc_code_write_alist(fpldpc_code_t code, char *buf, size_t cap, size_t *len);
/* Syndrome of hard bits (uint8 per var) on the host: returns 0 pass, 1 fail, <0 error. */
int fpldpc_code_syndrome_host(fpldpc_code_t code, const uint8_t *bits);
void fpldpc_code_free(fpldpc_code_t code);

/* ---------------------------------------------------------------- decoder */
void fpldpc_params_default(fpldpc_params *p);
/* Replaces constructing FP_Decoder (ArrayLDPCMacro.h:121-176) + ReadH.  Uploads the code's
 * edge tables to the device and picks the kernel variant for the code shape. */
int fpldpc_decoder_create(fpldpc_code_t code, const fpldpc_params *params, fpldpc_decoder_t *out);
int fpldpc_decoder_destroy(fpldpc_decoder_t dec);
/* Kernel variant chosen (e.g. "flood_reg<47,1,regular>") and its resident workgroups. */
int fpldpc_decoder_describe(fpldpc_decoder_t dec, char *buf, size_t cap);
/* Words per frame of the packed hard-decision output: ceil(n / 32). */
int fpldpc_decoder_hard_words(fpldpc_decoder_t dec);
/* Diagnostics (no reference counterpart): frames the most recent fpldpc_decode call on this
 * decoder re-decoded in its exact fallback chain -- counts[0] by the first fallback kernel (frames
 * that left the packed kernel's int16 range, plus a partner sharing their posterior words),
 * counts[1] by the second.  Both 0 for variants without a chain.  Blocking: waits for the last
 * decode call's kernels on whatever stream they were launched (a decode captured into a graph is
 * not tracked: synchronise its replay first). */
int fpldpc_decoder_fallback_counts(fpldpc_decoder_t dec, int32_t counts[2]);

/* Reference information bits for on-device BER accounting.  Replaces setInfoIndex
 * (ArrayLDPC_Decoder.cpp:698-705) + setInfoBit (:178-197): errors are counted as
 * DecodedCodeword[info_index[i]] != info_bits[i] over i < k (calculateBER, :707-722).
 * Host pointers; copied.  k = 0 clears. */
int fpldpc_set_reference(fpldpc_decoder_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k);

/* Batched flooding decode of `batch` frames, asynchronous on `stream` (all pointers device).
 * Replaces per-frame FP_Decoder::decode_general_fp (ArrayLDPC_Decoder.cpp:18-171), or
 * decode_fixpoint (:422-639) when params.precheck = 1, and the result getters.
 *   llr        [batch][n] FPLDPC_LLR_I32 or _I16                              (required)
 *   hard       [batch][hard_words] uint32, bit (v % 32) of word v/32 = DecodedCodeword[v]
 *   iters      [batch] returned iteration count (1..max_iter; 0 on a pre-check pass)
 *   syndrome_ok[batch] 1 if the output hard decision satisfies H
 *   post       [batch][n] int32 Posteriori_fp (getPost_fp, ArrayLDPCMacro.h:138)
 *   bit_errors [batch] calculateBER per frame (needs fpldpc_set_reference)
 *   totals     [4] int64, ADDED to: {bit_errors, frame_errors, frames, iteration_sum}
 * Any output may be NULL.  Bit-exact with the reference decoder for every frame. */
int fpldpc_decode(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t batch,
                  uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok, int32_t *post,
                  int32_t *bit_errors, int64_t *totals, void *stream);
/* Same on host buffers (synchronous; stages through device memory owned by the decoder). */
int fpldpc_decode_host(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t batch,
                       uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok, int32_t *post,
                       int32_t *bit_errors, int64_t *totals);

/* Stateful single-frame decode: FP_Decoder::decode_general_fp / decode_fixpoint with the decoder's
 * edge RAM kept across calls, as the reference's FSM uses it (ArrayLDPC_Decoder.cpp:443-488,
 * :621-630).  edge_ram is FP_Decoder's EdgeRAM (ArrayLDPCMacro.h:162), owned by the caller:
 * int32 edge_ram[k * m + c] = the v2c message on slot k (clist order) of check c as the last
 * variable-node phase left it (accum - c2v, :152 and :615); fpldpc_edge_ram_words gives dc_max * m.
 *   keep_edges = 0: edge init from the channel values first (:45-61, decode_fixpoint in state PCV
 *                   :462-485) -- decode_general_fp, or decode_fixpoint after setState(PCV);
 *   keep_edges = 1: no edge init: iterate from edge_ram with these LLRs in the variable-node phase
 *                   -- decode_fixpoint in state C2V without setState(PCV) (:488-618).
 * With params.precheck the channel syndrome is tested first (:443-450): on a pass the frame returns
 * 0 iterations with the channel decision and edge_ram / post left as they were.  Otherwise edge_ram
 * is overwritten with the final edge messages; iterations, hard decisions, syndrome flag and
 * posteriors as fpldpc_decode for one frame.  One workgroup of the int32 kernel (flood_edges):
 * the per-frame drop-in path; batches belong to fpldpc_decode.  Device pointers, async on stream.
 * The decoder holds one c2v scratch for this path: calls on one decoder must be serialised (one
 * stream, or wait for the previous call), even with distinct edge_ram buffers -- independent
 * per-channel states need one decoder each. */
int fpldpc_edge_ram_words(fpldpc_decoder_t dec, int64_t *words);
int fpldpc_decode_frame(fpldpc_decoder_t dec, const void *llr, int32_t llr_type, int32_t keep_edges,
                        int32_t *edge_ram, uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok,
                        int32_t *post, void *stream);
/* Same on host buffers (synchronous); llr int32[n]; post (nullable) in/out like fpldpc_decode_host. */
int fpldpc_decode_frame_host(fpldpc_decoder_t dec, const int32_t *llr, int32_t keep_edges, int32_t *edge_ram,
                             uint32_t *hard, int32_t *iters, uint8_t *syndrome_ok, int32_t *post);

/* Floating-point BP decode (exact-Jacobian box-plus in double), replacing FP_Decoder::decode_general
 * (ArrayLDPC_Decoder.cpp:735-933, sxor(double,double) :724-732, checkPost :335-372) batched, async
 * on `stream`, device pointers.  llr [batch][n] double (unquantised, e.g. fpldpc_channel_llr with
 * FPLDPC_LLR_F64); post [batch][n] double (getPost, ArrayLDPCMacro.h:149); the other outputs as
 * fpldpc_decode.  Uses params.max_iter and early_term; frac_bits, width_mask and precheck do not
 * apply.  Same flooding schedule and fold order as the reference, but by default each check's exact
 * box-plus is folded in the tanh domain (E = exp(-|x|), E_r = (E_x + E_y) / (1 + E_x E_y), one exp
 * in and one log out per edge); the reference's log-domain operation order is used only for a check
 * holding a message >= 690 in magnitude, or in a build with -DFPLDPC_FLOAT_TANH=0.  Different
 * rounding, same decisions: tests/test_gpu_float.py requires 0 frames differing in iterations / hard
 * decisions from the reference's fixtures and the oracle, and posteriors within 1e-8 relative
 * (measured worst 3.4e-9).  Supports n <= 16384, degrees <= 255. */
int fpldpc_decode_float(fpldpc_decoder_t dec, const double *llr, int32_t batch, uint32_t *hard,
                        int32_t *iters, uint8_t *syndrome_ok, double *post, int32_t *bit_errors,
                        int64_t *totals, void *stream);
/* Same on host buffers (synchronous; stages through the decoder's device memory and stream, the ones
 * fpldpc_decode_host uses). */
int fpldpc_decode_float_host(fpldpc_decoder_t dec, const double *llr, int32_t batch, uint32_t *hard,
                             int32_t *iters, uint8_t *syndrome_ok, double *post, int32_t *bit_errors,
                             int64_t *totals);

/* ---------------------------------------------------------------- layered decoder */
/* The layered (row-serial) schedule of the same fixed-point arithmetic (no reference counterpart: the
 * reference decodes by flooding only; this is the schedule quasi-cyclic / array-code hardware uses).
 * Per frame post[v] = LLR[v] and c2v[c][k] = 0 for slot k (clist order) of check c.  With
 * params.precheck the channel syndrome is tested first, as in fpldpc_decode.  Then, for
 * it = 1 .. max_iter and for each check c = 0 .. m-1 in code (alist) order, one after another:
 *     t[k] = post[v_k] - c2v[c][k]                                  (k < deg)
 *     new  = the reference's forward/backward sxor fold of t        (ArrayLDPC_Decoder.cpp:66-118)
 *     c2v[c][k] = new[k],  post[v_k] = t[k] + new[k]
 * and after the last check hard[v] = post[v] > 0 ? 0 : 1, the syndrome over clist, iters = it; with
 * early_term the frame stops on a pass.  Nothing is saturated (fpldpc_layered_create_sat is the
 * saturated form, defined for every input).
 * Envelope: results are defined while every intermediate fits int32 (the reference's own arithmetic
 * has the same limit).  Unsaturated posteriors roughly double per layer once a frame is converging:
 * the array code p = 47, r = 24 at 8 dB reaches 1.1e8 inside its single iteration, so a second
 * iteration (early_term = 0) would leave int32.  Check degrees 2..64, n <= 40956.
 * Layers are parallelism only, not semantics: checks [l*L, (l+1)*L) form layer l and are updated at
 * once, which equals the serial order because no variable occurs twice inside a layer. */
typedef struct fpldpc_layered *fpldpc_layered_t;
/* Host only, no GPU: out = {layer_checks used, layers}.  layer_checks = 0 picks the array code's p,
 * else qc_z when it gives valid layers, else 1 (always valid: rows are ascending).  FPLDPC_ERR_ARG
 * if layer_checks < 0 or does not divide m, FPLDPC_ERR_UNSUPPORTED if a variable repeats inside a
 * layer. */
int fpldpc_code_layering(fpldpc_code_t code, int32_t layer_checks, int32_t out[2]);
/* All six fpldpc_params fields apply.  FPLDPC_ERR_HIP without a HIP device, FPLDPC_ERR_UNSUPPORTED
 * (with a message) outside the envelope above. */
int fpldpc_layered_create(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks, fpldpc_layered_t *out);
/* The saturated layered decoder: the same schedule with posteriors post_bits wide and messages msg_bits
 * wide, defined for EVERY input (the unsaturated one above only while its intermediates fit int32).
 * With S_p = 2^(post_bits-1) - 1, S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S) and
 * C = the reference's Constant, int(5/8 * 2^frac_bits), per frame
 *     post[v] = clamp(LLR[v], S_p);  c2v[c][k] = 0
 *     for it = 1 .. max_iter, for each check c in code order:
 *         t[k]      = clamp(post[v_k] - c2v[c][k], S_m)
 *         new       = the reference's forward/backward sxor fold of t      (unchanged)
 *         c2v[c][k] = new[k]
 *         post[v_k] = clamp(t[k] + new[k], S_p)
 * Hard decision, syndrome, iters, early termination, layers and outputs as above (post stays int32);
 * precheck tests the clamped LLRs (the clamp keeps every sign) and leaves post untouched.
 * Bounds: |sxor(x, y)| <= min(|x|, |y|) + C, so every fold value and every c2v is at most S_m + C,
 * |post| <= S_p, and in registers |post - c2v| <= S_p + S_m + C and |t + new| <= 2 S_m + C.
 * FPLDPC_ERR_ARG (with a message, tested before a HIP device is looked for) unless
 *     2 <= msg_bits < post_bits <= 24   and   S_p > S_m + C.
 * Two widths, because one does not work: sgn(0) = -1 in the reference's sxor, and with S_m = S_p a
 * posterior pinned at S_p minus its own message near S_p gives t = 0, a message of the wrong sign (A at
 * 8 dB: no frame decodes).  S_p > S_m + C is that reason as a rule: a pinned posterior minus its own
 * message (at most S_m + C) keeps its sign.
 * post_bits <= 16 keeps posteriors and c2v as int16 on chip (S_m + C <= 32767 follows from the rule),
 * 17..24 as int32.  Check degrees 2..64; n <= 40956 with int32 state, any code's n (<= 65535) with int16 state.
 * The object is an fpldpc_layered_t like any other: destroy, describe (which adds sat=<post_bits>/<msg_bits>
 * and state=i16|i32), set_reference, decode and decode_host below apply unchanged. */
int fpldpc_layered_create_sat(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks,
                              int32_t post_bits, int32_t msg_bits, fpldpc_layered_t *out);
/* The layered min-sum decoder: the saturated schedule above with the check rule layered hardware runs,
 * normalised / offset min-sum, in place of the sxor fold.  With S_p, S_m and clamp as above and
 * f(x) = max(((x * scale_16) >> 4) - offset, 0) for x >= 0, per frame
 *     post[v] = clamp(LLR[v], S_p);  c2v[c][k] = 0
 *     for it = 1 .. max_iter, for each check c in code order:
 *         t[k]   = clamp(post[v_k] - c2v[c][k], S_m)                 (k < deg)
 *         s[k]   = t[k] <= 0          (the reference's sgn(0) = -1, the same rule as the hard decision)
 *         m1     = min_k |t[k]|,  k1 = a slot attaining it,  m2 = min_{k != k1} |t[k]|
 *         mag[k] = f(k == k1 ? m2 : m1)
 *         new[k] = (parity of s[j] over j != k) ? -mag[k] : mag[k]
 *         c2v[c][k] = new[k];  post[v_k] = clamp(t[k] + new[k], S_p)
 * Which slot is k1 on a tie changes no output: then m2 = m1.  scale_16 = 16, offset = 0 is plain min-sum,
 * which is the saturated decoder above at frac_bits = 0 (C = 0: sxor is sign * min) bit for bit.
 * Everything else is as in the saturated decoder: hard decision, syndrome, iters, early termination,
 * precheck on the clamped LLRs with post left untouched, layers as parallelism, outputs (post is int32).
 * Bounds: 0 <= f(x) <= x, so |c2v| <= S_m, |post| <= S_p, and in registers |post - c2v| <= S_p + S_m and
 * |t + new| <= 2 S_m, for every input.
 * FPLDPC_ERR_ARG (with a message, tested before a HIP device is looked for) unless
 *     2 <= msg_bits < post_bits <= 16,   1 <= scale_16 <= 16,   0 <= offset <= S_m.
 * S_p > S_m keeps the sign of a pinned posterior minus its own message; the on-chip state is int16.
 * params.frac_bits and params.width_mask are validated as for the other decoders; the arithmetic does not
 * use them.  On chip a check keeps 16 bytes whatever its degree -- f(m1), f(m2), k1 and a 64-bit sign
 * word, from which every c2v[c][k] is rebuilt -- so there is no per-edge state.
 * Envelope: check degrees 2..255 (the degree tables are bytes; a degree above 255 is FPLDPC_ERR_UNSUPPORTED,
 * "check degree above 255"), a valid layering and n <= 65535; no code is refused for its size.  A code with a
 * check degree above 64 -- and, under the diagnostic FPLDPC_MINSUM_FORM=wide read at creation, any code; any other
 * value is ignored -- takes the wide form: W = ceil(dc_max / 32) sign words in place of the 64-bit word, 8 + 4 W
 * bytes per check { f(m1) | f(m2) << 16, k1 | parity << 31, W words of sign bits }, of which an all-zero entry is
 * every message 0; in LDS wherever 2 n + (9 + 4 W) m + 18 bytes at most fit, else in slices of
 * roundup((8 + 4 W) m, 256) bytes; describe names it layered_minsum_wide<DC=32 W,..>.  For the other codes:
 * placement of the check state: in LDS wherever the int16 posteriors, the control
 * words and 16 (17 with mixed degrees) bytes per check, 2 n + 17 m + 16 bytes at most, fit the CU's 160 KiB,
 * with no global scratch; otherwise "global": LDS keeps the posteriors, the control words and (where they
 * fit) the degrees, and each resident workgroup keeps its frame's state [m] x 16 bytes in a slice of
 * roundup(16 m, 256) bytes of a scratch of grid * slice bytes that the decoder owns.  The environment variable
 * FPLDPC_LAYERED_MINSUM_STATE=global, read at creation, chooses the global placement for a code that fits
 * (a diagnostic switch; any other value is ignored).  Results do not depend on the placement.
 * The object is an fpldpc_layered_t like any other: destroy, set_reference, decode and decode_host apply
 * unchanged; describe names the kernel layered_minsum<..> (with ",mem=global" inside the brackets in the
 * global placement) and ends with " sat=<post_bits>/<msg_bits> ms=<scale_16>/16-<offset> state=compressed",
 * followed by " scratch=<bytes>" in the global placement. */
int fpldpc_layered_create_minsum(fpldpc_code_t code, const fpldpc_params *params, int32_t layer_checks,
                                 int32_t post_bits, int32_t msg_bits, int32_t scale_16, int32_t offset,
                                 fpldpc_layered_t *out);
int fpldpc_layered_destroy(fpldpc_layered_t dec);
/* Kernel variant, L, layers, resident workgroups, threads, LDS bytes. */
int fpldpc_layered_describe(fpldpc_layered_t dec, char *buf, size_t cap);
/* As fpldpc_set_reference. */
int fpldpc_layered_set_reference(fpldpc_layered_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k);
/* Conventions and outputs as fpldpc_decode: device pointers, asynchronous on `stream`, any output may
 * be NULL, I32 / I16 LLRs, totals ADDED to; one object per stream (its calls share one work counter). */
int fpldpc_layered_decode(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                          int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                          void *stream);
/* Same on host buffers (synchronous; stages through device memory owned by the decoder). */
int fpldpc_layered_decode_host(fpldpc_layered_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                               int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors,
                               int64_t *totals);

/* ---------------------------------------------------------------- flooding min-sum decoder */
/* Normalised / offset min-sum, saturated and defined for every input, on the flooding schedule: the check
 * rule, the clamps and the compressed check state of fpldpc_layered_create_minsum, with every check of a
 * step reading the same posteriors (the schedule of fpldpc_decode).  S_p = 2^(post_bits-1) - 1,
 * S_m = 2^(msg_bits-1) - 1, clamp(x, S) = min(max(x, -S), S) and f(x) = max(((x * scale_16) >> 4) - offset, 0)
 * are those of the layered min-sum decoder.  Per frame
 *     L[v] = clamp(LLR[v], S_p);  post[v] = L[v];  c2v[c][k] = 0
 *     for it = 1 .. max_iter:
 *         for every check c, all reading the same post (no order between checks):
 *             t[k]   = clamp(post[v_k] - c2v[c][k], S_m)                  (k < deg)
 *             s[k]   = t[k] <= 0
 *             m1 = min_k |t[k]|,  k1 = a slot attaining it,  m2 = min_{k != k1} |t[k]|
 *             new[k] = (parity of s[j], j != k) ? -f(k == k1 ? m2 : m1) : f(k == k1 ? m2 : m1)
 *             c2v[c][k] = new[k]
 *         for every variable v:  post[v] = clamp(L[v] + sum of c2v[c][k] over the edges (c, k) with v_k = v, S_p)
 *         hard[v] = post[v] > 0 ? 0 : 1;  the syndrome over clist;  iters = it;  with early_term stop on a pass
 * With params.precheck the syndrome of the clamped LLRs is tested first; on a pass the frame returns 0
 * iterations with the channel decision and post is left untouched.  Outputs as fpldpc_decode (post is int32,
 * totals are ADDED to).
 * scale_16 = 16, offset = 0 at widths where no clamp acts (clipped values: none) is fpldpc_decode at
 * frac_bits = 0 bit for bit: there the reference's Constant is 0 and its sxor is sign * min.
 * Bounds, for every input: |c2v| <= S_m, |post| <= S_p, |post - c2v| <= S_p + S_m and
 * |L + sum| <= S_p + dv_max * S_m (an int32 accumulator on chip; its sign is the posterior's).
 * FPLDPC_ERR_ARG (with a message, tested before a HIP device is looked for) unless
 *     2 <= msg_bits < post_bits <= 16,   1 <= scale_16 <= 16,   0 <= offset <= S_m.
 * params.frac_bits and params.width_mask are validated as for the other decoders; the arithmetic does not
 * use them.  A check keeps 16 bytes whatever its degree, as in the layered min-sum decoder; there is no
 * per-edge state.  Envelope: check degrees 2..255 (the degree tables are bytes) and n <= 65535; outside it
 * FPLDPC_ERR_UNSUPPORTED (with a message: "check degree above 255"); no code is refused for its size.  A code
 * with a check degree above 64 -- and, under the diagnostic FPLDPC_MINSUM_FORM=wide read at creation, any code;
 * any other value is ignored -- takes the wide form with the check state of the layered min-sum decoder's wide
 * form (8 + 4 W bytes per check, W = ceil(dc_max / 32)): in LDS wherever 14 n + (9 + 4 W) m + 18 bytes at most
 * fit, else in slices of roundup((8 + 4 W) m + 12 n, 256) bytes; describe names it flood_minsum_wide<DC=32 W,..>.  For the
 * other codes: placement of the state: in LDS
 * wherever 14 n + 17 m + 32 bytes (three int32 accumulators, the int16 LLRs, the state and the degrees; the
 * index table joins them only where it fits) fit the CU's 160 KiB, with no global scratch; otherwise
 * "global": LDS keeps the int16 LLRs, the control words and (where they fit) the degrees, and each resident
 * workgroup keeps its frame's state [m] x 16 bytes and accumulators [3][n] int32 in a slice of
 * roundup(16 m + 12 n, 256) bytes of a scratch of grid * slice bytes that the decoder owns.  The environment
 * variable FPLDPC_MINSUM_STATE=global, read at creation, chooses the global placement for a code that fits
 * (a diagnostic switch; any other value is ignored).  Results do not depend on the placement.
 * FPLDPC_ERR_HIP without a HIP device. */
typedef struct fpldpc_minsum *fpldpc_minsum_t;
int fpldpc_minsum_create(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                         int32_t scale_16, int32_t offset, fpldpc_minsum_t *out);
/* The saturated flooding decoder: the reference's own schedule (flooding) and check rule (the box-plus sxor in
 * the forward/backward fold) with posteriors post_bits wide and messages msg_bits wide, defined for EVERY input
 * (fpldpc_decode, the unsaturated int32 reference, only while its intermediates fit).
 * S_p = 2^(post_bits-1) - 1 and S_m = 2^(msg_bits-1) - 1;  clamp(x, S) = min(max(x, -S), S);  C is the
 * reference's Constant, int(5/8 * 2^frac_bits);  sxor and the forward/backward fold are the reference's
 * (ArrayLDPC_Decoder.cpp:66-118, :677-694, sgn(0) = -1), in clist order.  Per frame
 *     L[v] = clamp(LLR[v], S_p);  post[v] = L[v];  c2v[c][k] = 0
 *     for it = 1 .. max_iter:
 *         for every check c, all reading the same post (no order between checks):
 *             t[k]      = clamp(post[v_k] - c2v[c][k], S_m)          (k < deg)
 *             new       = the reference's forward/backward sxor fold of t, with C and width_mask
 *             c2v[c][k] = new[k]
 *         for every variable v:  post[v] = clamp(L[v] + sum of c2v[c][k] over the edges with v_k = v, S_p)
 *         hard[v] = post[v] > 0 ? 0 : 1;  the syndrome over clist;  iters = it;  with early_term stop on a pass
 * With params.precheck the syndrome of the clamped LLRs is tested first; on a pass the frame returns 0
 * iterations with the channel decision and post is left untouched: the same rule as the other saturated
 * decoders.  Outputs follow fpldpc_minsum_decode: post is int32 and totals are ADDED to.  All six fpldpc_params
 * fields apply: frac_bits gives C and width_mask is sxor's mask.
 * Bounds, for every input: |sxor(x, y)| <= min(|x|, |y|) + C, so every fold value and every c2v is at most
 * S_m + C;  |post| <= S_p;  |post - c2v| <= S_p + S_m + C;  |L + sum| <= S_p + dv_max * (S_m + C) (an int32
 * accumulator on chip; its sign is the posterior's).
 * FPLDPC_ERR_ARG (with a message that begins "saturated flooding decoder:" and names the rule, tested before a
 * HIP device is looked for) unless
 *     2 <= msg_bits < post_bits <= 16   and   S_p > S_m + C.
 * S_p > S_m + C is fpldpc_layered_create_sat's reason carried over: a posterior pinned at S_p, minus its own
 * message, keeps its sign.  S_m + C <= 32767 follows from the rule, so the per-edge state is always int16.
 * Identity: where no clamp acts this is fpldpc_decode at the same frac_bits and width_mask, bit for bit, in every
 * output (the reference's stored v2c = post - c2v is t, its K1 initialisation is c2v = 0).
 * Envelope: check degrees 2..64, n <= 65535, and, in this call, the state in LDS -- c2v [dc_max][m] int16 (up to
 * a whole word), three int32 accumulators [n], the int16 LLRs, 16 bytes of control words and one byte per check
 * with mixed degrees within the CU's 160 KiB; the index table joins them only where it fits and costs no resident
 * workgroup (FPLDPC_FLOOD_SAT_TABLE=global / lds, read at creation, places it regardless: a diagnostic switch).
 * Outside it FPLDPC_ERR_UNSUPPORTED with a message that names the decoder and the reason ("check degree above
 * 64", or the bytes that do not fit 160 KiB of LDS).  A code whose state does not fit is decoded by the global
 * form, which fpldpc_flood_create_sat_placed (below) gives on request; there is no wide form.
 * FPLDPC_ERR_HIP without a HIP device.
 * The object is an fpldpc_minsum_t like any other -- the type is named after its first check rule, not after
 * what every object of it runs: fpldpc_minsum_destroy, _set_reference, _decode, _decode_host and every
 * fpldpc_minsum_ber_sim* entry point apply unchanged, and fpldpc_minsum_describe prints
 * "flood_sat<DC=..,addr=computed|table|gtable,deg=exact|table> grid=N threads=N lds=N device=N
 * sat=<post_bits>/<msg_bits> state=i16". */
int fpldpc_flood_create_sat(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits, int32_t msg_bits,
                            fpldpc_minsum_t *out);
/* The same decoder -- definition, rules on the widths, outputs and entry points as fpldpc_flood_create_sat -- with
 * the placement of its state chosen by the caller:
 *     FPLDPC_STATE_LDS     fpldpc_flood_create_sat itself, its refusal and message included;
 *     FPLDPC_STATE_GLOBAL  the global form for any code of the envelope (check degrees 2..64, n <= 65535), also one
 *                          whose state fits LDS: LDS keeps the int16 LLRs, 16 bytes of control words and the degree
 *                          table (where 2 n + 16 + m bytes fit 160 KiB); every resident workgroup owns a slice of a
 *                          scratch the decoder allocates at creation, c2v [dc_max][m] int16 (up to a whole word) and
 *                          three int32 accumulators [n], rounded up to 256 bytes; the index table stays in global
 *                          memory and a forward array code reads it too;
 *     FPLDPC_STATE_AUTO    the LDS form wherever its bytes fit (kernel, grid and describe line as FPLDPC_STATE_LDS
 *                          gives them), else the global form.
 * Every placement gives the same outputs, bit for bit.  Any other `state` is FPLDPC_ERR_ARG with a message that
 * begins "saturated flooding decoder:", tested with the widths before a HIP device is looked for.
 * fpldpc_minsum_describe prints the global form as
 * "flood_sat<DC=..,addr=gtable,deg=exact|table,mem=global> grid=N threads=N lds=N device=N
 * sat=<post_bits>/<msg_bits> state=i16 scratch=<bytes>" (scratch = grid * slice). */
#define FPLDPC_STATE_LDS 0
#define FPLDPC_STATE_GLOBAL 1
#define FPLDPC_STATE_AUTO 2
int fpldpc_flood_create_sat_placed(fpldpc_code_t code, const fpldpc_params *params, int32_t post_bits,
                                   int32_t msg_bits, int32_t state, fpldpc_minsum_t *out);
int fpldpc_minsum_destroy(fpldpc_minsum_t dec);
/* "flood_minsum<DC=..,addr=computed|table|gtable,deg=exact|table> grid=N threads=N lds=N device=N
 * sat=<post_bits>/<msg_bits> ms=<scale_16>/16-<offset> state=compressed"; in the global placement
 * "flood_minsum<DC=..,addr=gtable,deg=exact|table,mem=global> ... state=compressed scratch=<bytes>".
 * A decoder of fpldpc_flood_create_sat: the line given there. */
int fpldpc_minsum_describe(fpldpc_minsum_t dec, char *buf, size_t cap);
/* As fpldpc_set_reference. */
int fpldpc_minsum_set_reference(fpldpc_minsum_t dec, const int32_t *info_index, const uint8_t *info_bits, int32_t k);
/* Conventions and outputs as fpldpc_layered_decode: device pointers, asynchronous on `stream`, any output
 * may be NULL, I32 / I16 LLRs, totals ADDED to; one object per stream (its calls share one work counter). */
int fpldpc_minsum_decode(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                         int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors, int64_t *totals,
                         void *stream);
/* Same on host buffers (synchronous; stages through device memory owned by the decoder). */
int fpldpc_minsum_decode_host(fpldpc_minsum_t dec, const void *llr, int32_t llr_type, int32_t batch, uint32_t *hard,
                              int32_t *iters, uint8_t *syndrome_ok, int32_t *post, int32_t *bit_errors,
                              int64_t *totals);

/* ---------------------------------------------------------------- channel model */
/* Lehmer state after `draws` calls of Random() from `seed` (rngs.cpp:52-69, a = 48271,
 * m = 2^31 - 1): seed * a^draws mod m. */
int64_t fpldpc_rng_skip(int64_t seed, uint64_t draws);
/* Quantised BPSK/AWGN LLRs exactly as the reference harness (PerfTest.cpp:108-120, 287-297):
 *   LLR_fp[f][i] = (int)(2*snr*(1 - 2*cw[i] + Normal(0, sigma)) * 2^frac_bits)
 * Normal = Odeh-Evans inverse CDF on one Random() draw (rvgs.cpp:152-181); frame f uses draws
 * [f*n, (f+1)*n) of the stream started at `seed` (the reference never re-seeds, rngs.cpp:47).
 * cw (uint8[n]) NULL = all-zero codeword.  out is [frames][n] of out_type; FPLDPC_LLR_F64 stores
 * the unquantised double 2*snr*(...) (PerfTest.cpp:108-110, the float decoder's input).
 * nthreads <= 0: all.
 * Returns FPLDPC_ERR_ARG if a value does not fit int16 for FPLDPC_LLR_I16. */
int fpldpc_channel_llr_host(int64_t seed, int64_t first_frame, int32_t frames, int32_t n,
                            double snr, double sigma, int32_t frac_bits, const uint8_t *cw,
                            void *out, int32_t out_type, int32_t nthreads);
/* The same channel on the device, asynchronous on `stream` (hipStream_t, NULL = default): every
 * pointer is device memory.  cw NULL = all-zero codeword; else cw is uint8[n] shared by all frames
 * (cw_per_frame = 0) or uint8[frames][n] (cw_per_frame = 1, e.g. fpldpc_encoder_encode output).
 * The Lehmer states are the host's exactly; the normals use the device's double log/sqrt, so an
 * LLR can in principle differ from the host's by one quantum where the product lands within an
 * ulp of an integer (never observed: tests/test_gpu_gen.py compares the full KAT-W stream).
 * For FPLDPC_LLR_I16, the number of values outside int16 is added to *overflow (device int32, may
 * be NULL; the caller zeroes it); such values are stored truncated to 16 bits. */
int fpldpc_channel_llr(int64_t seed, int64_t first_frame, int32_t frames, int32_t n, double snr,
                       double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame,
                       void *out, int32_t out_type, int32_t *overflow, void *stream);

/* ---------------------------------------------------------------- noise sources */
/* The Lehmer stream above is the reference's and stays the default of everything that makes noise.  Its period is
 * 2^31 - 2 draws and frame f uses draws [f*n, (f+1)*n): at n = 2209 the stream wraps every 972,152 frames, at
 * n = 1944 frames f and f + 119,304,647 receive identical noise, and nothing reports either; one 31-bit uniform
 * per variate bounds |z| near 6.2.  FPLDPC_NOISE_PHILOX is a counter-based source beside it: the variate is a pure
 * function of (seed, frame, position), no two frames share noise for any run length, and the uniforms carry 53
 * bits.  Every entry point that takes a `source` accepts these two values; any other is FPLDPC_ERR_ARG. */
#define FPLDPC_NOISE_LEHMER 0 /* the reference's stream; everything without a source argument */
#define FPLDPC_NOISE_PHILOX 1
/* Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments
 * 0x9E3779B9, 0xBB67AE85.  One round maps (c0, c1, c2, c3) to
 *     (hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),  hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0));
 * ten rounds, the key bumped after each.  For seed S (0 <= S < 2^63), frame f >= 0 and position i in [0, n):
 *     key     = (S & 0xffffffff, S >> 32)
 *     counter = (i >> 1, 0, f & 0xffffffff, f >> 32)     word 1 is a stream id: 0 = channel noise, others reserved
 *     (r0, r1, r2, r3) = Philox4x32-10(counter, key)
 *     a = (r0 | r1 << 32) >> 11,   b = (r2 | r3 << 32) >> 11
 *     u1 = (a + 1) * 2^-53  in (0, 1],   u2 = b * 2^-53  in [0, 1)
 *     rad = sqrt(-2 ln u1)
 *     z   = rad * cos(2 pi u2) for even i,   rad * sin(2 pi u2) for odd i        (|z| <= 8.58)
 *     nrm = 0.0 + sigma * z;  LLR = (2*snr) * ((1 - 2*cw[i]) + nrm);  LLR_fp = (int)(LLR * 2^frac_bits)
 * The last three operations and the I16 / I32 / F64 outputs are the Lehmer channel's exactly (each operation
 * rounded once, no contraction, the int16 overflow rules).  One Philox call serves the two positions of a pair;
 * with odd n the last pair's sine half is unused.  Frame indices are limited only by first_frame + frames < 2^63:
 * there is no 2^48 rule and no period.  ln, sin and cos come from the C library of the side that runs (the device
 * uses sincospi(2*u2), where 2*u2 is exact), so the transform is defined as the mathematical value: two
 * implementations agree to a few ulps of z, an F64 output within 1e-12 * 2*snr * (1 + 9*sigma), a quantised one
 * exactly except where LLR * 2^frac_bits lies that close to an integer (tests/philox_model.py).  The same device
 * call always gives the same bits.
 * The information bits of random_info (fpldpc_info_bits) stay on their Lehmer generator whatever the noise
 * source: a repeated information word only repeats a codeword, and the code is linear.
 * Host only: the primitive that replays a frame without this library's channel. */
void fpldpc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* fpldpc_channel_llr_host / fpldpc_channel_llr on `source`.  FPLDPC_NOISE_LEHMER: exactly those functions, under
 * their argument rules.  FPLDPC_NOISE_PHILOX: 0 <= seed < 2^63, first_frame >= 0, first_frame + frames < 2^63,
 * every other rule as before; the host result does not depend on nthreads or on how a frame range is split into
 * calls. */
int fpldpc_channel_llr_src_host(int32_t source, int64_t seed, int64_t first_frame, int32_t frames, int32_t n,
                                double snr, double sigma, int32_t frac_bits, const uint8_t *cw, void *out,
                                int32_t out_type, int32_t nthreads);
int fpldpc_channel_llr_src(int32_t source, int64_t seed, int64_t first_frame, int32_t frames, int32_t n, double snr,
                           double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out,
                           int32_t out_type, int32_t *overflow, void *stream);

/* ---------------------------------------------------------------- systematic encoder */
/* Replaces FP_Encoder (ArrayLDPC_Encoder.cpp:22-225, decl ArrayLDPCMacro.h:179-214). */
typedef struct fpldpc_encoder *fpldpc_encoder_t;
/* FP_Encoder(char *Filename, int) (:34-157): the reference's G file ("N M_G / x cmax /
 * ColumnFlag[N] / ChkDeg[M_G] / rows").  Unlike the reference, errors are returned, not exit(0). */
int fpldpc_encoder_load_g(const char *path, fpldpc_encoder_t *out);
/* The same encoder derived natively from H (what codes/simplfy_generator_alist.m made offline):
 * parity positions = pivot columns of a column-order GF(2) row reduction, info = the rest in
 * ascending order; identical to the reference's G files for its codes (tests/test_encoder.py). */
int fpldpc_encoder_from_code(fpldpc_code_t code, fpldpc_encoder_t *out);
/* dims = n, k, max parity-row weight */
int fpldpc_encoder_dims(fpldpc_encoder_t enc, int32_t dims[3]);
/* getInfoIndex (ArrayLDPCMacro.h:186): info_index[k], parity_index[n-k]; either may be NULL. */
int fpldpc_encoder_info_index(fpldpc_encoder_t enc, int32_t *info_index, int32_t *parity_index);
/* setInfoBit / encode bit unpacking of a char stream (ArrayLDPC_Decoder.cpp:178-197). */
int fpldpc_unpack_info_bytes(const char *in, int32_t in_len, int32_t k, uint8_t *bits);
/* encode (:160-225) of `batch` frames: info [batch][k] bits -> cw [batch][n] bits (host). */
int fpldpc_encoder_encode_host(fpldpc_encoder_t enc, const uint8_t *info, int32_t batch, uint8_t *cw, int32_t nthreads);
/* The same on the device, asynchronous on `stream`: info [batch][k] and cw [batch][n] are device
 * uint8 arrays (bit in the LSB).  The encoder binds to the current device on first use and keeps
 * a packed-info scratch sized to the largest batch seen: like a decoder, one encoder object is
 * used from one thread / stream at a time. */
int fpldpc_encoder_encode(fpldpc_encoder_t enc, const uint8_t *info, int32_t batch, uint8_t *cw, void *stream);
void fpldpc_encoder_free(fpldpc_encoder_t enc);

/* ---------------------------------------------------------------- BER/FER simulation */
/* The frame loop the reference's harness runs around one decoder (ArrayLDPC_Debug_Wifi
 * PerfTest.cpp:97-135, ArrayLDPC_Debug :275-311, ArrayLDPC_Debug_Shorten :385-426,
 * ArrayLDPC_PerfTest :485-511, ArrayLDPC_TimeTrial :574-600), batched: frames are generated on the
 * host (channel model above, skip-ahead, all threads) while the GPU decodes the previous chunk, and
 * errors are accounted IN FRAME ORDER so that "stop at the frame with the Nth frame error" is
 * reproduced exactly.  Two chunks are in flight: the call creates a twin of `dec` (same code,
 * parameters and kernel choice, no diagnostics; its own stream and a second set of decoder device
 * buffers, about the decoder's own footprint) for the duration of the call, and submits the next
 * chunk before waiting for the current one, so that its launch fills the CUs a chunk's last frames
 * leave idle (environment FPLDPC_SIM_OVERLAP=0: one chunk at a time on `dec` alone).  Counters are
 * the same either way; a chunk decoded past the stop frame is waited for and not counted. */
#define FPLDPC_COUNT_BITS 0  /* blkerror = calculateBER() (ArrayLDPC_Decoder.cpp:707-722) */
#define FPLDPC_COUNT_ITERS 1 /* blkerror = decode_fixpoint()'s return value: the reference's
                                ArrayLDPC_PerfTest/TimeTrial count iterations as bit errors
                                (PerfTest.cpp:507-510, 596-600); kept for output parity */
typedef struct {
    int64_t seed;                 /* Lehmer state of draw 0 (rngs.cpp:45 DEFAULT = 123456789) */
    int64_t first_frame;          /* frame f uses draws [f*n, (f+1)*n) */
    double snr, sigma;            /* LLR = 2*snr*(1 - 2c + Normal(0, sigma)), PerfTest.cpp:108-120 */
    int32_t frac_bits;            /* LLR_fp = (int)(LLR * 2^frac_bits) */
    const uint8_t *codeword;      /* [n] transmitted codeword, NULL = all-zero */
    const int32_t *info_index;    /* [k] setInfoIndex (host) */
    const uint8_t *info_bits;     /* [k] setInfoBit (host) */
    int32_t k;
    const int32_t *forced_index;  /* shortening: LLR_fp[forced_index[i]] = forced_llr after the */
    int32_t n_forced;             /* channel (PerfTest.cpp:410-414); NULL/0 = none */
    int32_t forced_llr;
    int64_t max_frame_errors;     /* stop at the frame that reaches this many frame errors (0 = none) */
    int64_t max_frames;           /* stop after this many frames (0 = none); one limit is required */
    int32_t count_mode;           /* FPLDPC_COUNT_* */
    int32_t chunk;                /* frames per launch (0 = auto) */
    int32_t host_threads;         /* channel threads (<= 0 = all) */
    /* optional, called in frame order for every counted frame (e.g. ArrayLDPC_Debug_Shorten
     * prints each decode_fixpoint return value, PerfTest.cpp:419) */
    void (*on_frame)(void *ctx, int64_t frame, int32_t iterations, int64_t blkerror);
    void *on_frame_ctx;
    int32_t device_channel;       /* 1 = generate the LLRs on the device (fpldpc_channel_llr) in the
                                     decoding stream instead of on host threads (default 0) */
    int32_t random_info;          /* 1 = fresh information bits per frame, encoded on the device (default 0) */
    int64_t info_seed;            /* Lehmer state of the information-bit stream (default 987654321) */
} fpldpc_sim_params;

typedef struct {
    int64_t bit_errors, frame_errors, frames, iter_sum; /* over frames [first_frame, first_frame + frames) */
    int64_t frames_decoded;       /* incl. the tail of the last waited chunk past the stop frame */
    double seconds;               /* wall time of the whole simulation */
} fpldpc_sim_result;

void fpldpc_sim_params_default(fpldpc_sim_params *p);
int fpldpc_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out);
/* The same simulation around a layered decoder (all three kinds: unsaturated, saturated with int16 or int32
 * state, min-sum) and around the flooding min-sum decoder, in either placement of the min-sum state: the
 * same chunks, stop rule, FPLDPC_SIM_OVERLAP switch and counters.  The twin is a second object of the same
 * code, parameters, layering, widths, scale, offset and kernel choice (copied from `dec`, not chosen again:
 * the environment switches read at creation are not read here), with its own tables, counter block, scratch
 * (grid * slice bytes in the global placement) and stream: about the decoder's own footprint.  The int32
 * envelope of the unsaturated layered decoder stays the caller's business, as for fpldpc_layered_decode. */
int fpldpc_layered_ber_sim(fpldpc_layered_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out);
int fpldpc_minsum_ber_sim(fpldpc_minsum_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out);

/* A codeword per frame (fpldpc_sim_params.random_info = 1, on every fpldpc_*ber_sim* entry point).  The
 * decoders are not symmetric at zero (a zero posterior or message counts as bit 1), so the error rate of one
 * fixed codeword, the all-zero one above all, is biased by that codeword; with random_info every frame
 * carries fresh information bits.  Per chunk, on the slot's stream: fpldpc_info_bits, the device encoder
 * (derived from the decoder's own code as fpldpc_encoder_from_code does, one per slot), the device channel
 * with a codeword per frame, the decode with its hard output, and a count of each frame's hard decisions at
 * the encoder's info positions against the bits that frame was sent with (FPLDPC_COUNT_ITERS: no count,
 * blkerror is the iteration count as ever).  FPLDPC_ERR_ARG, with a message naming the rule, unless
 * device_channel = 1 (the host channel takes one codeword only), codeword, info_index and info_bits are
 * NULL (the simulation owns them; k is ignored), n_forced = 0 (shortening fixes information bits) and
 * 1 <= info_seed <= 2^31 - 2.  random_info = 0 ignores info_seed and changes nothing.
 *
 * The information-bit stream is public so that anyone can reproduce what was sent.  It is the reference's
 * Lehmer generator (a = 48271, m = 2^31 - 1, fpldpc_rng_skip) started at info_seed, independent of the noise
 * stream: bit i < k of frame f is (fpldpc_rng_skip(info_seed, (uint64_t)f * k + i + 1) >> 30) & 1, the state
 * after draw f*k + i read as "uniform >= 1/2".  out is uint8 [frames][k] for frames [first_frame,
 * first_frame + frames): host memory for fpldpc_info_bits_host; device memory, written asynchronously on
 * `stream` (hipStream_t, NULL = default), for fpldpc_info_bits.  FPLDPC_ERR_ARG unless
 * 1 <= info_seed <= 2^31 - 2, k >= 1, frames >= 0, first_frame >= 0 and (first_frame + frames) * k < 2^48
 * (the device channel's limit on a draw index). */
int fpldpc_info_bits_host(int64_t info_seed, int64_t first_frame, int32_t frames, int32_t k, uint8_t *out);
int fpldpc_info_bits(int64_t info_seed, int64_t first_frame, int32_t frames, int32_t k, uint8_t *out_dev, void *stream);

/* The same simulation over `ndev` decoders (one per device; SURVEY §8e: codeword batches shard
 * across the GPUs of a node), one host thread per decoder.  Frames go out in rounds: in round r
 * decoder i takes frames [first_frame + (r*ndev + i)*chunk, +chunk), so frame f keeps draws
 * [f*n, (f+1)*n) of the one channel stream; after each round the decoders exchange their chunk sums
 * (an all-gather), the one holding the stop frame locates it, and an all-reduce adds the counts.
 * The result equals fpldpc_ber_sim's (same frames, same counters) for any ndev and chunk.
 * Replaces the reference's single-threaded frame loop (PerfTest.cpp:97-135) on a multi-GPU node.
 *   collective: FPLDPC_COLL_RCCL  = RCCL communicators over the decoders' devices (ncclCommInitAll in
 *                                   this process; collectives on each decoder's stream, xGMI on MI355X);
 *                                   the devices must be distinct
 *               FPLDPC_COLL_HOST  = exchange through host memory (decoders may share a device)
 *               FPLDPC_COLL_AUTO  = RCCL when ndev > 1 and the devices are distinct, else host
 *   collective_used (nullable) receives the one that ran (HOST after an AUTO fallback, whose RCCL
 *   error goes to stderr).  Every decoder must be a different object
 *   (each is single-stream) on the same code; on_frame is called in frame order from one thread. */
#define FPLDPC_COLL_AUTO 0
#define FPLDPC_COLL_RCCL 1
#define FPLDPC_COLL_HOST 2
int fpldpc_ber_sim_multi(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                         int32_t collective, fpldpc_sim_result *out, int32_t *collective_used);
/* The same over layered decoders and over flooding min-sum decoders (fpldpc_layered_ber_sim above). */
int fpldpc_layered_ber_sim_multi(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_sim_result *out, int32_t *collective_used);
int fpldpc_minsum_ber_sim_multi(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                int32_t collective, fpldpc_sim_result *out, int32_t *collective_used);

/* ---------------------------------------------------------------- harvest of the failing frames */
/* What a simulation's counters do not say (no reference counterpart): which frames failed, and to what.  For
 * one decoded frame let h be the hard decision (n bits) and c the word the frame was sent with -- the frame's
 * own codeword under random_info, else fpldpc_sim_params.codeword, else all-zero.  Then
 *     e = h XOR c,                          weight = |e|   (wrong bits)
 *     s[k] = parity of h over check k,      unsat  = |s|   (unsatisfied checks; taken on h itself, not on e)
 * and the frame is a codeword error when weight > 0: detected when unsat > 0 as well (the decoder ended
 * outside the code), undetected when unsat = 0 (it ended on another codeword).  (weight, unsat) is the
 * frame's class, the (a, b) of an absorbing-set profile.
 *
 * A harvest of a simulation covers exactly its counted frames, first_frame up to and including the stop
 * frame, in frame order; nothing of a chunk decoded past the stop frame enters it.  It holds
 *   records  one per codeword-error frame, the first max_records of them in frame order (a deterministic
 *            choice): frame (int64), iterations, info_errors (the simulation's blkerror of that frame),
 *            weight, unsat, err uint32[hard_words] (bit v % 32 of word v / 32, bits at or above n zero) and
 *            syn uint32[ceil(m / 32)] (the same packing over checks, bits at or above m zero);
 *   counts   int64[6] = {frames, codeword_errors, detected, undetected, recorded, dropped}, over all counted
 *            frames whatever max_records is; dropped = codeword_errors - recorded;
 *   classes  the distinct (weight, unsat) over all counted codeword-error frames with their frame counts,
 *            sorted by weight, then by unsat; independent of max_records too.
 * A record's frame index is enough to replay it: fpldpc_info_bits (first_frame = frame, frames = 1), the
 * encoder and fpldpc_channel_llr (first_frame = frame, frames = 1) regenerate that frame's LLRs for any decoder.
 * A simulation run on another noise source (fpldpc_ber_sim_source) is replayed with fpldpc_channel_llr_src and that source.
 *
 * Per chunk and on the slot's stream, after the decode (called with its hard output) and before the slot is
 * waited for: the scan kernel below over every frame, an ordered compaction of the codeword-error frames'
 * err / syn rows into a buffer of min(max_records, chunk) records, and asynchronous copies to the host of
 * 8 bytes per frame (weight, unsat) plus that buffer.  No host synchronisation is added.  Counts and classes
 * accumulate on the host, where the stop frame is known. */
typedef struct fpldpc_harvest *fpldpc_harvest_t;
/* Host only, no GPU: copies the code's check lists.  FPLDPC_ERR_ARG unless code != NULL and
 * 0 <= max_records <= 1 << 20. */
int fpldpc_harvest_create(fpldpc_code_t code, int32_t max_records, fpldpc_harvest_t *out);
void fpldpc_harvest_free(fpldpc_harvest_t h);
/* The device primitive, asynchronous on `stream`, device pointers.  For each of `batch` frames: weight[f],
 * unsat[f] and, where non-NULL, err[f][hard_words] and syn[f][syn_words] as defined above.  hard is
 * [batch][hard_words] as fpldpc_decode writes it; bits >= n of the last word are IGNORED, whatever they hold.
 * cw NULL = all-zero, else uint8 [n] (cw_per_frame = 0) or [batch][n] (cw_per_frame = 1), bit in the LSB.
 * Binds to the current device on first use (uploads the check lists), like an encoder.  Touches no record. */
int fpldpc_harvest_scan(fpldpc_harvest_t h, const uint32_t *hard, const uint8_t *cw, int32_t cw_per_frame,
                        int32_t batch, int32_t *weight, int32_t *unsat, uint32_t *err, uint32_t *syn, void *stream);
/* The simulation with a harvest: the _multi signatures plus h; ndev = 1 with FPLDPC_COLL_HOST is the single
 * form.  The fpldpc_sim_result, the on_frame sequence and collective_used are exactly those of the matching
 * *_ber_sim_multi call.  h is cleared when the call starts and filled when it returns FPLDPC_OK; after an
 * error it stays a valid, freeable object with unspecified content.  FPLDPC_ERR_ARG, with a message naming
 * the harvest, if h is NULL, if count_mode != FPLDPC_COUNT_BITS, or if h was made from a code whose n, m or
 * check lists differ from the decoders'; every other rule of fpldpc_sim_params is as before, and so is every
 * mode: host or device channel, all-zero, fixed or per-frame codeword, forced positions,
 * FPLDPC_SIM_OVERLAP=0, several ranks with either collective (each rank uploads the check lists to its own
 * device; one thread appends the ranks' chunks in frame order). */
int fpldpc_ber_sim_harvest(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                           int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used);
int fpldpc_layered_ber_sim_harvest(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                   int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                   int32_t *collective_used);
int fpldpc_minsum_ber_sim_harvest(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used);
/* dims = n, m, hard_words, syn_words */
int fpldpc_harvest_dims(fpldpc_harvest_t h, int32_t dims[4]);
int fpldpc_harvest_counts(fpldpc_harvest_t h, int64_t counts[6]);
/* Copies records [first, first + count); any pointer may be NULL.  FPLDPC_ERR_ARG outside [0, recorded]. */
int fpldpc_harvest_records(fpldpc_harvest_t h, int64_t first, int64_t count, int64_t *frame, int32_t *iters,
                           int32_t *info_errors, int32_t *weight, int32_t *unsat, uint32_t *err, uint32_t *syn);
/* *n_classes receives the number of classes; at most `cap` are copied. */
int fpldpc_harvest_classes(fpldpc_harvest_t h, int32_t *weight, int32_t *unsat, int64_t *count, int32_t cap,
                           int32_t *n_classes);

/* ---------------------------------------------------------------- importance sampling: a shifted mean */
/* What the harvest cannot say (no reference counterpart): how often a structure it found costs a frame at an
 * Eb/N0 where plain simulation sees none.  Mean-shift importance sampling moves the transmitted amplitude on
 * the positions of a suspected structure toward the wrong decision and weights every frame by the likelihood
 * ratio between the true channel and the shifted one.
 *
 * A bias is n, count positions pos[j] (strictly ascending, 0 <= pos[j] < n, 0 <= count <= n) and count finite
 * doubles a[j], the shift in units of the transmitted amplitude: a = 1 moves the mean to zero; negative and
 * zero values are allowed.  For frame f and a position i outside the bias the LLR is fpldpc_channel_llr's, bit
 * for bit.  For i = pos[j], with s = 1 - 2*cw[i], z the Odeh-Evans variate of draw f*n + i and
 * nrm = 0.0 + sigma*z exactly as in that channel,
 *     LLR     = (2*snr) * (s*(1 - a[j]) + nrm)            (each operation rounded once, no contraction)
 *     LLR_fp  = (int)(LLR * 2^frac_bits)                  (I16 / I32 / F64 outputs as the channel's)
 *     term_j  = a[j] * (2*s*nrm - a[j]) / (2*sigma*sigma)
 *     logw[f] = sum_j term_j                              (double; 0.0 exactly when count = 0)
 * The frame's weight w = exp(logw[f]) is the ratio of the true density N(s, sigma^2) to the shifted density
 * N(s(1 - a), sigma^2) at the received values.  sigma is the noise deviation passed in; snr only scales the
 * LLR, as in the channel.
 *   - The reference's variates come from a 31-bit uniform, so |z| is bounded near 6.2: the weight is exact for
 *     the Gaussian the stream approximates, not for its truncation.  The *_src forms below take the source
 *     argument: with FPLDPC_NOISE_PHILOX z is that source's variate at (f, pos[j]), |z| <= 8.58.
 *   - One call carries one bias.  Mixing biases and multiplying by orbit sizes is the caller's arithmetic.
 * Host only, no GPU: copies pos and shift.  FPLDPC_ERR_ARG, with a message naming the rule, for n <= 0,
 * count < 0 or count > n, a position out of range, unsorted or duplicate positions, a non-finite shift. */
typedef struct fpldpc_bias *fpldpc_bias_t;
int fpldpc_bias_create(int32_t n, const int32_t *pos, const double *shift, int32_t count, fpldpc_bias_t *out);
void fpldpc_bias_free(fpldpc_bias_t b);
/* dims = n, count */
int fpldpc_bias_dims(fpldpc_bias_t b, int32_t dims[2]);
/* The shifted channel on the host: fpldpc_channel_llr_host's arguments with n the bias's, cw uint8[n]
 * (cw_per_frame = 0) or uint8[frames][n] (cw_per_frame = 1), NULL = all-zero, and logw double[frames]
 * (may be NULL), term_j summed in ascending j.  The argument rules and the int16 rule (FPLDPC_ERR_ARG if a
 * stored value does not fit, whether the shift put it there or not) are that channel's. */
int fpldpc_bias_channel_llr_host(fpldpc_bias_t b, int64_t seed, int64_t first_frame, int32_t frames, double snr,
                                 double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out,
                                 int32_t out_type, double *logw, int32_t nthreads);
/* The same on the device, asynchronous on `stream`: fpldpc_channel_llr's arguments with n the bias's, every
 * pointer device memory, logw double[frames] (may be NULL).  It is fpldpc_channel_llr followed, on the same
 * stream, by a patch kernel over the biased positions: a wave per frame, each lane summing its term_j in
 * ascending j and the 64 lane sums reduced in a fixed order, so that the same call gives the same logw bits
 * every time (no floating-point atomic); against the host's, logw differs by the summation order and the device
 * libm's log (tests/test_gpu_bias_channel.py: within 1e-12 * (sum_j |term_j| + 1)).  *overflow counts the values
 * actually stored outside int16, as the channel's: where the shifted value overflows and the unshifted one
 * does not, or the other way round, the count follows the stored value.  The bias binds to the current device
 * on first use (uploads positions and shifts), like a harvest. */
int fpldpc_bias_channel_llr(fpldpc_bias_t b, int64_t seed, int64_t first_frame, int32_t frames, double snr,
                            double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame, void *out,
                            int32_t out_type, int32_t *overflow, double *logw, void *stream);
/* The weighted sums of a biased simulation over its counted frames, first_frame up to and including the stop
 * frame, added in frame order with w = exp(logw[f]), blk the frame's blkerror and fe = (blk > 0):
 *     sum_w += w;  sum_w2 += w*w;  sum_w_fe += w*fe;  sum_w2_fe += w*w*fe;  sum_w_be += w*blk
 * and the extremes of logw.  frames, frame_errors and bit_errors are the result's unweighted counts.  The order
 * is the frame order whatever the chunk size and the number of ranks, so the sums depend on neither.
 * sum_w_fe / frames estimates the frame error rate, sum_w_be / (frames * k) the bit error rate. */
typedef struct {
    int64_t frames, frame_errors, bit_errors;
    double sum_w, sum_w2, sum_w_fe, sum_w2_fe, sum_w_be, min_logw, max_logw;
} fpldpc_bias_sums;
/* The simulation on the shifted channel: the _multi signatures plus b and h (h may be NULL: no harvest; else as
 * the *_ber_sim_harvest calls); ndev = 1 with FPLDPC_COLL_HOST is the single form.  Per chunk, on the slot's
 * stream, the patch kernel follows the channel kernel and runs before the forced positions are written; the
 * chunk's logw is copied with the slot's other results.  After the stop decision one thread walks the ranks'
 * chunks in frame order up to and including the stop frame and adds the sums above; a chunk decoded past the
 * stop frame is drained and not added.  The stop rule, the fpldpc_sim_result (frame_errors stays the
 * unweighted count), the on_frame sequence and the harvest keep their definitions, on the shifted channel's
 * LLRs.  It works with random_info, with a fixed codeword and with the all-zero one.  FPLDPC_ERR_ARG, with a
 * message naming the bias, if b is NULL, device_channel != 1, count_mode != FPLDPC_COUNT_BITS, b's n is not
 * the code's, or a forced position is also a biased one; every other rule is as before.  b's sums are zeroed
 * when the call starts and set when it returns FPLDPC_OK. */
int fpldpc_ber_sim_biased(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out, int32_t *collective_used);
int fpldpc_layered_ber_sim_biased(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                  int32_t *collective_used);
int fpldpc_minsum_ber_sim_biased(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                                 int32_t *collective_used);
/* Of the last simulation run with b (all zero before the first). */
int fpldpc_bias_sums_get(fpldpc_bias_t b, fpldpc_bias_sums *out);

/* ---------------------------------------------------------------- the noise source through bias and simulation */
/* The shifted channel on `source` (noise sources, above): the formulas for LLR, term_j and logw are unchanged, z
 * is the source's variate at (f, pos[j]).  FPLDPC_NOISE_LEHMER: exactly fpldpc_bias_channel_llr_host /
 * fpldpc_bias_channel_llr.  FPLDPC_NOISE_PHILOX: that source's argument rules; on the device the Philox channel
 * kernel is followed by a patch kernel of the same form (a wave per frame, a fixed summation order, no
 * floating-point atomic). */
int fpldpc_bias_channel_llr_src_host(fpldpc_bias_t b, int32_t source, int64_t seed, int64_t first_frame, int32_t frames,
                                     double snr, double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame,
                                     void *out, int32_t out_type, double *logw, int32_t nthreads);
int fpldpc_bias_channel_llr_src(fpldpc_bias_t b, int32_t source, int64_t seed, int64_t first_frame, int32_t frames,
                                double snr, double sigma, int32_t frac_bits, const uint8_t *cw, int32_t cw_per_frame,
                                void *out, int32_t out_type, int32_t *overflow, double *logw, void *stream);
/* The simulation on `source`: the *_ber_sim_biased signatures with the source after `collective`; b and h may each
 * be NULL (no bias, no harvest).  sp->seed is read by the source's rule (FPLDPC_NOISE_PHILOX: 0 <= seed < 2^63,
 * first_frame + max_frames < 2^63); every other rule, the result, on_frame, the harvest and the bias sums keep
 * their definitions, in every mode: host or device channel, every codeword mode, forced positions,
 * FPLDPC_SIM_OVERLAP=0, several ranks with either collective.  random_info's information bits stay on their
 * Lehmer generator.  With FPLDPC_NOISE_LEHMER the call equals *_ber_sim_multi (b = h = NULL), *_ber_sim_harvest
 * (b = NULL) or *_ber_sim_biased bit for bit. */
int fpldpc_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp, int32_t collective,
                          int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h, fpldpc_sim_result *out,
                          int32_t *collective_used);
int fpldpc_layered_ber_sim_source(const fpldpc_layered_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                  int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                  fpldpc_sim_result *out, int32_t *collective_used);
int fpldpc_minsum_ber_sim_source(const fpldpc_minsum_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                 int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                 fpldpc_sim_result *out, int32_t *collective_used);

/* ---------------------------------------------------------------- the simulation around the float decoder */
/* fpldpc_ber_sim_source's loop around fpldpc_decode_float (FP_Decoder::decode_general, the reference's floating-point
 * belief propagation) instead of fpldpc_decode: the same rounds, two chunks in flight with a twin of `dec`,
 * FPLDPC_SIM_OVERLAP=0, the ordered stop, counter exchange, on_frame, both count_modes, several ranks with either
 * collective, random_info, the harvest (h) and the bias (b) under their definitions and argument rules; b and h may
 * each be NULL.  fpldpc_float_ber_sim is the second form with ndev = 1, FPLDPC_COLL_HOST, FPLDPC_NOISE_LEHMER and no
 * bias or harvest.  Two things differ:
 *   - the channel writes FPLDPC_LLR_F64, the unquantised double 2*snr*(...) -- host or device channel, either source,
 *     with or without the bias's patch kernel; nothing is quantised, so there is no int16 overflow to count;
 *   - the decode is fpldpc_decode_float with the decoder's max_iter and early_term; as there, frac_bits, width_mask
 *     and precheck of the decoder's parameters do not apply.
 * The fixed-point channel quantises the same double, LLR_fp = (int)(LLR * 2^frac_bits): frame f of a float run is
 * frame f of the fixed run at the same seed, source, snr and sigma, and harvests of the two compare by frame index.
 * Forced positions receive the double forced_llr * 2^-sp->frac_bits, the value whose quantisation at sp->frac_bits is
 * the fixed run's forced_llr, written after the bias's patch as in the fixed run; sp->frac_bits has no other use here.
 * FPLDPC_ERR_UNSUPPORTED with the float decoder's message, before any frame is generated, outside its envelope
 * (n <= 16384, check and variable degrees <= 255; fpldpc_decoder_create bounds n and the check degree more
 * tightly, not the variable degree: a decoder of a code with a variable of degree above 255 meets this refusal).
 * A decoder stays usable both ways: a float simulation and a fixed-point one on the same
 * object, in either order, give each call's own counters.  The twin's float state is made by its first decode, as
 * any decoder's: its tables and its edge scratch, allocated and uploaded synchronously during round 0. */
int fpldpc_float_ber_sim(fpldpc_decoder_t dec, const fpldpc_sim_params *sp, fpldpc_sim_result *out);
int fpldpc_float_ber_sim_source(const fpldpc_decoder_t *decs, int32_t ndev, const fpldpc_sim_params *sp,
                                int32_t collective, int32_t source, fpldpc_bias_t b, fpldpc_harvest_t h,
                                fpldpc_sim_result *out, int32_t *collective_used);

#ifdef __cplusplus
}
#endif
#endif /* FPLDPC_H */
