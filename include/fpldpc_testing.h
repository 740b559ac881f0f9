/* fpldpc_testing.h -- test-only entry points of libfpldpc.so.
 *
 * NOT part of the drop-in interface (include/fpldpc.h) and with no reference counterpart: fault
 * injection for the tests of the multi-decoder simulation (fpldpc_ber_sim_multi), set explicitly by
 * a test program through this call.  Nothing in the library reads them from the environment, so a
 * production run is never affected unless it calls this function. */
#ifndef FPLDPC_TESTING_H
#define FPLDPC_TESTING_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Process-wide, for the next fpldpc_ber_sim_multi calls until reset (fail_rank = -1, fail_comm_init = 0):
 *   fail_rank >= 0   rank `fail_rank` fails in round `fail_round` as a device error would -- reported
 *                    through the round's all-gather, or with abrupt != 0 by leaving the loop before it
 *                    (every other rank must stop either way, not hang);
 *   fail_comm_init   1: the RCCL communicator set-up fails as if ncclCommInitAll had returned an
 *                    error (FPLDPC_COLL_RCCL: the call fails; FPLDPC_COLL_AUTO: host exchange, reported
 *                    in collective_used); 2: the same, and FPLDPC_COLL_AUTO with a single decoder
 *                    attempts RCCL too (it would not), so the AUTO fallback runs on a one-GPU box. */
void fpldpc_testing_sim_inject(int32_t fail_rank, int64_t fail_round, int32_t abrupt, int32_t fail_comm_init);

/* The int16 range parameters the kernel choice derives for a code whose largest variable degree is
 * dv_max at Constant C (no device needed): returns cmax, the largest c2v magnitude the packed kernels
 * accept (0: none), and in *chain_guard whether an array check of `slots` = (P+1)/2 fold steps takes
 * the range guard from two chain values (G = slots * C <= (cmax + 1) / 8) rather than per output. */
uint32_t fpldpc_testing_range_guard(int32_t dv_max, int32_t C, int32_t slots, int32_t *chain_guard);

/* The number of frames that the last completed fpldpc_decode call of `decoder` (an fpldpc_decoder_t)
 * ended by the packed array kernel's stationary exit: frames whose check-to-variable messages were
 * the same after two consecutive updates, reported with max_iter iterations and the outputs max_iter
 * updates give.  0 for a decoder whose kernel has no such exit, or with FPLDPC_STATIONARY_EXIT=0 in
 * the environment at its creation.  Returns an fpldpc status. */
int fpldpc_testing_stationary_exits(void *decoder, int32_t *count);

/* The number of frames that the last completed fpldpc_decode call of `decoder` ended by the same kernel's
 * cycle exit: frames whose check-to-variable messages, while the frame ran alone in the tail's split
 * form, equalled those of 2 to 8 updates earlier, reported with max_iter iterations and the outputs
 * max_iter updates give.  0 for a decoder whose kernel has no such exit, or with FPLDPC_CYCLE_EXIT=0,
 * FPLDPC_STATIONARY_EXIT=0 or FPLDPC_SPLIT_TAIL=0 in the environment at its creation.  Returns an fpldpc
 * status. */
int fpldpc_testing_cycle_exits(void *decoder, int32_t *count);

/* Which kernel fpldpc_decode_float launches for `decoder` (an fpldpc_decoder_t), its persistent grid and
 * the planes of its edge scratch, written to buf (at most len bytes) as one of
 *   bp_float_reg<DC=47,regular,array> grid=N planes=1    regular degree 47, variable indices computed
 *   bp_float_reg<DC=47,regular,table> grid=N planes=1    regular degree 47, indices from the table
 *   bp_float_reg<DC=8,predicated,table> grid=N planes=1  check degrees 2..8
 *   bp_float_kernel grid=N planes=2                      every other code
 * The form is the name the HIP runtime gives the function the decoder launches, not a second statement
 * of the choice.  A decoder that has not decoded yet builds its float tables first, by decoding one
 * all-zero frame (FPLDPC_FLOAT_WG_PER_CU is read then).  Returns an fpldpc status. */
int fpldpc_testing_float_describe(void *decoder, char *buf, int32_t len);

/* The ordered compaction a harvesting simulation runs per chunk (include/fpldpc.h), on its own so that it can
 * be tested and timed: rows [batch][row_words] of the frames with weight[f] > 0 go, in frame order, to
 * rec [cap][row_words]; codeword-error frames beyond the first `cap` are left out, and records past the last
 * one are not written.  pos [batch] is scratch (it receives each frame's record index, or -1).  Device
 * pointers, asynchronous on `stream`.  Returns an fpldpc status. */
int fpldpc_testing_harvest_compact(const int32_t *weight, const uint32_t *rows, int32_t row_words, int32_t batch,
                                   int32_t cap, int32_t *pos, uint32_t *rec, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPLDPC_TESTING_H */
