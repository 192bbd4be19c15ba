/* h2v_guards.h — every proof's Guard out of a launched staged batch: an extension of the C ABI of include/h2v.h, exported by the
 * same library.
 *
 * The reference's verify_proof returns a GuardKZG: two term lists (the DualMSM's left and right channel) that the caller's own
 * VerificationStrategy then scales, accumulates or checks (halo2_verifier/src/poly/kzg/strategy.rs).  A staged batch (h2v_batch_*) runs
 * verify_proof for all its proofs in one launch and leaves every proof's scalars and points resident; the entry points here gather them
 * into term lists, for any range of the upload, by one kernel (k_guards_gather) — into device arrays, into host arrays, or behind the
 * end of two resident h2v_msm objects.
 *
 * What a Guard of a batch is.  T_L and T_R (h2v_batch_guard_shape) are the term counts of the left and the right channel, the same
 * for every proof of an upload.  Proof p's term t is (scalar, base) in the plan's order; the scalar is the value the launch left
 * resident: the Guard's own scalar times mult[p], the product of the draws behind p inside its group.  Proof p's terms are thus what
 * the reference's msm_accumulator holds for that proof once its whole group has been `process`ed (kzg/strategy.rs:129,
 * kzg/msm.rs:173-183): per group, the MSM over the group's terms is the accumulator h2v_batch_finish_groups reports.  With unit draws
 * (every draw 1) the terms are the raw GuardKZG of every proof.
 *   SHPLONK: order and scalars are the reference's, term for term (multiopen/shplonk.rs:256-264).
 *   GWC:     a commitment opened at several points occurs ONCE, at its first appearance, with its scalars summed: the merged order
 *            of the plan's MSM.  It is sum-equal to the reference's per-query list (gwc.rs:86-132) — every base carries the sum of
 *            the scalars the reference gives it — not term for term.  h2v_guard_msm keeps returning the per-query list.
 *   A proof whose status is non-zero has no Guard in the reference; here every one of its terms is the zero scalar under the
 *   all-zero (identity) base, so that lengths never depend on the data and a consumer's MSM stays defined.  The status says which
 *   proofs these are.  A proof with a zero multiplier (a zero draw behind it in its group) has zero scalars under its own bases.
 *
 * Formats.  Scalars: 32 canonical little-endian bytes.  Bases: 64 bytes x | y, canonical little-endian, the identity all-zero.
 * Term t of proof first + j lies at index j * T + t of a channel's arrays.  mult: 32 canonical bytes per proof.  status: one int per
 * proof, the codes h2v_batch_finish reports before the pairing (0, H2V_ERR_TRANSCRIPT, ...).
 *
 * Common rules.  The batch must be launched (h2v_batch_launch) or finished; the calls leave its stage alone, may be repeated with the
 * same result, and change nothing that h2v_batch_finish, _finish_groups, _finish_device, _recheck or _identify report before or
 * after.  first + count <= n of the upload; count == 0 does nothing; a range may cross group boundaries.  One call gathers fewer than
 * 2^31 terms per channel (H2V_ERR_UNSUPPORTED beyond: take the range in pieces).  H2V_ERR_BAD_ARGUMENT, before any device work and
 * with the batch untouched: a batch with nothing launched, a guard-variant upload (h2v_guard_msm), a range outside the upload.
 *
 * Draws uploaded from device memory (h2v_batch_upload_device).  A draw >= r there is found by a kernel and reported by
 * h2v_batch_finish(_groups), which refuses the launch, and by h2v_batch_finish_device's summary.  h2v_batch_guards and
 * h2v_batch_guards_append wait for the batch's stream and refuse such a launch in the same words (H2V_ERR_BAD_ARGUMENT, nothing
 * written, the objects unchanged, the batch left to its finish).  h2v_batch_guards_device waits for nothing and cannot know: its
 * arrays then hold terms computed with the scalar 1 in that draw's place, and are to be used only with a finish that accepted the
 * launch.
 *
 * Threading.  A batch is used from one thread at a time, as for every h2v_batch_* call; h2v_batch_guards_append also takes the lock
 * of the objects' context(s), like every h2v_msm_* call.  The entry points are not named in the scene table that covers
 * include/h2v.h (tests/thread_scenes.py), and join h2v.h when that table is next revised.  Errors are reported as in h2v.h
 * (h2v_last_error, per thread).
 */
#ifndef H2V_GUARDS_H
#define H2V_GUARDS_H

#include "h2v.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The term counts of a proof's two channels under the plan of the batch's upload.  Valid from a successful upload on.
 * Either output may be NULL. */
int h2v_batch_guard_shape(const h2v_batch* b, size_t* n_left_terms, size_t* n_right_terms);

/* The Guards of proofs [first, first + count) into the caller's device arrays, by kernels on the batch's stream; waits for nothing
 * (no synchronise, no copy): the caller orders its readers behind the batch's stream.  Every output may be NULL = not wanted:
 *   d_left_scalars32  32 * count * T_L bytes     d_left_bases64   64 * count * T_L bytes
 *   d_right_scalars32 32 * count * T_R bytes     d_right_bases64  64 * count * T_R bytes
 *   d_mult32          32 * count bytes           d_status         count ints
 * Each pointer given: device memory of the batch's device, 16-byte aligned, with the bytes the call writes inside its allocation
 * (H2V_ERR_BAD_ARGUMENT otherwise, before any device work). */
int h2v_batch_guards_device(h2v_batch* b, size_t first, size_t count, void* d_left_scalars32, void* d_left_bases64, void* d_right_scalars32,
                            void* d_right_bases64, void* d_mult32, void* d_status);

/* The same into host arrays of the same sizes (every output may be NULL): the kernels write into scratch of the batch's own, one copy
 * and one synchronise of the batch's stream follow.  Nothing is written on an error. */
int h2v_batch_guards(h2v_batch* b, size_t first, size_t count, uint8_t* left_scalars32, uint8_t* left_bases64, uint8_t* right_scalars32,
                     uint8_t* right_bases64, uint8_t* mult32, int* per_proof_status);

/* The count * T_L left terms behind the end of `left` and the count * T_R right terms behind the end of `right` (resident h2v_msm
 * objects; either may be NULL), in the objects' own form: no bytes in between.  *n_failed (may be NULL) = the proofs of the range
 * with a non-zero status (their terms are zero terms on the identity).  The objects keep their commit rule: they grow first, and
 * their lengths change only when the call succeeds, both or neither.  The call returns with the batch's stream idle.
 * H2V_ERR_BAD_ARGUMENT before any device work: an object that would hold more than 2^24 terms, an object on another device or over
 * other params (g[0], g2, s_g2) than the batch's context, left == right. */
int h2v_batch_guards_append(h2v_batch* b, size_t first, size_t count, h2v_msm* left, h2v_msm* right, size_t* n_failed);

#ifdef __cplusplus
}
#endif

#endif
