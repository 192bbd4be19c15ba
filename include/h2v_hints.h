/* h2v_hints.h — point hints for a staged batch, the one-shot calls and the resident accumulator: an extension of the C ABI of
 * include/h2v.h, exported by the same library.
 *
 * Every launch of a staged batch begins with G1Affine::from_bytes for every compressed point of every proof, and each of them pays a
 * square root in Fq: about 320 field products.  The sender of a proof — a prover, a relay, a rank that has verified the shard
 * already — knows both coordinates of every point it sends.  A HINT is the claimed y coordinate of a point, 32 bytes beside the
 * proof.  The encoding fixes y completely (y^2 = x^3 + 3, and the parity of y is the sign flag), so a hint is checked, never trusted:
 * the check is two squarings, one product and a comparison.  A hint that does not check out costs that one point the square root it
 * would have paid anyway.
 *
 * The invariant.  The results of a launch depend on the uploaded proofs, instances and draws only.  The hints, whatever bytes they
 * hold, change its time and nothing else.  "Results": statuses, verdicts, both accumulator points of every group, Guards, records,
 * and everything h2v_batch_finish*, _recheck, _identify and h2v_batch_guards* return.  A batch that is given no hints enqueues exactly
 * the kernels it enqueues without this header.
 *
 * A hint row.  For one proof: Np x 32 bytes, Np = n_points of h2v_ctx_proof_shape.  Entry j is the y coordinate of the j-th compressed
 * point of the proof in BYTE order (h2v_hints_point_offsets, ascending; for a proof of several circuit instances too), as 32
 * little-endian canonical bytes (y < p).  A hint is USED exactly when the point decodes and the hint's 32 bytes equal its canonical y;
 * everything else is a miss: a wrong value, a non-canonical one (y + p), the other root (p - y), and every hint of a point that does
 * not decode.
 *
 * Cost.  Hints add 32 bytes per point to what is sent and uploaded (12 x 32 B beside a 1024 B proof for the headline key).  A sender
 * of bad hints gets the speed of a launch without hints plus the check.  Hints may come from SOME senders only: a proof has a row or
 * none (include/h2v_hint_rows.h).  The points whose hint is not used are collected on the device and their
 * roots are taken together, 64 to a wave, behind the check: a launch pays for the roots it needs, whichever proofs they belong to.
 * (Only a wave of 64 consecutive points ALL of whose hints fail takes its roots where it stands.)
 *
 * Who takes hints.  A staged batch, here; and through include/h2v_hint_rows.h a staged batch row by row (h2v_batch_set_hint_rows), the
 * one-shot calls h2v_verify_batch, _shapes and _keys (h2v_verify_batch_keys_hinted), h2v_verify_batches (h2v_verify_batches_hinted) and
 * the resident accumulator (h2v_accumulator_process_hinted).  Without hints still: the identifying and the seeded one-shot calls (h2v_verify_batch_identify,
 * _keys_identify, _seeded, _seeded_identify), h2v_verify_each, and h2v_batch_upload_launch, whose decompression runs under its own
 * copy.  The calls of include/h2v.h enqueue exactly what they enqueue without this header.
 *
 * Threading.  A batch is used from one thread at a time, as for every h2v_batch_* call; none of the calls here takes a context's
 * lock (the one-shot calls of include/h2v_hint_rows.h do, as their forms without hints).  h2v_hints_from_points touches neither a context nor a device and may be called from any thread at any time;
 * h2v_hints_point_offsets reads the context as h2v_ctx_proof_shape does.  The entry points are not named in the scene table that
 * covers include/h2v.h (tests/thread_scenes.py), and join h2v.h when that table is next revised.  Errors are reported as in h2v.h
 * (h2v_last_error, per thread).
 */
#ifndef H2V_HINTS_H
#define H2V_HINTS_H

#include "h2v.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The byte offsets of the Np compressed points inside a proof of this context's VK (ascending); *n_points is always written.
 * offsets may be NULL (cap 0) to ask for the count.  cap < Np with offsets given: H2V_ERR_BAD_ARGUMENT. */
int h2v_hints_point_offsets(const h2v_ctx* ctx, size_t* offsets, size_t cap, size_t* n_points);

/* Host only, context-free, no device: y32[32 i ..] = the y of G1Affine::from_bytes(points32[32 i ..]) and decoded[i] = 1,
 * or 32 zero bytes and decoded[i] = 0 where from_bytes fails (x >= p, the identity flag 0x80, x^3 + 3 not a square).
 * decoded may be NULL.  What a sender without a GPU uses to make hints. */
int h2v_hints_from_points(const uint8_t* points32, size_t n, uint8_t* y32, uint8_t* decoded);

/* The hints of the batch's current upload, from host memory (n x Np x 32 bytes, copied: the caller's again at return) or from
 * device memory (row i at d_y32 + i * row_stride, row_stride >= 32 Np and a multiple of 16; device -> device on the batch's
 * stream, no host wait; h2v_batch_upload_device's rules for the pointer: memory of the context's device, 16-byte aligned,
 * the bytes read lie inside its allocation).  y32 / d_y32 NULL: the upload's hints are dropped.
 * The batch must be Uploaded and not launched since; n must equal the upload's n.  The hints belong to that upload: every
 * launch of it uses them, the next upload (or an error that leaves the batch empty) drops them.  (The batch keeps them where the
 * canonical y of its points will lie, so from the second launch of an upload on every decodable point's hint is a right one.)
 * H2V_ERR_BAD_ARGUMENT before any device work, the batch untouched: another stage, an upload that has already decompressed
 * its points (h2v_batch_upload_launch), n != the upload's, a bad pointer / stride. */
int h2v_batch_set_hints(h2v_batch* b, size_t n, const uint8_t* y32);
int h2v_batch_set_hints_device(h2v_batch* b, size_t n, const void* d_y32, size_t row_stride);

/* The hints a launch leaves behind, for the next verifier of the same proofs: the canonical y of the points of proofs
 * [first, first + count) of the last launch, rows of Np x 32 bytes; a point that did not decode is 32 zero bytes.
 * Batch Launched or Finished.  The host form waits for the batch's stream; the device form enqueues one copy kernel and
 * waits for nothing (row_stride and pointer rules as above, "written" for "read").  first + count <= n of the upload
 * (H2V_ERR_BAD_ARGUMENT otherwise); count == 0 does nothing. */
int h2v_batch_hints(h2v_batch* b, size_t first, size_t count, uint8_t* y32);
int h2v_batch_hints_device(h2v_batch* b, size_t first, size_t count, void* d_y32, size_t row_stride);

/* Of the last launch (Launched or Finished; waits for the batch's stream): n_points = n x Np; n_hinted = n_points when the
 * launch had hints — after h2v_batch_set_hint_rows (include/h2v_hint_rows.h), Np x (the rows that were not NULL) — else 0; n_missed = the hinted points whose
 * hint was not used (the points of a proof without a row are neither hinted nor missed).  A hint is USED exactly when the point
 * decodes and the hint's 32 bytes equal its canonical y; every other case is a miss (a wrong, non-canonical or
 * other-root hint, and every point that does not decode).  Any pointer may be NULL. */
int h2v_batch_hint_stats(h2v_batch* b, size_t* n_points, size_t* n_hinted, size_t* n_missed);

#ifdef __cplusplus
}
#endif

#endif
