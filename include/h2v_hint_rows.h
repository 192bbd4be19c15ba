/* h2v_hint_rows.h — point hints from SOME senders: a hint row per proof, or none, for a staged batch, the one-shot calls and the
 * resident accumulator.  An extension of include/h2v_hints.h (what a hint and a hint row are, when a hint is used, and the invariant:
 * hints change a launch's time and nothing else), exported by the same library.
 *
 * A service that batches proofs from many senders gets hints from some of them.  Here a proof has a row or a NULL.  The points whose
 * hint is not used — a sender gave none, or gave a wrong one — are collected on the device and their roots are taken together, 64 to a
 * wave, behind the check, so a launch pays for the roots it needs, whichever proofs they belong to.
 *
 * Threading.  h2v_batch_set_hint_rows: a batch is used from one thread at a time, no context lock, as every h2v_batch_* call.  The
 * three _hinted calls take the locks their forms without hints take (include/h2v.h, "Threading"), for the whole call.
 */
#ifndef H2V_HINT_ROWS_H
#define H2V_HINT_ROWS_H

#include "h2v_hints.h"

#ifdef __cplusplus
extern "C" {
#endif

/* h2v_batch_set_hints from a row per proof, or none: rows[i] is proof i's Np x 32 bytes, or NULL where its sender gave none.  A proof without
 * a row is staged as a zero row, whose hints all miss (no point of the curve has y = 0).  rows NULL: the upload's hints are dropped;
 * an array of n NULLs does the same.  Otherwise h2v_batch_set_hints's rules, word for word: Uploaded and not launched since, n the
 * upload's, the rows copied and the caller's again at return, H2V_ERR_BAD_ARGUMENT before any device work.  h2v_batch_hint_stats of
 * the launch: n_hinted = Np x (the rows that were not NULL), n_missed = the hints of those rows that were not used.  (A second launch
 * of the same upload finds the canonical y of ALL its points where the rows lay, as after h2v_batch_set_hints, and counts every
 * point as hinted.) */
int h2v_batch_set_hint_rows(h2v_batch* b, size_t n, const uint8_t* const* rows);

/* The one-shot calls and the resident accumulator with hints.  Each is its unhinted form (include/h2v.h: h2v_verify_batch_keys,
 * h2v_verify_batches, h2v_accumulator_process — every rule, refusal and result of it) plus two arguments:
 *   hint_rows   after proof_lens: n entries, proof i's row of Np x 32 bytes — Np of THAT proof's context, keys differ in it — or NULL
 *               for a proof without hints.  hint_rows NULL: the call IS the unhinted one.
 *   hint_stats  last, may be NULL: [0] the points of the call's proofs, [1] the hinted ones among them, [2] the hinted ones whose hint
 *               was not used, summed over the call's launches (h2v_batch_hint_stats of each).  Written when the call returns 0.
 * A proof shorter than its key's proof is refused on the host as ever (its packed copy is 0xff bytes, no point of it decodes): its
 * row is not read and it counts as a proof without one.  One context and key_of_proof all zero make h2v_verify_batch_keys_hinted
 * the hinted h2v_verify_batch (one shape) or h2v_verify_batch_shapes (several). */
int h2v_verify_batch_keys_hinted(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs, const size_t* proof_lens,
                                 const uint8_t* const* hint_rows, const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                                 const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t hint_stats[3]);
int h2v_verify_batches_hinted(h2v_ctx* ctx, size_t n_batches, const size_t* batch_sizes, const uint8_t* const* proofs, const size_t* proof_lens,
                              const uint8_t* const* hint_rows, const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                              const uint8_t* rand32, int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, size_t hint_stats[3]);
int h2v_accumulator_process_hinted(h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n, const uint8_t* const* proofs,
                                   const size_t* proof_lens, const uint8_t* const* hint_rows, const uint8_t* const* instances32, const size_t* n_instance_columns,
                                   const size_t* col_lens, const uint8_t* rand32, int* per_proof_status, int* all_ok, size_t hint_stats[3]);

#ifdef __cplusplus
}
#endif

#endif
