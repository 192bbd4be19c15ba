/* h2v.h — C ABI of the MI355X-native Halo2/KZG/SHPLONK batch verifier.
 *
 * The reference (ChainSafe/halo2-verifier, pure Rust, no FFI of its own) exposes the hot path
 * through Rust traits; this header is what an `extern "C"` block on the Rust side binds
 * (INTEGRATION.md shows the shim).  Each entry point cites the reference item it replaces;
 * paths are relative to the reference repository root.
 *
 * Conventions
 *   - All buffers are caller-owned; the library never retains a host pointer past the call
 *     that received it.  No exceptions or panics cross the boundary.
 *   - Return value 0 = OK; negative = error.  -1..-6 mirror plonk::Error
 *     (halo2_verifier/src/plonk/mod.rs:19-32) in declaration order.
 *   - Field elements: 32 bytes little-endian canonical (== ff::PrimeField::to_repr).
 *   - G1 points at this boundary: x | y, 64 bytes canonical, all-zero = identity.
 *   - Proofs, VerifyingKey and ParamsKZG bytes are in the reference's own formats
 *     (VerifyingKey::write  halo2_verifier/src/plonk/vk.rs:41-64;
 *      ParamsKZG::write_custom  halo2_verifier/src/poly/kzg/commitment.rs:142-152).
 *   - serde format codes follow helpers.rs:7-19: 0 Processed, 1 RawBytes, 2 RawBytesUnchecked.
 *   - Threading: a context may be shared between host threads.  Its VK and params are immutable after creation; its compiled plans
 *     are a bounded cache behind a lock of its own, and a plan stays pinned while a batch holds it.  The entry points that run on the
 *     context's stream with its cached workspaces serialise themselves on the context's lock — on the lock of every context they
 *     are given, taken in address order, so that calls over overlapping sets of contexts cannot deadlock.  They are:
 *       h2v_verify_batch, h2v_verify_batch_shapes, h2v_verify_batch_keys, h2v_verify_batch_seeded, h2v_verify_batches,
 *       h2v_verify_each, h2v_verify_batch_identify, h2v_verify_batch_keys_identify, h2v_verify_batch_seeded_identify,
 *       h2v_guard_msm, h2v_msm_g1, h2v_pairing_check, h2v_guards_check_each, h2v_fold_check,
 *       h2v_msm_append_terms, h2v_msm_add_msm, h2v_msm_scale, h2v_msm_terms, h2v_msm_eval_many, h2v_dual_msm_check_many,
 *       h2v_msm_destroy, h2v_accumulator_process, h2v_accumulator_add_msm, h2v_accumulator_add_msms, h2v_ctx_set_tuning.
 *     Some of them take the lock several times in a row — the seeded forms (two MSMs over the seed, its pairing, then the batch) and
 *     the accumulator's add_msm (two MSMs) — so another thread's call may run between their steps; every step is complete in itself.
 *     The tuning call writes under the lock, but launches of staged batches read the setting without it: set it while the context is
 *     idle.  A batch, an accumulator or an MSM object is used by one thread at a time (a batch and an accumulator own a HIP stream and
 *     their device memory); many of them may be in flight on one context, and one accumulator per feeder thread, merged at the end,
 *     is the intended use.  An object may pass from one thread to another between calls.  The text of the last error is per thread.
 */
#ifndef H2V_H
#define H2V_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2V_OK 0
#define H2V_ERR_INVALID_INSTANCES (-1)         /* Error::InvalidInstances          lib.rs:51-55          */
#define H2V_ERR_CONSTRAINT_SYSTEM_FAILURE (-2) /* Error::ConstraintSystemFailure   kzg/strategy.rs:171-175 */
#define H2V_ERR_BOUNDS_FAILURE (-3)            /* Error::BoundsFailure                                     */
#define H2V_ERR_OPENING (-4)                   /* Error::Opening                   lib.rs:420-424        */
#define H2V_ERR_TRANSCRIPT (-5)                /* Error::Transcript                plonk/mod.rs:34-39    */
#define H2V_ERR_INSTANCE_TOO_LARGE (-6)        /* Error::InstanceTooLarge                                  */
#define H2V_ERR_REFERENCE_PANIC (-7)  /* inputs on which the reference panics: zero inverse (vanishing.rs:100, shplonk.rs:215) */
#define H2V_ERR_BAD_ARGUMENT (-16)
#define H2V_ERR_FORMAT (-17)          /* VK / params bytes rejected (io::Error in VerifyingKey::read / ParamsKZG::read_custom) */
#define H2V_ERR_DEVICE (-18)          /* HIP runtime error; h2v_last_error() has the text */
#define H2V_ERR_UNSUPPORTED (-19)

#define H2V_SERDE_PROCESSED 0
#define H2V_SERDE_RAW_BYTES 1
#define H2V_SERDE_RAW_BYTES_UNCHECKED 2

typedef struct h2v_ctx h2v_ctx;
typedef struct h2v_batch h2v_batch;

/* Library / device probe: number of HIP devices visible (0 if none; never fails). */
int h2v_device_count(void);
/* Text of the most recent error on this thread (never NULL). */
const char* h2v_last_error(void);

/* Context = ParamsKZG + VerifyingKey resident on one GPU, plus everything derived from them
 * once per VK (evaluation domain constants, the compiled per-proof program, G2 line
 * coefficients).
 *   replaces: ParamsKZG::read_custom (poly/kzg/commitment.rs:155-207),
 *             VerifyingKey::read (plonk/vk.rs:76-115) -> EvaluationDomain::new (poly/domain.rs:34-140),
 *             G2Prepared::from (poly/kzg/msm.rs:186-187).
 * vk may be NULL (vk_len 0) for a context that only serves h2v_msm_g1 / h2v_pairing_check. */
int h2v_ctx_create(const uint8_t* params, size_t params_len, int params_format,
                   const uint8_t* vk, size_t vk_len, int vk_format,
                   int device, h2v_ctx** out);
/* The two generic parameters of the reference's verify_proof that change what is computed (lib.rs:33-40):
 *   multiopen:  0 = VerifierSHPLONK (poly/kzg/multiopen/shplonk.rs), 1 = VerifierGWC (poly/kzg/multiopen/gwc.rs)
 *   transcript: 0 = Blake2bRead, 1 = Keccak256Read (transcript/mod.rs:104-116)
 * and the length of its `instances: &[&[&[Fr]]]` argument (lib.rs:43,51-55,63):
 *   circuit_instances: how many circuit instances share ONE proof transcript (0 or 1 = one, what every caller inside the reference
 *                      passes).  With M > 1 a proof carries M sets of advice / permutation / lookup / shuffle commitments and
 *                      evaluations in the reference's interleaved order (lib.rs:91-161, 220-253), and every entry point below takes
 *                      n_instance_columns = M x the VK's instance columns, col_lens and instances32 instance-major.
 *                      (Parity for M > 1 is pinned by the repository's two restatements only — oracle/ and oracle/pyref.py,
 *                      the _m2 fixtures under tests/golden — no caller inside the reference passes M > 1.)
 *   struct_size:       sizeof(h2v_options) as the CALLER's header declares it.  The library reads only the fields that lie inside
 *                      it (later fields default to 0), and rejects a value that is not a layout it knows with H2V_ERR_BAD_ARGUMENT:
 *                      a caller built against another revision of this struct gets an error, not another proof layout.
 *   instance_kernel_threshold: debug / test.  0 = the default: instance columns of more than 1024 values in total are summed by the
 *                      wide-instance kernel instead of being unrolled into the per-proof program; n > 0 sets that bound to n - 1
 *                      (1 = every circuit takes the kernel path).
 * h2v_ctx_create == h2v_ctx_create_ex with {sizeof(h2v_options), 0, 0, 1, 0}. */
typedef struct h2v_options { size_t struct_size; int multiopen; int transcript; int circuit_instances; int instance_kernel_threshold; } h2v_options;
#define H2V_OPTIONS_INIT { sizeof(h2v_options), 0, 0, 1, 0 }
#define H2V_ABI_VERSION 4   /* bumped whenever a struct of this header changes layout; h2v_abi_version() returns the library's */
int h2v_abi_version(void);
#define H2V_MULTIOPEN_SHPLONK 0
#define H2V_MULTIOPEN_GWC 1
#define H2V_TRANSCRIPT_BLAKE2B 0
#define H2V_TRANSCRIPT_KECCAK256 1
int h2v_ctx_create_ex(const uint8_t* params, size_t params_len, int params_format,
                      const uint8_t* vk, size_t vk_len, int vk_format,
                      int device, const h2v_options* options, h2v_ctx** out);
/* Debug / test: force the kernel variants that the library otherwise chooses from the shape of a launch (how many proofs, groups,
 * MSM terms it carries).  Every field 0 = automatic, which is what production runs; the library reads no environment variable.
 * The bit-exact suite uses this to put every variant under test at sizes the CPU oracle can follow.  The setting belongs to the
 * context and is read when a launch is enqueued; it is NOT synchronised with launches of other threads (set it while the context is
 * idle).  A NULL pointer restores automatic choice.
 *   frvm_streams        1..4: instruction streams per proof of the Fr program (automatic: 4 up to 341 waves per launch, else 2)
 *   frvm_lds_kb         LDS slice for the program's slots, KB (automatic: 156 / 78 / 36 by launch size)
 *   msm_parts           pieces the accumulators are left in for the pairing (automatic: 6); 1 = whole points (full Horner, whole-point pairing)
 *   msm_global_sort     1: the global counting sort instead of the per-window LDS sort
 *   msm_no_term_split   1: do not cut problems of more than 16 384 terms into sub-problems
 *   msm_window_threads  lanes per window reduction (64, 128, 256; automatic by bucket and window count)
 *   msm_window_wpw      windows per workgroup of the window reduction (1, 2, 4)
 *   msm_window_slots    3: the 20 KB form of the window reduction without the two-bit digit table (automatic: beyond 1024 windows)
 *   pairing_one_stream  1: the single-stream pairing table over split accumulators instead of the two-stream one */
typedef struct h2v_tuning {
    size_t struct_size;
    int frvm_streams, frvm_lds_kb;
    int msm_parts, msm_global_sort, msm_no_term_split, msm_window_threads, msm_window_wpw, msm_window_slots;
    int pairing_one_stream;
} h2v_tuning;
int h2v_ctx_set_tuning(h2v_ctx* ctx, const h2v_tuning* tuning);
/* Destroys the context and everything compiled for it.  Every h2v_batch created on it must have been destroyed before. */
void h2v_ctx_destroy(h2v_ctx* ctx);

/* Re-serialisation of a VerifyingKey / ParamsKZG in another SerdeFormat — host only, no device needed:
 *   replaces: VerifyingKey::read(from_format) followed by VerifyingKey::write / to_bytes(to_format)   (plonk/vk.rs:41-123)
 *             ParamsKZG::read_custom followed by write_custom / to_bytes                               (poly/kzg/commitment.rs:142-224)
 * out == NULL: *out_len receives the size.  Otherwise *out_len holds the capacity on entry and the size on return.
 * layout (VerifyingKey only): the reference's writer emits a lookup / shuffle argument as all first expressions, then all second
 * ones (lookup.rs:36-49, shuffle.rs:70-84), while its reader takes them in pairs (lookup.rs:51-68, shuffle.rs:86-102).  They
 * agree for arguments of one expression pair; for more, the reference's read does not invert its write.
 *   H2V_VK_LAYOUT_WRITER: exactly the bytes VerifyingKey::write produces;
 *   H2V_VK_LAYOUT_READER: the bytes that VerifyingKey::read (and h2v_ctx_create) read back as the SAME key. */
#define H2V_VK_LAYOUT_WRITER 0
#define H2V_VK_LAYOUT_READER 1
int h2v_vk_convert(const uint8_t* vk, size_t vk_len, int from_format, int to_format, int layout, uint8_t* out, size_t* out_len);
int h2v_params_convert(const uint8_t* params, size_t params_len, int from_format, int to_format, uint8_t* out, size_t* out_len);

/* Shape of one proof for this VK (Np points, Ns scalars, T_R right-channel terms). */
int h2v_ctx_proof_shape(const h2v_ctx* ctx, size_t* proof_len, size_t* n_points, size_t* n_scalars,
                        size_t* n_right_terms, size_t* n_instance_columns);

/* sum_i scalars[i] * bases[i] in G1.
 *   replaces: MSMKZG::eval + to_affine (poly/kzg/msm.rs:81-86) == best_multiexp (arithmetic.rs:102-108). */
int h2v_msm_g1(h2v_ctx* ctx, const uint8_t* scalars32, const uint8_t* bases64, size_t n,
               uint8_t out_xy[64], int* out_is_identity);

/* e(left, s_g2) * e(right, -g2) == 1 ?
 *   replaces: DualMSM::check after both channels are evaluated (poly/kzg/msm.rs:185-203). */
int h2v_pairing_check(h2v_ctx* ctx, const uint8_t left_xy[64], const uint8_t right_xy[64], int* ok);
/* n x DualMSM::check, one verdict per Guard: SingleStrategy::process at the trait seam (kzg/strategy.rs:164-176, msm.rs:185-203).
 * The Guards in the formats of h2v_accumulator_process_guards, under its refusals (nothing is written on an error).  guard_ok[i] is the
 * raw bit of e(L_i, s_g2) e(R_i, -g2) == 1 over Guard i's own evaluated channels.  Runs in launches of at most 512 Guards — one pooled
 * MSM over their 2 K problems, one pairing launch over the K pairs, one copy of K verdict words — and serialises on the context's lock. */
int h2v_guards_check_each(h2v_ctx* ctx, size_t n,
                          const size_t* left_counts, const size_t* right_counts,
                          const uint8_t* left_scalars32, const uint8_t* left_bases64,
                          const uint8_t* right_scalars32, const uint8_t* right_bases64,
                          int* guard_ok);

/* N x verify_proof under AccumulatorStrategy, then finalize():
 *   replaces: the loop  s = verify_proof(&params, &vk, s, instances_i, &mut Blake2bRead::init(proof_i))?
 *             followed by s.finalize()   (lib.rs:33-425, poly/kzg/strategy.rs:125-140).
 * proofs[i] / proof_lens[i]: proof byte strings.  Instances: instances32[i] is the concatenation of proof i's instance
 * columns — of all its circuit instances, instance by instance, when the context was created with circuit_instances > 1 —
 * col_lens[c] the number of values in column c (same for every proof of the batch; h2v_verify_batch_shapes lifts that),
 * n_instance_columns must equal circuit_instances x the VK's instance columns (else H2V_ERR_INVALID_INSTANCES, lib.rs:51-55).
 * rand32: the n scalars that AccumulatorStrategy::process draws with Fr::random
 * (kzg/strategy.rs:129), in call order; NULL = draw from the OS RNG.
 * per_proof_status[i]: 0 or the plonk::Error the reference's verify_proof returns for proof i;
 * a failing proof contributes nothing to the accumulator.  (An instance value that is not a canonical
 * field element cannot be expressed in the reference, whose instances are typed Fr; here it is
 * reported as H2V_ERR_INVALID_INSTANCES for that proof.)
 * batch_ok: all statuses OK and the single pairing check passed.
 * out_left_xy / out_right_xy: the two evaluated channels of the final DualMSM (may be NULL). */
int h2v_verify_batch(h2v_ctx* ctx, size_t n,
                     const uint8_t* const* proofs, const size_t* proof_lens,
                     const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                     const uint8_t* rand32,
                     int* per_proof_status, int* batch_ok,
                     uint8_t out_left_xy[64], uint8_t out_right_xy[64]);

/* As h2v_verify_batch, but every proof brings its own instance column lengths — what N independent calls of the reference's
 * verify_proof allow (`instances: &[&[&[Fr]]]` is an argument of each call, lib.rs:33-49).  col_lens_per_proof is
 * [n][n_instance_columns]; instances32[i] is the concatenation of proof i's columns.  Proofs are grouped by shape inside the
 * library (one compiled plan per shape); the multipliers follow call order over the whole batch and ONE pairing closes it, so
 * the result equals n calls of verify_proof on one AccumulatorStrategy followed by finalize().
 * Cost and limits: every distinct shape compiles a plan (host work quadratic in the per-proof program's length, ~10 device uploads)
 * and resizes the workspace, and the shapes are chosen by whoever supplies the proofs — so one call takes at most 64 distinct
 * shapes (H2V_ERR_UNSUPPORTED beyond) and a context keeps at most 32 compiled plans (least recently used out; plans held by a
 * batch object stay). */
int h2v_verify_batch_shapes(h2v_ctx* ctx, size_t n,
                            const uint8_t* const* proofs, const size_t* proof_lens,
                            const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens_per_proof,
                            const uint8_t* rand32,
                            int* per_proof_status, int* batch_ok,
                            uint8_t out_left_xy[64], uint8_t out_right_xy[64]);

/* N x verify_proof on ONE AccumulatorStrategy whose proofs belong to several VerifyingKeys, then finalize(): one pairing.
 *   replaces: the same loop as h2v_verify_batch with a different `vk` per call (lib.rs:33-49 takes params, vk and instances on
 *             every call; kzg/strategy.rs:125-140 only ever sees MSMs), followed by s.finalize().
 * ctxs[k]: a context per key (its own VK and multi-open / transcript / circuit_instances options), every one on the same device and
 * over the same params (g[0], g2 and s_g2 equal; k may differ), no context twice; key_of_proof[i] < n_keys.  Keys no proof uses are
 * allowed.  Any of these violated: H2V_ERR_BAD_ARGUMENT, before any device work.
 * n_instance_columns[k]: must equal context k's instance-column count (else H2V_ERR_INVALID_INSTANCES, as h2v_verify_batch).
 * col_lens: proof by proof in call order, n_instance_columns[key_of_proof[i]] entries each (per-proof shapes allowed).
 * rand32 / per_proof_status / batch_ok / out_*: as h2v_verify_batch, with draws and multipliers in CALL order over all keys: proof i
 * is scaled by the product of the draws of all later proofs, whatever their key.  n == 0 behaves as h2v_verify_batch on ctxs[0].
 * At most 64 distinct (key, instance shape) groups per call (H2V_ERR_UNSUPPORTED beyond).  The call holds every context (and its
 * one-shot scratch batch) for its whole duration, taking them in one global order, so concurrent calls over overlapping sets of
 * contexts do not deadlock. */
int h2v_verify_batch_keys(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n,
                          const uint8_t* const* proofs, const size_t* proof_lens,
                          const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                          const uint8_t* rand32, int* per_proof_status, int* batch_ok,
                          uint8_t out_left_xy[64], uint8_t out_right_xy[64]);

/* As h2v_verify_batch, starting from an existing accumulator instead of an empty one:
 *   replaces: AccumulatorStrategy::with(msm_accumulator) (poly/kzg/strategy.rs:75-78) — the reference's only pause / resume hook —
 *             followed by the same loop of verify_proof calls and finalize().
 * The seed is a DualMSM as the reference holds it: two lists of (scalar, base) terms, left and right channel (either may be empty).
 * Every verify_proof of this call scales the whole accumulator by its fresh draw before its Guard joins (strategy.rs:129), so the
 * seed's terms end up multiplied by the product of all n draws — which is what makes
 *     verify_batch(first half) -> (L, R);  verify_batch_seeded(second half, seed = {(1, L)}, {(1, R)})
 * equal, bit for bit, to ONE verify_batch over both halves with the draws concatenated.
 * Seed scalars: 32-byte canonical; seed bases: 64-byte x | y (all-zero = identity), rejected with H2V_ERR_BAD_ARGUMENT when not
 * on the curve.  out_left_xy / out_right_xy: the evaluated channels of the final DualMSM, seed included. */
int h2v_verify_batch_seeded(h2v_ctx* ctx, size_t n,
                            const uint8_t* const* proofs, const size_t* proof_lens,
                            const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                            const uint8_t* rand32,
                            const uint8_t* seed_left_scalars32, const uint8_t* seed_left_bases64, size_t n_seed_left,
                            const uint8_t* seed_right_scalars32, const uint8_t* seed_right_bases64, size_t n_seed_right,
                            int* per_proof_status, int* batch_ok,
                            uint8_t out_left_xy[64], uint8_t out_right_xy[64]);

/* ---- resident accumulator: an AccumulatorStrategy that lives across calls.  The strategy's DualMSM is two G1 points (L, R) that stay
 * in device memory, both the identity at creation, plus two counters (proofs processed, proofs that failed).  Proofs are fed as they
 * arrive, in any number of h2v_accumulator_process calls over any mix of VerifyingKeys and instance shapes over one SRS, and ONE
 * pairing runs when the caller asks for it.  A process call of n proofs with draws r_0 .. r_{n-1} is n x (scale the accumulator by
 * the draw, add the proof's Guard), kzg/strategy.rs:129-134:
 *     (L, R) <- M (L, R) + sum_i (prod_{j > i} r_j) Guard_i,     M = r_0 r_1 .. r_{n-1}     (a failed proof contributes nothing)
 * so process(A); process(B); finalize() equals, bit for bit, one h2v_verify_batch_keys over A || B with the draws concatenated: the
 * verdict, the per-proof statuses and both accumulator points, for any cut and any number of calls.  No pairing runs, and no
 * accumulator point passes through host memory, before finalize / read.
 * Threading: one accumulator is used from one thread at a time; several accumulators may share a context. */
typedef struct h2v_accumulator h2v_accumulator;
/* An empty accumulator on ctx's device, over ctx's params.  ctx may have been created without a VK; it must outlive the accumulator.
 *   replaces: AccumulatorStrategy::new (poly/kzg/strategy.rs:69-73). */
int h2v_accumulator_create(h2v_ctx* ctx, h2v_accumulator** out);
void h2v_accumulator_destroy(h2v_accumulator* a);
/* n x verify_proof on this strategy.
 *   replaces: the loop  s = verify_proof(&params, &vk_i, s, instances_i, transcript_i)?  (lib.rs:33-49, poly/kzg/strategy.rs:125-136).
 * Takes the arguments of h2v_verify_batch_keys under its rules (contexts distinct, each with a VK, per-proof shapes allowed, at most
 * 64 (key, instance shape) groups per call, rand32 NULL = OS draws); every context must be on the accumulator's device and over its
 * params (g[0], g2 and s_g2 equal).  Every argument check runs before any device work.  per_proof_status[i]: as h2v_verify_batch;
 * all_ok: 1 when every status of THIS call is 0.  n == 0 changes nothing.  A call that returns non-zero leaves the accumulator and the
 * counters exactly as they were: the scaled accumulator goes to a staging record and the accumulator is written by the call's last step.
 * The call holds every context (and its one-shot scratch batch) for its whole duration, taken in one global order. */
int h2v_accumulator_process(h2v_accumulator* a, h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n,
                            const uint8_t* const* proofs, const size_t* proof_lens,
                            const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                            const uint8_t* rand32, int* per_proof_status, int* all_ok);
/* (L, R) += (sum left_scalars[i] left_bases[i], sum right_scalars[i] right_bases[i]), unscaled; on an empty accumulator this starts
 * from an existing DualMSM.
 *   replaces: AccumulatorStrategy::with(msm_accumulator) (poly/kzg/strategy.rs:76-78), DualMSM::add_msm (poly/kzg/msm.rs:179-183).
 * Scalars 32-byte canonical, bases 64-byte x | y on the curve or all-zero (the identity), as the seed of h2v_verify_batch_seeded: a
 * violation is H2V_ERR_BAD_ARGUMENT and changes nothing.  Either list may be empty. */
int h2v_accumulator_add_msm(h2v_accumulator* a,
                            const uint8_t* left_scalars32, const uint8_t* left_bases64, size_t n_left,
                            const uint8_t* right_scalars32, const uint8_t* right_bases64, size_t n_right);
/* n x (scale the accumulator by the draw, add the Guard): AccumulatorStrategy::process at the trait seam, where the reference's own
 * verify_proof runs on the CPU and hands over the Guard it made.
 *   replaces: msm_accumulator.scale(Fr::random) then f(acc) adding the Guard's terms (kzg/strategy.rs:125-136, msm.rs:173-183)
 * Guard i is two term lists: side s has counts_s[i] terms (either may be 0), scalars 32-byte canonical, bases 64-byte x | y with
 * all-zero = the identity (the seed formats of h2v_verify_batch_seeded); the terms of all guards lie back to back, in guard order, in
 * the four flat arrays.  With draws r_0 .. r_{n-1} (rand32; NULL = OS draws; zero draws allowed):
 *     (L, R) <- M (L, R) + sum_i (prod_{j > i} r_j) (sum_t ls_it lb_it, sum_t rs_it rb_it),     M = r_0 r_1 .. r_{n-1}
 * — h2v_accumulator_process with the Guard supplied instead of computed: feeding each proof's Guard equals, bit for bit, process over
 * the same proofs and draws when every status is 0, and equals n x (scale by r_i; add_msm(guard_i)).  n == 0 changes nothing.
 * Counters: n_proofs += n, n_failed unchanged (a Guard exists only where verify_proof succeeded).  Journal: one entry, as process leaves.
 * H2V_ERR_BAD_ARGUMENT, with points, counters and journal exactly as they were: a null array that the counts say is read, n > 2^20,
 * a side's total above 2^24, a draw or scalar that is not canonical, a base that is neither all-zero nor a canonical point on the curve
 * (h2v_last_error names the guard and the side of the first bad term).  A full journal: H2V_ERR_UNSUPPORTED before any device work.
 * No accumulator point and no MSM result passes through host memory; the accumulator is written by the call's last step, after the
 * terms are known to be valid.  The context may have been created without a VK.  The call uses buffers of the accumulator only. */
int h2v_accumulator_process_guards(h2v_accumulator* a, size_t n,
                                   const size_t* left_counts, const size_t* right_counts,
                                   const uint8_t* left_scalars32, const uint8_t* left_bases64,
                                   const uint8_t* right_scalars32, const uint8_t* right_bases64,
                                   const uint8_t* rand32);
/* The G groups of a finished staged batch as G legs, in group order: the staged launch's throughput under this strategy's one pairing.
 *   replaces: per group, msm_accumulator.scale(draw) then the Guard's terms for each of its proofs (kzg/strategy.rs:125-136,
 *   msm.rs:173-183) — with the Guards' sum taken from what the launch left on the device instead of computed again.
 * Group g holds the proofs [first_g, first_g + n_g) with the draws the batch was uploaded with; S_g is its own sum (the two points the
 * launch left for it) and M_g the product of its draws:
 *     (L, R) <- (prod_g M_g) (L, R) + sum_g W_g S_g,     W_g = prod_{f > g} M_f,     n_proofs += n,   n_failed += the non-zero statuses
 * — bit for bit, in everything read / finalize / check_legs return, what h2v_accumulator_process called once per group over that group's
 * proofs and draws leaves, and so ONE h2v_verify_batch (or _keys) over all proofs so far with all draws concatenated.  Zero draws are
 * allowed (M_g = 0 drops everything before it); a proof that failed by status contributes nothing and is counted.
 * b: a batch whose last launch is finished (h2v_batch_finish / _finish_groups has returned), groups equal or unequal, launched with or
 * without its own pairing.  H2V_ERR_BAD_ARGUMENT before any device work, h2v_last_error naming the reason: a null argument; a batch that
 * is not finished; a fold since the launch (h2v_batch_fold_check_enqueue); a shard (a tail of draws longer than the upload); multipliers
 * that are not those of the uploaded draws; a guard-variant upload; a batch on another device, or over other params (g[0], g2, s_g2).
 * A journal with fewer than G free entries: H2V_ERR_UNSUPPORTED before any device work.  Any non-zero return leaves points, counters
 * and journal exactly as they were: the accumulator is written by the call's last enqueued step, the counters and entries follow the
 * one synchronise.  An upload of no proofs changes nothing.  n_proofs_added / n_failed_added (may be NULL): what the call added.
 * The batch is only read: finish_groups, recheck and identify afterwards return what they returned before, and it may be uploaded
 * again at once.  Synchronous like every accumulator call (its stream is idle at return); other batches' launches stay in flight.
 * Journal: G entries in group order, entry g with sum S_g (unscaled), M_g (read back from the device: 32 G bytes with the call's
 * synchronise) and the group's size and non-zero statuses; (L, R) = sum_e W_e sum_e holds as it stands.  check_legs names a failing
 * GROUP and drop_legs takes it out; h2v_batch_identify / h2v_batch_recheck on the still-resident batch name the proofs inside it. */
int h2v_accumulator_process_batch(h2v_accumulator* a, h2v_batch* b, size_t* n_proofs_added, size_t* n_failed_added);
/* The two points as affine bytes (all-zero = identity) and the counters; any pointer but `a` may be NULL. */
int h2v_accumulator_read(h2v_accumulator* a, uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_proofs, size_t* n_failed);
/* ok = the pairing check of (L, R) passes AND no processed proof failed — what batch_ok means for h2v_verify_batch.
 *   replaces: AccumulatorStrategy::finalize (poly/kzg/strategy.rs:138-140).
 * The accumulator is not consumed and not changed: the caller may go on processing, or finalize again. */
int h2v_accumulator_finalize(h2v_accumulator* a, int* ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]);

/* ---- the leg journal of a resident accumulator: find and drop failing legs.  A proof that decodes and passes its transcript but is
 * wrong (a wrong public input, a flipped h2) leaves every status 0 and poisons (L, R) for good; the journal keeps what it takes to
 * say which LEG (one process or add_msm call) did it and to take that leg out again, without feeding the good proofs a second time.
 * Off by default: an accumulator that never begins a journal runs the launches it ran before.  With the journal on the accumulator
 * keeps one entry per successful call that changed it: the call's own sum (l, r) — two Jacobian points in device memory, for process
 * sum_i (prod_{j > i} r_j) Guard_i over the call's proofs alone, what h2v_verify_batch_keys over that leg accumulates; for add_msm
 * the two evaluated sums — M, the product of the call's draws (1 for add_msm; host memory), and the call's proof and failure counts.
 * Entry 0 is the base: the points and counters as they stood when the journal was begun.  At every return
 *     (L, R) = sum_e W_e sum_e,     W_e = prod_{f > e} M_f   over the entries present. */
#define H2V_ACC_JOURNAL_MAX 4096
/* capacity 0: the journal off, its entries forgotten.  capacity in [2, H2V_ACC_JOURNAL_MAX]: a fresh journal of that many entries, the
 * base included, whose base is the current points and counters — on a journaled accumulator a checkpoint, "everything so far is one
 * base".  Any other capacity: H2V_ERR_BAD_ARGUMENT.  The points and counters never change.  A device error leaves the journal off.
 *   serves: AccumulatorStrategy::with(msm_accumulator) (poly/kzg/strategy.rs:76-78) — the base is the DualMSM an accumulation resumes. */
int h2v_accumulator_journal_begin(h2v_accumulator* a, size_t capacity);
/* One pairing check per entry, side by side in one launch: *n_legs = the entries present, the base included (always written; 0 with
 * the journal off); leg_proofs[e] / leg_failed[e] = the entry's counters; leg_pairing_ok[e] = the raw bit of
 * e(l_e, s_g2) e(r_e, -g2) == 1 — for a process entry the pairing of h2v_verify_batch_keys over that leg alone: a leg of good proofs
 * always passes, a leg of n proofs holding a bad one passes with probability <= n / r.  A proof that failed by status contributes
 * nothing to its leg's sum: it shows in leg_failed, not in the bit.  The arrays may be NULL; a non-NULL array with cap < *n_legs is
 * H2V_ERR_BAD_ARGUMENT.  Changes nothing.
 *   serves: AccumulatorStrategy::finalize (poly/kzg/strategy.rs:138-140), DualMSM::check (poly/kzg/msm.rs:185-203), per leg. */
int h2v_accumulator_check_legs(h2v_accumulator* a, size_t cap, size_t* n_legs, size_t* leg_proofs, size_t* leg_failed, int* leg_pairing_ok);
/* Take entries out again: afterwards the points, the counters and the journal are those of an accumulator that was never given the
 * dropped calls, with the same draws for the kept ones; later entries move down.  legs: n_drop distinct entry indices, each below the
 * entry count and none 0 (the base stays) — else, or with the journal off, H2V_ERR_BAD_ARGUMENT before any device work.  n_drop == 0
 * rebuilds the points from the journal.  A call that returns non-zero leaves points, counters and journal as they were.
 *   serves: DualMSM::scale, DualMSM::add_msm (poly/kzg/msm.rs:173-183): (L, R) <- sum over the kept entries of W_e sum_e. */
int h2v_accumulator_drop_legs(h2v_accumulator* a, const size_t* legs, size_t n_drop);

/* ---- merging resident accumulators: ONE pairing for K accumulators (one per feeder thread, per GPU of a node, per process).
 * With draws c_1 .. c_K
 *     (L, R) <- (L, R) + sum_k c_k (L_k, R_k),     n_proofs += sum_k n_proofs_k,     n_failed += sum_k n_failed_k
 * dst itself is not scaled; the sources are neither consumed nor changed, and a source's own journal is not read.  finalize afterwards
 * means what it means now: the pairing passes and no counted proof failed.
 * Soundness.  The check phi(L, R) = e(L, s_g2) e(R, -g2) is a homomorphism from pairs of G1 points into G_T, so the merged accumulator
 * is checked as phi(dst) prod_k phi(src_k)^(c_k).  If one of the factors phi(dst), phi(src_1) .. phi(src_K) is not 1 and the c_k are
 * independent and uniform in F_r (G_T has prime order r), the product is 1 for at most one value of a c_k given the others:
 * probability <= 1 / r (when only phi(dst) != 1 and every source is good the product is phi(dst) != 1, always).  Good accumulators
 * always merge to a good one.  A zero draw would drop its source from the check without a trace, so it is refused.  The draws must be
 * made AFTER the sources are fixed (draws32 NULL = fresh OS draws, the safe form; programmed draws are for tests and for ranks that
 * must agree on them).
 * Journal.  With dst's journal on, every source leaves one entry, in call order: its sum is c_k (L_k, R_k), its M is 1 (as for add_msm)
 * and it carries the source's counters, so (L, R) = sum_e W_e sum_e holds unchanged.  check_legs names a bad source (c_k != 0: the
 * entry's bit is the source's own bit), drop_legs takes the source out again.  A merge that needs more entries than are free is refused
 * as a whole with H2V_ERR_UNSUPPORTED, after the argument checks and before any device work.
 * Refusals, H2V_ERR_BAD_ARGUMENT before any device work: a null argument with n > 0; n above H2V_ACC_MERGE_MAX; a source equal to dst
 * or given twice; a source on another device or over other params (g[0], g2, s_g2); a draw that is not canonical or is zero.  n == 0
 * changes nothing.  A call that returns non-zero leaves points, counters and journal exactly as they were: the accumulator is written
 * by the call's last enqueued step, the counters and entries follow the synchronise.  out_draws32 (n x 32, may be NULL): the draws
 * used, written on success.
 *   serves: DualMSM::scale and DualMSM::add_msm (poly/kzg/msm.rs:173-183) per source, AccumulatorStrategy::with (poly/kzg/strategy.rs:76-78). */
#define H2V_ACC_MERGE_MAX 512   /* sources per call */
int h2v_accumulator_merge(h2v_accumulator* dst, h2v_accumulator* const* srcs, size_t n_src, const uint8_t* draws32, uint8_t* out_draws32);
/* An accumulator as bytes, for a merge on another device or in another process; little-endian:
 *   [u32 magic = H2V_ACC_STATE_MAGIC ("H2VS")][u32 version = 1][u64 n_proofs][u64 n_failed][left x | y (64)][right x | y (64)]
 * the points as h2v_accumulator_read gives them (affine, canonical, all-zero = the identity).  Changes nothing.  A state carries no
 * SRS: the importer CANNOT check that it was accumulated over its own params — that is the caller's to guarantee (compare the params
 * bytes once, as ShardedAccumulator does); a state over another SRS makes the merged pairing fail, it cannot make a bad proof pass.
 *   serves: AccumulatorStrategy::with (poly/kzg/strategy.rs:76-78): a state is a DualMSM handed on. */
#define H2V_ACC_STATE_BYTES 152
#define H2V_ACC_STATE_MAGIC 1398157896   /* 0x53563248 */
#define H2V_ACC_STATE_VERSION 1
int h2v_accumulator_export_state(h2v_accumulator* a, uint8_t out[H2V_ACC_STATE_BYTES]);
/* h2v_accumulator_merge over n exported states (n x H2V_ACC_STATE_BYTES, contiguous): the states' points are lifted into device memory
 * and merged by the very code of h2v_accumulator_merge, under its rules, draws and journal entries included.  Further refusals,
 * H2V_ERR_BAD_ARGUMENT: a state with a wrong magic or version, or with n_failed > n_proofs (host checks, before any device work); a state
 * with a point that is not canonical or not on the curve and is not all-zero (checked on the device, before anything of dst changes).
 *   serves: DualMSM::scale, DualMSM::add_msm (poly/kzg/msm.rs:173-183), AccumulatorStrategy::with (poly/kzg/strategy.rs:76-78). */
int h2v_accumulator_merge_states(h2v_accumulator* dst, const uint8_t* states, size_t n, const uint8_t* draws32, uint8_t* out_draws32);

/* A device-resident MSMKZG: the (scalar, base) terms of the reference's MSM trait (poly/commitment.rs:56-79) as MSMKZG holds them
 * (poly/kzg/msm.rs:17-21), kept on the context's GPU in the form the pooled MSM reads in place.  For term lists that live across calls —
 * a GuardKZG::msm_accumulator to manipulate, an AccumulatorStrategy::with(msm) to resume, the Guards of many proofs combined under the
 * caller's own scheme; the per-proof feeders (h2v_accumulator_process, _process_guards, _process_batch) stay the fast paths.
 *   - An object holds at most 2^24 terms (H2V_ERR_BAD_ARGUMENT beyond).  Scalars 32-byte canonical, bases 64-byte x | y on the curve,
 *     all-zero = the identity.
 *   - Commit rule: a call that returns non-zero leaves every object it was given exactly as it was (length, contents, read-back).
 *   - Every call takes the lock of the objects' contexts, runs on the context's stream with the context's workspaces (an object owns its
 *     two term arrays and nothing else: there may be one per Guard) and returns with that stream idle.  The objects of one call share the
 *     device and the params (g[0], g2, s_g2), else H2V_ERR_BAD_ARGUMENT before any device work.  An object is used from one thread at a
 *     time and is destroyed before its context.
 *   - Evaluation is offered for MANY objects per call (K objects = K problems of one pooled MSM launch, at most 1024 problems or 512
 *     pairs per launch): the reference builds many tiny MSMs, and a launch per tiny object would be a bad trade. */
typedef struct h2v_msm h2v_msm;
/*   replaces: MSMKZG::new (poly/kzg/msm.rs:25-30): no term. */
int h2v_msm_create(h2v_ctx* ctx, h2v_msm** out);
void h2v_msm_destroy(h2v_msm* m);
/* n x MSM::append_term, in order (msm.rs:57-60).  A scalar >= r, or a base that is neither all-zero nor a canonical point on the curve, is
 * H2V_ERR_BAD_ARGUMENT (checked on the device): h2v_last_error names the lowest bad term ("term i"), and the object is unchanged.  n = 0 is
 * a no-op. */
int h2v_msm_append_terms(h2v_msm* m, const uint8_t* scalars32, const uint8_t* bases64, size_t n);
/*   replaces: MSM::add_msm (msm.rs:62-65): dst's terms, then src's, in order; src is not changed.  dst == src is H2V_ERR_BAD_ARGUMENT (the
 * reference's borrow rules forbid it); an empty src is a no-op. */
int h2v_msm_add_msm(h2v_msm* dst, const h2v_msm* src);
/*   replaces: MSM::scale (msm.rs:67-75): scalar_i <- scalar_i * factor mod r for every term, applied at once (h2v_msm_terms afterwards
 * returns the scaled values, as the reference's scalars() does).  A factor >= r is H2V_ERR_BAD_ARGUMENT; 0 is allowed (every scalar
 * becomes 0, the terms stay); an empty object is a no-op. */
int h2v_msm_scale(h2v_msm* m, const uint8_t factor32[32]);
/* The number of terms. */
int h2v_msm_len(const h2v_msm* m, size_t* n);
/*   replaces: MSM::scalars, MSM::bases (msm.rs:88-94) over the terms [first, first + count): count x 32 and count x 64 canonical bytes.
 * Either output may be NULL.  A range outside the object is H2V_ERR_BAD_ARGUMENT; nothing is written on an error. */
int h2v_msm_terms(h2v_msm* m, size_t first, size_t count, uint8_t* scalars32, uint8_t* bases64);
/*   replaces: MSM::eval + to_affine (msm.rs:81-86) for k objects, and MSM::check (msm.rs:77-79): out_is_identity[i].
 * out_xy: k x 64 bytes; an empty object evaluates to the identity (all-zero bytes, flag 1).  Either output may be NULL.  The same object
 * may occur more than once.  Runs in launches of at most 1024 problems, one synchronise each, the MSM reading the objects' own arrays
 * (no copy, no conversion).  Nothing is written on an error. */
int h2v_msm_eval_many(h2v_msm* const* msms, size_t k, uint8_t* out_xy, int* out_is_identity);
/*   replaces: DualMSM::check (msm.rs:185-203) for k pairs (lefts[i], rights[i]): per launch of at most 512 pairs one pooled MSM over the
 * 2 K problems, one pairing launch over the K pairs, one copy of K verdict words.  ok[i] is the raw bit of e(L_i, s_g2) e(R_i, -g2) == 1
 * (two empty channels: 1); out_left_xy / out_right_xy (k x 64 bytes each, either may be NULL) are the evaluated channels.
 * lefts[i] == rights[i] is allowed.  Nothing is written on an error. */
int h2v_dual_msm_check_many(h2v_msm* const* lefts, h2v_msm* const* rights, size_t k,
                            int* ok, uint8_t* out_left_xy, uint8_t* out_right_xy);
/* h2v_accumulator_add_msm with both channels resident: left and right are evaluated in one pooled launch and added unscaled, with the
 * counters, the journal entry and the refusals of h2v_accumulator_add_msm (a full journal: H2V_ERR_UNSUPPORTED before any device work).
 * Either channel may be NULL (empty).  The objects lie on the accumulator's device, over its params.
 *   replaces: AccumulatorStrategy::with(msm_accumulator) (poly/kzg/strategy.rs:76-78), DualMSM::add_msm (poly/kzg/msm.rs:179-183). */
int h2v_accumulator_add_msms(h2v_accumulator* a, h2v_msm* left, h2v_msm* right);

/* N x verify_proof under SingleStrategy (one pairing per proof; poly/kzg/strategy.rs:164-176).
 * per_proof_status[i] = 0, or H2V_ERR_CONSTRAINT_SYSTEM_FAILURE when that proof's pairing fails,
 * or the transcript/opening error. */
int h2v_verify_each(h2v_ctx* ctx, size_t n,
                    const uint8_t* const* proofs, const size_t* proof_lens,
                    const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                    int* per_proof_status);

/* n_batches x h2v_verify_batch in few launches: batch i holds batch_sizes[i] proofs (>= 1, else H2V_ERR_BAD_ARGUMENT), and the proofs,
 * instances and draws of all batches sit back to back in call order (n = the sum of the sizes entries each; one instance shape; rand32
 * NULL = draw from the OS RNG).  per_proof_status[n], batch_ok[n_batches] and out_left_xy / out_right_xy (n_batches x 64 bytes, may
 * be NULL) hold, for batch i, what h2v_verify_batch returns over its slice.  The batches are cut, in call order, into launches of
 * groups of unequal size (h2v_batch_set_group_sizes) of at most 512 batches and 16384 proofs each, and of at most the 1024 MSM
 * sub-problems a launch holds (a batch whose MSM problem exceeds 16384 terms counts for more than two: fewer batches then share its
 * launch — the call never returns h2v_batch_upload's H2V_ERR_UNSUPPORTED for its own cut); a batch above 16384 proofs, or one left
 * alone by these rules, runs as h2v_verify_batch does.  Every argument is checked before any device work. */
int h2v_verify_batches(h2v_ctx* ctx, size_t n_batches, const size_t* batch_sizes,
                       const uint8_t* const* proofs, const size_t* proof_lens,
                       const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                       const uint8_t* rand32,
                       int* per_proof_status, int* batch_ok, uint8_t* out_left_xy, uint8_t* out_right_xy);

/* Which proofs made a batch fail: h2v_verify_batch, plus the proofs that fail the pairing.  batch_ok / out_left_xy / out_right_xy
 * are exactly what h2v_verify_batch returns for the same arguments; per_proof_status[i] is what h2v_verify_each returns for proof i
 * (0, the instance / transcript / opening errors, or H2V_ERR_CONSTRAINT_SYSTEM_FAILURE).  When the batch's pairing passes this costs
 * what h2v_verify_batch costs; otherwise the failing ranges of proofs are re-checked on the batch's resident scalars
 * (h2v_batch_recheck) and cut until single proofs remain.  A proof flagged H2V_ERR_CONSTRAINT_SYSTEM_FAILURE always fails
 * SingleStrategy; a failing proof escapes only with the probability AccumulatorStrategy itself allows (<= n / r).
 * rand32 must hold no zero scalar (H2V_ERR_BAD_ARGUMENT); NULL = draw from the OS RNG.
 * n_range_checks (may be NULL): how many range checks the search ran (0 when the batch passes). */
int h2v_verify_batch_identify(h2v_ctx* ctx, size_t n,
                              const uint8_t* const* proofs, const size_t* proof_lens,
                              const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                              const uint8_t* rand32,
                              int* per_proof_status, int* batch_ok,
                              uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_range_checks);

/* Which proofs made a batch of several VerifyingKeys and instance shapes fail: h2v_verify_batch_keys, plus the proofs that fail the
 * pairing.  Takes the arguments of h2v_verify_batch_keys (same rules for ctxs, key_of_proof, n_instance_columns and col_lens:
 * per-proof shapes allowed); h2v_verify_batch_shapes' case is n_keys = 1 with every key index 0.  batch_ok / out_left_xy /
 * out_right_xy are exactly what h2v_verify_batch_keys returns for the same arguments; per_proof_status[i] is what h2v_verify_each on
 * ctxs[key_of_proof[i]] returns for proof i (0, the instance / transcript / opening errors, or H2V_ERR_CONSTRAINT_SYSTEM_FAILURE).
 * Every (key, shape) group stays resident until the search ends: a key's first group on its context's one-shot batch, its later groups
 * on batches made for the call and destroyed at its end.  The search runs only when the folded pairing itself fails: failing ranges of
 * every group are re-checked together, one set of launches per round over all groups (h2v_batches_recheck), until single proofs remain.
 * rand32 must hold no zero scalar (H2V_ERR_BAD_ARGUMENT before any device work); NULL = draw from the OS RNG.
 * n_range_checks (may be NULL): how many range checks the search ran (0 when the pairing passes).  Nothing is written on an error. */
int h2v_verify_batch_keys_identify(h2v_ctx* const* ctxs, size_t n_keys, const uint32_t* key_of_proof, size_t n,
                                   const uint8_t* const* proofs, const size_t* proof_lens,
                                   const uint8_t* const* instances32, const size_t* n_instance_columns, const size_t* col_lens,
                                   const uint8_t* rand32, int* per_proof_status, int* batch_ok,
                                   uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_range_checks);

/* h2v_verify_batch_seeded, plus the proofs that fail the pairing.  Takes the arguments of h2v_verify_batch_seeded; batch_ok /
 * out_left_xy / out_right_xy are exactly what it returns for them (seed included).  The seed's terms belong to no proof, so it enters
 * no proof's check: per_proof_status[i] is what h2v_verify_each returns for proof i, and seed_ok (may be NULL) is the pairing check
 * of the evaluated seed alone (1 for an empty seed) — batch_ok = 0 with every status 0 and seed_ok = 0 says "the accumulator this call
 * resumed was bad already".  The batch's own record (the sum over this call's proofs, without the seed) is checked on its own, and the
 * search (h2v_batch_identify on that record) runs only when it fails.  rand32 must hold no zero scalar (H2V_ERR_BAD_ARGUMENT before
 * any device work); NULL = draw from the OS RNG.  n_range_checks (may be NULL): how many range checks the search ran.  Nothing is
 * written on an error. */
int h2v_verify_batch_seeded_identify(h2v_ctx* ctx, size_t n,
                                     const uint8_t* const* proofs, const size_t* proof_lens,
                                     const uint8_t* const* instances32, size_t n_instance_columns, const size_t* col_lens,
                                     const uint8_t* rand32,
                                     const uint8_t* seed_left_scalars32, const uint8_t* seed_left_bases64, size_t n_seed_left,
                                     const uint8_t* seed_right_scalars32, const uint8_t* seed_right_bases64, size_t n_seed_right,
                                     int* per_proof_status, int* batch_ok, int* seed_ok,
                                     uint8_t out_left_xy[64], uint8_t out_right_xy[64], size_t* n_range_checks);

/* Debug / parity: the Guard of one proof term by term in the order the reference appends them (shplonk.rs:256-264;
 * gwc.rs:86-132: witness_with_aux, commitment_multi query by query — a commitment opened at several points occurs once per
 * query, each time with that query's own scalar — then (eval_multi, -g)), and the
 * Fiat-Shamir challenges [user challenges.., theta, beta, gamma, y, x, y', v, u] (GWC: [.., x, v, u]).
 * On entry *n_right / *n_left / *n_challenges hold the capacities (in elements). */
int h2v_guard_msm(h2v_ctx* ctx, const uint8_t* proof, size_t proof_len,
                  const uint8_t* instances32, size_t n_instance_columns, const size_t* col_lens,
                  uint8_t* right_scalars32, uint8_t* right_bases64, size_t* n_right,
                  uint8_t* left_scalars32, uint8_t* left_bases64, size_t* n_left,
                  uint8_t* challenges32, size_t* n_challenges);

/* n x Fr::random(OsRng) as AccumulatorStrategy::process draws them (kzg/strategy.rs:129): 64 bytes of OS randomness reduced mod r,
 * 32 canonical bytes each.  What rand32 = NULL makes the entry points above draw internally; a SHARDED batch needs the one stream
 * on every rank (draw on one rank, broadcast, pass each rank its tail: h2v_batch_upload). */
int h2v_random_scalars(uint8_t* out32, size_t n);

/* ---- staged interface: inputs resident in HBM, asynchronous execution on the batch's stream.
 * h2v_verify_batch == upload + launch + finish.  A sharded (multi-GPU) run uses
 * h2v_batch_launch(b, 0) on every rank, exchanges the accumulator records (h2v_batch_export_accumulators),
 * and closes with h2v_batch_fold_check_enqueue (or h2v_fold_check).
 * After an error from h2v_batch_upload, h2v_batch_launch, h2v_batch_upload_launch, h2v_batch_finish(_groups) or
 * h2v_batch_fold_check_enqueue the batch holds nothing: every call that works on an upload or a launch (launch, finish,
 * finish_groups, recheck, identify, export_accumulators, fold_check_enqueue) returns H2V_ERR_BAD_ARGUMENT until an upload succeeds.
 * h2v_batch_set_groups leaves the batch empty in the same way. */
int h2v_batch_create(h2v_ctx* ctx, size_t max_proofs, size_t max_instance_values_per_proof, h2v_batch** out);
void h2v_batch_destroy(h2v_batch* b);
/* Host -> device copy of one shard.  proofs_flat = n * proof_len bytes, instances_flat = n * (sum col_lens) * 32 bytes.
 * rand32_tail: the Fr::random draws of proofs [first_index, total) of the whole (possibly sharded)
 * batch — the multiplier of proof i is the product of the draws of all later proofs
 * (kzg/strategy.rs:129, msm.rs:173-176) — n_tail = total - first_index >= n. NULL = OS RNG (unsharded only). */
int h2v_batch_upload(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len,
                     const uint8_t* instances_flat, size_t n_instance_columns, const size_t* col_lens,
                     const uint8_t* rand32_tail, size_t n_tail);
/* h2v_batch_upload for inputs that are ALREADY in device memory (a shard received over RCCL, a GPU prover's output, a NIC's buffer, a
 * tensor): device -> device, on the batch's stream (its own, or h2v_batch_set_stream's), with no host wait when the draws are given.
 * Row i of the proofs starts at d_proofs + i * proof_stride and only the VK's proof length of it is read (proof_stride >= that
 * length); d_instances has h2v_batch_upload's flat layout; d_rand_tail holds n_tail canonical 32-byte scalars under h2v_batch_upload's
 * tail rules (equal groups, unequal groups with n_tail == n, a shard's tail with n_tail > n).  d_rand_tail NULL = OS draws made on
 * the host and copied: only that form waits for the stream.  col_lens is a host array.
 * Checked on the host before any device work (H2V_ERR_BAD_ARGUMENT, the batch untouched): everything h2v_batch_upload checks without
 * reading an input byte; every pointer is device memory of the context's device, 16-byte aligned, and the bytes read from it lie
 * inside its allocation; proof_stride is a multiple of 16.
 * The caller orders whatever produces the inputs before this call (the same stream, or an event the stream waits for) and leaves the
 * inputs alone until the enqueued work has run: return from h2v_batch_finish(_groups) is sufficient.
 * The DRAWS cannot be seen by the host: a kernel checks them, and its verdict arrives with h2v_batch_finish(_groups).  A draw >= r makes
 * that call return H2V_ERR_BAD_ARGUMENT naming the lowest offending index; it writes nothing and leaves the batch empty.  (The batch's
 * own copy of the tail holds the scalar 1 in place of such a draw: no proof drops out of an accumulator, and ranks of a sharded batch
 * that upload the same tail substitute alike, so a record exported before the finish is never a silent partial sum.)  Zero draws are
 * handled as in h2v_batch_upload; what h2v_batch_recheck and h2v_batch_identify need to know about them is there after the finish. */
int h2v_batch_upload_device(h2v_batch* b, size_t n, const void* d_proofs, size_t proof_stride,
                            const void* d_instances, size_t n_instance_columns, const size_t* col_lens,
                            const void* d_rand_tail, size_t n_tail);
/* Enqueue decompress -> transcript -> Fr program -> fold -> MSM (-> pairing if with_pairing). */
int h2v_batch_launch(h2v_batch* b, int with_pairing);
/* h2v_batch_upload followed by h2v_batch_launch, with most of the host -> device copy HIDDEN behind the first stage: only the point
 * bytes of the proofs (a few runs at fixed offsets: 12 x 32 of 1024 bytes for the headline VK) are copied first, the point
 * decompression is enqueued, and the calling thread copies everything — whole proofs, instances, draws — while the GPU decompresses.
 * Same results as the two calls; returns when the host buffers are the caller's again, with the launch still running
 * (h2v_batch_finish waits for it).  For callers whose proofs arrive from the host for every batch (the C ABI hands over host
 * memory): a single launch has nothing else to hide the PCIe copy behind. */
int h2v_batch_upload_launch(h2v_batch* b, size_t n, const uint8_t* proofs_flat, size_t proof_len,
                            const uint8_t* instances_flat, size_t n_instance_columns, const size_t* col_lens,
                            const uint8_t* rand32_tail, size_t n_tail, int with_pairing);
/* Wait for the launch and fetch results (any pointer may be NULL).  A launch with its own pairing checks runs on the batch's stream
 * from its first kernel to its last (the pairing launch, which writes the verdicts and the rest of the results into pinned host memory
 * itself); a launch of more than 64 groups ends on an internal auxiliary stream as well (the whole accumulators, their bytes, the copy
 * of the result block), and this call waits for both.  So the batch's stream alone going idle does NOT always mean the results are
 * there; every other h2v_batch_* call orders its work behind that auxiliary stream by itself. */
int h2v_batch_finish(h2v_batch* b, int* per_proof_status, int* batch_ok, uint8_t out_left_xy[64], uint8_t out_right_xy[64]);
/* Grouped batches: one upload / launch carries `groups` INDEPENDENT AccumulatorStrategy batches (kzg/strategy.rs:99-141 each):
 * group g owns proofs [g*n/groups, (g+1)*n/groups) and the draws rand32_tail[g*n_tail/groups, (g+1)*n_tail/groups), has its own
 * pair of accumulators and its own pairing check — exactly what `groups` separate h2v_batch objects would compute, but with
 * every kernel launched once for all of them (the pairing and the tail of the MSM are latency-bound single-wave kernels, so G
 * of them side by side cost the time of one).  n and n_tail of later uploads must be multiples of `groups`.  Call before upload. */
int h2v_batch_set_groups(h2v_batch* b, size_t groups);
/* Groups of UNEQUAL size: group g owns the next sizes[g] proofs of later uploads, in order, and the same slice of the draws — exactly
 * h2v_verify_batch over its proofs with its draws, as h2v_batch_set_groups defines a group.  1 <= n_groups <= 512 (half the MSM's
 * problems per launch), every size >= 1 (a zero size is H2V_ERR_BAD_ARGUMENT), the sizes sum to at most max_proofs.  Leaves the batch
 * empty, as h2v_batch_set_groups does; a later h2v_batch_set_groups returns it to equal groups.  An upload then needs n = the sum of
 * the sizes and takes ONE draw per proof (rand32_tail NULL, or n_tail == n).  launch, upload_launch, finish_groups, accumulators,
 * recheck, identify and h2v_batches_recheck work as on equal groups (a range must lie inside one group, found from the sizes);
 * h2v_batch_export_accumulators and h2v_batch_fold_check_enqueue refuse the batch (H2V_ERR_BAD_ARGUMENT): a sharded launch of unequal
 * groups would need a tail of draws per group.  An upload whose MSM problems, cut into sub-problems of at most 16384 terms, would be
 * more than a launch holds (1024) is refused with H2V_ERR_UNSUPPORTED before any device work. */
int h2v_batch_set_group_sizes(h2v_batch* b, const size_t* sizes, size_t n_groups);
/* As h2v_batch_finish for a grouped batch: group_ok[n_groups], out_left_xy / out_right_xy = n_groups x 64 bytes. */
int h2v_batch_finish_groups(h2v_batch* b, int* per_proof_status, int* group_ok, uint8_t* out_left_xy, uint8_t* out_right_xy, size_t n_groups);
/* h2v_batch_finish_groups INTO DEVICE MEMORY, for a consumer that lives on the GPU (a tensor pipeline that masks the rejected proofs, a
 * rank that gathers statuses, a service that queues launches back to back): the results of the last launch are written by kernels on
 * the batch's stream into the caller's device arrays, bit for bit what h2v_batch_finish_groups would write to host arrays for the same
 * launch.  The call waits for nothing — no stream or event synchronise, no blocking copy — and returns once the kernels are enqueued;
 * the caller orders its readers behind the batch's stream (h2v_batch_stream).  Every output pointer may be NULL (not wanted):
 *   d_status        n int32: the per-proof codes (0 or H2V_ERR_*)
 *   d_group_ok      G int32: 0 / 1
 *   d_left_xy, d_right_xy   G x 64 bytes each
 *   d_group_failed  G uint32: the proofs of the group whose status is not 0
 *   d_failed_index  the proofs whose status is not 0, ASCENDING, the first failed_cap of them; nothing is written from position
 *                   failed_cap on (failed_cap is read only with d_failed_index, and 0 is refused)
 *   d_summary       H2V_SUMMARY_WORDS uint32:
 *     [0] 0xffffffff, or the lowest index of a non-canonical draw of an upload that took its draws from device memory
 *         (h2v_batch_upload_device).  With such a fault every group_ok is 0 and [2] is 0; statuses and bytes are what the launch left.
 *     [1] the number of proofs whose status is not 0 (the true count, also above failed_cap)
 *     [2] the number of groups with group_ok = 1        [3] n        [4] G
 *     [5] flags: bit 0 the launch ran its own pairing checks, bit 1 a fold ran since the launch (h2v_batch_fold_check_enqueue)
 *     [6], [7] 0
 * The batch must be launched or finished; its stage does not change, so the call may be repeated, and h2v_batch_finish(_groups) before
 * or after it returns exactly what it returns without it (after a draw fault: the refusal, and the batch left empty).
 * Checked on the host before any device work (H2V_ERR_BAD_ARGUMENT, h2v_last_error names the argument, the batch untouched): the stage;
 * every pointer given is device memory of the context's device, 16-byte aligned, and the bytes written to it lie inside its
 * allocation (d_failed_index: min(failed_cap, n) words). */
#define H2V_SUMMARY_WORDS 8
int h2v_batch_finish_device(h2v_batch* b, void* d_status, void* d_group_ok, void* d_left_xy, void* d_right_xy, void* d_group_failed,
                            void* d_failed_index, size_t failed_cap, void* d_summary);
/* Pairing checks of ranges of the last FINISHED launch of b (h2v_batch_finish / _finish_groups), on its resident per-proof Guard
 * scalars: no stage before the MSM runs again.  Range i = proofs [first[i], first[i] + count[i]); count > 0; every range inside one
 * group of the launch (else H2V_ERR_BAD_ARGUMENT: the last proof of every group has multiplier 1, so a range over two groups could
 * pair up equal multipliers); ranges may overlap.  range_ok[i] = the check of sum over the range of (multiplier_p * Guard_p), proofs
 * with a non-zero status contributing nothing; out_left_xy / out_right_xy (n_ranges x 64 bytes each, may be NULL) the two evaluated
 * channels per range.  A range over a proof whose multiplier is zero (a zero draw behind it in its group) is H2V_ERR_BAD_ARGUMENT: its
 * check would say nothing about that proof.  The launch's own results, and later uploads and launches, are unaffected.  Synchronous. */
int h2v_batch_recheck(h2v_batch* b, size_t n_ranges, const size_t* first, const size_t* count,
                      int* range_ok, uint8_t* out_left_xy, uint8_t* out_right_xy);
/* h2v_batch_recheck over ranges of several batches in ONE set of launches per MSM_MAX_PROBLEMS / 2 ranges: range i = proofs
 * [first[i], first[i] + count[i]) of batches[batch_of_range[i]], under h2v_batch_recheck's rules for that batch (inside one group of its
 * last finished launch, no proof with a zero multiplier, ...); range_ok / out_left_xy / out_right_xy as h2v_batch_recheck.  Every batch
 * must be Finished, on one device and over the same params (g[0], g2 and s_g2 equal; keys and instance shapes may differ); the same
 * batch may appear more than once.  A batch not finished, on another device or over other params, an index out of range or a null
 * pointer: H2V_ERR_BAD_ARGUMENT, and nothing is written.  Synchronous.  The re-checks run on the stream of batches[0] and use its
 * re-check workspace (the one h2v_batch_recheck on batches[0] uses); the other batches' streams are waited for, and only read.  No
 * batch's own results are touched. */
int h2v_batches_recheck(h2v_batch* const* batches, size_t n_batches, size_t n_ranges, const uint32_t* batch_of_range,
                        const size_t* first, const size_t* count, int* range_ok, uint8_t* out_left_xy, uint8_t* out_right_xy);
/* Which proofs of the last FINISHED launch of b fail the pairing — whatever closed it: its own pairing checks, none (a shard), or a
 * later h2v_batch_fold_check_enqueue (a sharded or seeded batch); any group count.
 * Step 1, the groups' own verdicts: group_own_ok[g] (groups entries, may be NULL) = the raw bit of e(L_g, s_g2) e(R_g, -g2) == 1 over
 * group g's OWN accumulators, sum over the group's proofs of multiplier_p * Guard_p — what the launch's pairing says when it ran and
 * no fold followed, otherwise one pairing launch over all groups; no MSM runs.  A group of good proofs always passes; a group of
 * count proofs holding a bad one passes with probability <= count / r (its sum is a random linear combination with distinct
 * monomials in the draws), whatever other shards or a seed add to the batch's final verdict.
 * own_records: the device address of the groups x H2V_ACC_RECORD_BYTES records h2v_batch_export_accumulators wrote for THIS launch, or
 * NULL when the batch's resident accumulators are still its own.  A fold overwrites them: NULL after a fold is
 * H2V_ERR_BAD_ARGUMENT.  A record whose piece count is outside 1 .. H2V_ACC_RECORD_PIECES, or whose failure count differs from the
 * group's number of non-zero statuses, is H2V_ERR_BAD_ARGUMENT.
 * Step 2: the groups whose own check fails are searched together, as h2v_verify_batch_keys_identify searches its batches: failing
 * ranges are re-checked on the resident scalars (h2v_batch_recheck) and cut until single proofs remain.
 * per_proof_status[i] (n entries, may be NULL): the launch's status for proof i, and H2V_ERR_CONSTRAINT_SYSTEM_FAILURE for the proofs
 * with status 0 whose own check fails — what h2v_verify_each returns.  n_range_checks (may be NULL): the ranges handed to re-check
 * launches (the pairing of step 1 not counted; 0 when every group passes).
 * H2V_ERR_BAD_ARGUMENT, before any device work, when a proof of the batch has a zero multiplier (a zero draw behind it in its
 * group's uploaded draws: h2v_batch_recheck's rule), or when the batch is not finished.  The launch's results, its accumulators and
 * its workspace are untouched (h2v_batch_finish_groups afterwards returns what it returned before), and a call that returns
 * non-zero writes nothing.  Synchronous. */
int h2v_batch_identify(h2v_batch* b, const void* own_records, int* per_proof_status, int* group_own_ok, size_t* n_range_checks);
/* Device address of this batch's accumulator points after launch: per group [left, right], 2 x 108 bytes each, Jacobian
 * (X, Y, Z) in the library's Montgomery limb layout (debug / inspection; the record a sharded run exchanges is written by
 * h2v_batch_export_accumulators). */
int h2v_batch_accumulators(h2v_batch* b, void** device_ptr, size_t* nbytes);
/* What a shard contributes to a sharded batch, per group — opaque bytes to be moved by a collective (all-gather):
 *   [u32 failed][u32 parts][u32 shift][u32 0][left piece 0 .. 5][right piece 0 .. 5]      (a piece: 108 B, Jacobian X, Y, Z)
 * `failed` = number of this shard's proofs with a non-zero status.  It matters: a failed proof is zeroed out of its shard's
 * accumulators, so the folded pairing alone would accept a batch in which another shard rejected a proof;
 * h2v_batch_fold_check_enqueue / h2v_fold_check clear `ok` when any folded record reports failures, so every rank reaches the same
 * verdict without a second collective.
 * The accumulators travel the way a launch leaves them — in `parts` pieces, accumulator = sum_j 2^(shift j) piece_j — because the
 * folded pairing takes them in pieces too (the doublings move to precomputed multiples of the two G2 points; the whole point would
 * cost ~120 dependent doublings on every rank before AND the slower pairing after the exchange).  parts = 1, shift = 0 is a whole
 * point.  Records of ranks whose launches chose another (parts, shift) — shards of very different size — are folded correctly all
 * the same (their pieces are put together first, and join the fold's piece 0).
 * A malformed record never vanishes from a fold: one whose `parts` is outside 1 .. H2V_ACC_RECORD_PIECES — a record that was never
 * written, all zero, is one — or that is cut differently from the fold and asks for more than 256 doublings, shift * (parts - 1) > 256
 * (a launch exports at most 128), contributes the identity and counts as max(failed, 1) failed proofs, so the fold's group cannot be
 * ok.  The folded failure count saturates at 2^32 - 1 instead of wrapping. */
#define H2V_ACC_RECORD_PIECES 6
#define H2V_ACC_RECORD_BYTES 1312   /* 16 + 2 * H2V_ACC_RECORD_PIECES * 108 */
/* The HIP stream (hipStream_t) the batch runs on, for event timing and stream-ordered interop. */
void* h2v_batch_stream(h2v_batch* b);
/* Run the batch on a caller-owned stream (e.g. a torch.cuda.Stream's cuda_stream) instead of its own,
 * so that collectives issued by the caller on that stream are ordered with the batch's kernels without
 * host synchronisation.  The caller keeps the stream alive while the batch uses it. */
int h2v_batch_set_stream(h2v_batch* b, void* hip_stream);
/* Stream-ordered write of the batch's accumulator records (groups x H2V_ACC_RECORD_BYTES) into caller device memory. */
int h2v_batch_export_accumulators(h2v_batch* b, void* device_dst);
/* Stream-ordered version of h2v_fold_check on the batch's stream: fold n_parts gathered accumulator
 * sets (each laid out as h2v_batch_export_accumulators writes it: [group][left, right]) group by group and enqueue one
 * pairing per group; the result is fetched by h2v_batch_finish / h2v_batch_finish_groups (ok, left, right): a group is ok
 * when its pairing passes, its local proofs are all ok AND no folded record reports a failed proof. */
int h2v_batch_fold_check_enqueue(h2v_batch* b, const void* device_accumulators, size_t n_parts);
/* Fold n_parts accumulator records (as written by h2v_batch_export_accumulators for an ungrouped batch, contiguous in
 * device memory) with G1 additions and run the single pairing check; ok = pairing passed and no record reports a failed proof.
 *   replaces: DualMSM::add_msm + check across shards (poly/kzg/msm.rs:178-203). */
int h2v_fold_check(h2v_ctx* ctx, const void* device_accumulators, size_t n_parts, int* ok,
                   uint8_t out_left_xy[64], uint8_t out_right_xy[64]);
/* Per-stage device time of the last finished launch, milliseconds, measured with HIP events on
 * the batch's stream: [decompress, transcript, fr_program, fold, msm, pairing, msm_accumulate (the dominant kernel
 * inside the msm stage)]; returns the number of entries written (<= cap).  Entries the profiling level does not record are 0. */
int h2v_batch_timings(h2v_batch* b, float* ms, int cap);
/* level 0: off; 1 (or any other non-zero value): an event between the stages and around the dominant kernel — every event is a
 * barrier packet on the stream, ~6 us of idle time each, ~0.06 ms per launch; H2V_PROFILE_KERNEL: only the dominant kernel's own
 * start / stop timestamps (attached to its dispatch, no extra packet). */
#define H2V_PROFILE_KERNEL 3
int h2v_batch_set_profiling(h2v_batch* b, int level);

#ifdef __cplusplus
}
#endif
#endif /* H2V_H */
