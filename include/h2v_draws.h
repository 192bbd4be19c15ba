/* h2v_draws.h — draws from a seed: an extension of the C ABI of include/h2v.h, exported by the same library.
 *
 * The per-proof draws of a batch (Fr::random of AccumulatorStrategy::process, halo2_verifier/src/poly/kzg/strategy.rs:129) are
 * otherwise made on the host, 32 bytes per proof (h2v_random_scalars).  Here they are the expansion of ONE 32-byte secret seed, so
 * that a batch whose proofs live in device memory, or a batch sharded over GPUs, needs 32 bytes instead of 32 per proof: each
 * holder of the seed expands the indices it needs, where it needs them.
 *
 * The derivation is part of the interface:
 *
 *   draw(seed, i) = LE512( BLAKE2b-512( msg = seed[32] | LE64(i), key = none, personal = "h2v-draws-v1" | 0x00 x 4 ) ) mod r
 *
 * stored as 32 little-endian canonical bytes; i is a 64-bit index; the 40-byte message is one final block, one compression per
 * draw; the 64 digest bytes are reduced as ff::FromUniformBytes<64> reduces them, which is what Fr::random does with 64 random bytes.
 * In Python:
 *   int.from_bytes(hashlib.blake2b(seed + i.to_bytes(8, 'little'), digest_size=64, person=b'h2v-draws-v1').digest(), 'little') % r
 *
 * Security contract.  The draws must be unpredictable to whoever made the proofs, so:
 *   - the seed is 32 bytes from the OS RNG;
 *   - it is chosen independently of the proofs (after they are fixed, or without looking at them);
 *   - it is not revealed to provers before the verdict;
 *   - a canonical scalar from h2v_random_scalars(out, 1) is an acceptable seed for C callers.
 * A zero draw has the probability it has for Fr::random (about 2^-254), and is handled downstream exactly as a zero draw given any
 * other way (h2v_batch_upload, h2v_batch_upload_device).
 *
 * Threading.  The two entry points are context-free: they take no context, no lock and no shared state, and may be called from any
 * number of threads at once (the device form enqueues one kernel on the caller's stream).  They are not named in the scene table
 * that covers include/h2v.h (tests/thread_scenes.py); their own two-thread test (tests/test_gpu_draws_threads.py) stands in for a
 * scene, and they join h2v.h when that table is next revised.  Errors are reported as in h2v.h (h2v_last_error, per thread).
 */
#ifndef H2V_DRAWS_H
#define H2V_DRAWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out32[32 j ..] = draw(seed32, first_index + j), j < n.  Host only, no device.
 * H2V_ERR_BAD_ARGUMENT: seed32 null, out32 null with n > 0, first_index + n beyond 2^64. */
int h2v_draws_expand(const uint8_t seed32[32], uint64_t first_index, size_t n, uint8_t* out32);

/* The most draws one device call expands: one launch of a one-wave workgroup per 16 draws, and a launch holds fewer than 2^32
 * threads, so (2^26 - 1) * 16 draws, 32 GiB of them.  A longer range takes several calls (the index is the caller's to advance). */
#define H2V_DRAWS_DEVICE_MAX 1073741808

/* The same values into device memory, by a kernel enqueued on `stream` (a hipStream_t; NULL = the default stream) of `device`;
 * waits for nothing.  d_out32: device memory of that device, 16-byte aligned, 32*n bytes inside its allocation.  The seed travels
 * in the kernel's arguments: nothing is copied, and seed32 is the caller's again when the call returns.
 * H2V_ERR_BAD_ARGUMENT, before any device work: the refusals above, and a d_out32 that is a host address, off a 16-byte boundary,
 * memory of another device, or too short an allocation for 32*n bytes; n above H2V_DRAWS_DEVICE_MAX. */
int h2v_draws_expand_device(int device, void* stream, const uint8_t seed32[32], uint64_t first_index, size_t n, void* d_out32);

#ifdef __cplusplus
}
#endif

#endif
