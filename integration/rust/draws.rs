//! `extern "C"` binding of include/h2v_draws.h — draws from a seed — for the halo2_verifier crate (feature "mi355x").
//! UNCOMPILED in this repository, as ffi.rs is: the build image has no Rust toolchain.  The tested callers of the same two entry
//! points are halo2_verifier_amd/draws.py (ctypes) and include/h2v_draws.hpp; tests/test_draws_host.py checks that both functions
//! the header declares are bound here.  ffi.rs stays the binding of include/h2v.h alone.
//!
//!   draw(seed, i) = LE512(BLAKE2b-512(seed | LE64(i), digest 64, no key, personal "h2v-draws-v1")) mod r, 32 canonical bytes
//!
//! The seed is 32 bytes from the OS RNG, chosen independently of the proofs and not revealed to provers before the verdict.  Both
//! entry points are context-free: no context, no lock, any number of threads.
use core::ffi::{c_int, c_void};

/// the most draws one `h2v_draws_expand_device` call expands (one launch stays below 2^32 threads); longer ranges take several calls
pub const H2V_DRAWS_DEVICE_MAX: usize = 1073741808;

extern "C" {
    pub fn h2v_draws_expand(seed32: *const u8, first_index: u64, n: usize, out32: *mut u8) -> c_int;
    pub fn h2v_draws_expand_device(device: c_int, stream: *mut c_void, seed32: *const u8, first_index: u64, n: usize, d_out32: *mut c_void) -> c_int;
}

/// A fresh seed from the OS RNG.
pub fn new_seed() -> [u8; 32] {
    use getrandom_or_panic::RngCore;
    let mut s = [0u8; 32];
    getrandom_or_panic::getrandom_or_panic().fill_bytes(&mut s);
    s
}

/// draw(seed, first) | .. | draw(seed, first + n - 1), on the host.  Err: the library's code (first + n beyond 2^64).
pub fn expand(seed: &[u8; 32], first: u64, n: usize) -> Result<Vec<u8>, c_int> {
    let mut out = vec![0u8; 32 * n];
    let rc = unsafe { h2v_draws_expand(seed.as_ptr(), first, n, out.as_mut_ptr()) };
    if rc != 0 { return Err(rc); }
    Ok(out)
}

/// The tail a shard of a sharded batch uploads (h2v_batch_upload's rand32_tail), from the batch's seed instead of a broadcast of the
/// draws: the whole stream is expand(seed, 0, groups * total), group g owns indices [g * total, (g + 1) * total), and the shard that
/// starts at proof `lo` takes [g * total + lo, (g + 1) * total) of each group, group-major.  With `GpuAccumulatorStrategy` — one
/// accumulation, groups = 1 — `seeded_tail(seed, k, k + 1, 1)` is the draw of its k-th `process`, in place of `Fr::random`.
pub fn seeded_tail(seed: &[u8; 32], lo: usize, total: usize, groups: usize) -> Result<Vec<u8>, c_int> {
    assert!(lo <= total, "a shard starts inside its batch");
    let mut out = Vec::with_capacity(32 * groups * (total - lo));
    for g in 0..groups {
        out.extend_from_slice(&expand(seed, (g * total + lo) as u64, total - lo)?);
    }
    Ok(out)
}

/// The same tail into device memory (`d_out32`: groups * (total - lo) draws, 16-byte aligned), a kernel per group on `stream` of
/// `device`; waits for nothing.  What h2v_batch_upload_device takes as d_rand_tail.
pub unsafe fn seeded_tail_device(device: c_int, stream: *mut c_void, seed: &[u8; 32], lo: usize, total: usize, groups: usize, d_out32: *mut c_void) -> Result<(), c_int> {
    assert!(lo <= total, "a shard starts inside its batch");
    let per = total - lo;
    for g in 0..groups {
        if per == 0 { break; }
        let rc = h2v_draws_expand_device(device, stream, seed.as_ptr(), (g * total + lo) as u64, per, (d_out32 as *mut u8).add(32 * g * per) as *mut c_void);
        if rc != 0 { return Err(rc); }
    }
    Ok(())
}
