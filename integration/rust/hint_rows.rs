//! `extern "C"` binding of include/h2v_hint_rows.h — a hint row per proof, or none, for a staged batch, the one-shot calls and the
//! resident accumulator — for the halo2_verifier crate (feature "mi355x").  UNCOMPILED in this repository, as ffi.rs and hints.rs are:
//! the build image has no Rust toolchain.  The tested callers of the same four entry points are halo2_verifier_amd/hints.py (ctypes)
//! and include/h2v_hints.hpp; tests/test_hinted_calls_host.py checks that every function the header declares is bound here.  hints.rs
//! stays the binding of include/h2v_hints.h alone, and says what a hint and a hint row are.
//!
//! A service that batches proofs from many senders gets hints from some of them: here a proof has `Some(row)` or `None`.  The results
//! are those of the calls without hints; the points whose hint is not used have their roots taken together on the device.
use super::ffi::*;
use super::hints::HintStats;
use super::strategy::GpuStagedBatch;
use crate::plonk::Error;
use core::ffi::c_int;

extern "C" {
    pub fn h2v_batch_set_hint_rows(b: *mut h2v_batch, n: usize, rows: *const *const u8) -> c_int;
    pub fn h2v_verify_batch_keys_hinted(ctxs: *const *mut h2v_ctx, n_keys: usize, key_of_proof: *const u32, n: usize, proofs: *const *const u8,
                                        proof_lens: *const usize, hint_rows: *const *const u8, instances32: *const *const u8, n_instance_columns: *const usize,
                                        col_lens: *const usize, rand32: *const u8, per_proof_status: *mut c_int, batch_ok: *mut c_int, out_left_xy: *mut u8,
                                        out_right_xy: *mut u8, hint_stats: *mut usize) -> c_int;
    pub fn h2v_verify_batches_hinted(ctx: *mut h2v_ctx, n_batches: usize, batch_sizes: *const usize, proofs: *const *const u8, proof_lens: *const usize,
                                     hint_rows: *const *const u8, instances32: *const *const u8, n_instance_columns: usize, col_lens: *const usize,
                                     rand32: *const u8, per_proof_status: *mut c_int, batch_ok: *mut c_int, out_left_xy: *mut u8, out_right_xy: *mut u8,
                                     hint_stats: *mut usize) -> c_int;
    pub fn h2v_accumulator_process_hinted(a: *mut h2v_accumulator, ctxs: *const *mut h2v_ctx, n_keys: usize, key_of_proof: *const u32, n: usize,
                                          proofs: *const *const u8, proof_lens: *const usize, hint_rows: *const *const u8, instances32: *const *const u8,
                                          n_instance_columns: *const usize, col_lens: *const usize, rand32: *const u8, per_proof_status: *mut c_int,
                                          all_ok: *mut c_int, hint_stats: *mut usize) -> c_int;
}

/// The library's refusals have no variant of `plonk::Error`: reported as `Opening`, as strategy.rs's `map_err` reports them.
fn code(_rc: c_int) -> Error { Error::Opening }

/// The pointer array the entry points take: null where a proof has no row.  `n_points[i]` is Np of proof i's key.
pub fn row_pointers(rows: &[Option<&[u8]>], n_points: &[usize]) -> Vec<*const u8> {
    assert!(rows.len() == n_points.len());
    rows.iter().zip(n_points).map(|(r, np)| match r {
        Some(row) => { assert!(row.len() == 32 * np); row.as_ptr() }
        None => core::ptr::null(),
    }).collect()
}

/// The three counters a `_hinted` call returns: the points of its proofs, the hinted ones, the hinted ones whose hint was not used.
pub fn stats_of(raw: [usize; 3]) -> HintStats { HintStats { points: raw[0], hinted: raw[1], missed: raw[2] } }

impl GpuStagedBatch {
    /// The hints of the current upload from one row per proof (`None`: its sender gave none); `n_points` is Np of the batch's key.
    /// Uploaded and not launched since.  `hint_stats()` then counts the rows given.
    pub fn set_hint_rows(&mut self, rows: &[Option<&[u8]>], n_points: usize) -> Result<(), Error> {
        let p = row_pointers(rows, &vec![n_points; rows.len()]);
        let rc = unsafe { h2v_batch_set_hint_rows(self.handle(), rows.len(), p.as_ptr()) };
        if rc != 0 { Err(code(rc)) } else { Ok(()) }
    }
}
