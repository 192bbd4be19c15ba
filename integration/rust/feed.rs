//! `extern "C"` binding of include/h2v_feed.h — feed a launched staged batch to a resident accumulator without a host wait — for the
//! halo2_verifier crate (feature "mi355x").  UNCOMPILED in this repository, as ffi.rs is: the build image has no Rust toolchain.  The
//! tested callers of the same three entry points are halo2_verifier_amd/feed.py (ctypes) and include/h2v_feed.hpp;
//! tests/test_feed_host.py checks that every function the header declares is bound here.  ffi.rs stays the binding of include/h2v.h
//! alone.  The safe methods are `GpuResidentAccumulator::{feed_batch, settle, pending}` in strategy.rs, beside `process_batch`.
//!
//! `feed_batch` is `process_batch` ENQUEUED: the groups of the batch's last launch become legs of the accumulator on the device, behind
//! the launch; nothing waits, and the batch may be uploaded again at once.  `settle` waits for the accumulator's stream once, commits
//! the counters and journal entries of every feed since, and returns a `FeedReport` per feed since the last `settle`.  Every other
//! call on the accumulator settles first and leaves the reports queued.  A feed the device dropped (a draw >= r in a tail uploaded
//! from device memory) reports `rc = -16`: the points keep their value, no journal entry appears, and its proofs count as failed.
use super::ffi::*;
use core::ffi::c_int;

pub const H2V_FEED_MAX_PENDING: usize = 64;

extern "C" {
    pub fn h2v_accumulator_feed_batch(a: *mut h2v_accumulator, b: *mut h2v_batch) -> c_int;
    pub fn h2v_accumulator_pending(a: *const h2v_accumulator, n_unsettled: *mut usize, n_unreported: *mut usize) -> c_int;
    pub fn h2v_accumulator_settle(a: *mut h2v_accumulator, cap: usize, n_feeds: *mut usize, feed_rc: *mut c_int, feed_proofs: *mut usize,
                                  feed_failed: *mut usize) -> c_int;
}

/// One feed as `settle` reports it.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct FeedReport { pub rc: i32, pub n_proofs: usize, pub n_failed: usize }

/// `h2v_accumulator_settle` over a raw handle: the count first, then the reports.  `Err(rc)` is the library's code.
pub unsafe fn settle_raw(a: *mut h2v_accumulator) -> Result<Vec<FeedReport>, c_int> {
    let mut n = 0usize;
    let rc = h2v_accumulator_settle(a, 0, &mut n, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut());
    if rc != 0 { return Err(rc); }
    let (mut codes, mut proofs, mut failed) = (vec![0 as c_int; n.max(1)], vec![0usize; n.max(1)], vec![0usize; n.max(1)]);
    let rc = h2v_accumulator_settle(a, n, &mut n, codes.as_mut_ptr(), proofs.as_mut_ptr(), failed.as_mut_ptr());
    if rc != 0 { return Err(rc); }
    Ok((0..n).map(|i| FeedReport { rc: codes[i], n_proofs: proofs[i], n_failed: failed[i] }).collect())
}
