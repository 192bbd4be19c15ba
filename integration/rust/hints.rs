//! `extern "C"` binding of include/h2v_hints.h — point hints for a staged batch — for the halo2_verifier crate (feature "mi355x").
//! UNCOMPILED in this repository, as ffi.rs is: the build image has no Rust toolchain.  The tested callers of the same seven entry
//! points are halo2_verifier_amd/hints.py (ctypes) and include/h2v_hints.hpp; tests/test_hints_host.py checks that every function the
//! header declares is bound here.  ffi.rs stays the binding of include/h2v.h alone.
//!
//! A hint is the y coordinate of a compressed point of a proof, 32 canonical little-endian bytes: `Fq::to_repr` of
//! `G1Affine::coordinates().unwrap().y()`.  A prover has the affine points it writes to the transcript; a relay or a verifier that has
//! decoded the proof once (`G1Affine::from_bytes`) has them too, and a `GpuStagedBatch` hands out the y of every point of a launch
//! (`hints()`).  A row is the y of the Np points of one proof in the order of their bytes (`point_offsets`).  Hints are checked, never
//! trusted: the results of a launch depend on the proofs, instances and draws only, and a hint that does not hold costs its point the
//! square root it would have paid anyway.
use super::ffi::*;
use super::strategy::GpuStagedBatch;
use crate::plonk::Error;
use core::ffi::{c_int, c_void};
use ff::PrimeField;
use halo2curves::bn256::G1Affine;
use halo2curves::CurveAffine;

extern "C" {
    pub fn h2v_hints_point_offsets(ctx: *const h2v_ctx, offsets: *mut usize, cap: usize, n_points: *mut usize) -> c_int;
    pub fn h2v_hints_from_points(points32: *const u8, n: usize, y32: *mut u8, decoded: *mut u8) -> c_int;
    pub fn h2v_batch_set_hints(b: *mut h2v_batch, n: usize, y32: *const u8) -> c_int;
    pub fn h2v_batch_set_hints_device(b: *mut h2v_batch, n: usize, d_y32: *const c_void, row_stride: usize) -> c_int;
    pub fn h2v_batch_hints(b: *mut h2v_batch, first: usize, count: usize, y32: *mut u8) -> c_int;
    pub fn h2v_batch_hints_device(b: *mut h2v_batch, first: usize, count: usize, d_y32: *mut c_void, row_stride: usize) -> c_int;
    pub fn h2v_batch_hint_stats(b: *mut h2v_batch, n_points: *mut usize, n_hinted: *mut usize, n_missed: *mut usize) -> c_int;
}

/// The library's refusals have no variant of `plonk::Error`: reported as `Opening`, as strategy.rs's `map_err` reports them.
fn code(_rc: c_int) -> Error { Error::Opening }

/// The byte offsets of the Np compressed points inside a proof of the context's key, ascending.
pub fn point_offsets(ctx: *const h2v_ctx) -> Result<Vec<usize>, Error> {
    let mut n = 0usize;
    let rc = unsafe { h2v_hints_point_offsets(ctx, core::ptr::null_mut(), 0, &mut n) };
    if rc != 0 { return Err(code(rc)); }
    let mut off = vec![0usize; n];
    let rc = unsafe { h2v_hints_point_offsets(ctx, off.as_mut_ptr(), off.len(), &mut n) };
    if rc != 0 { Err(code(rc)) } else { Ok(off) }
}

/// The hint of a point the caller holds: its y as 32 canonical little-endian bytes (the identity, which no proof carries: zeros).
pub fn hint_of(p: &G1Affine) -> [u8; 32] {
    let mut out = [0u8; 32];
    if let Some(c) = Option::<halo2curves::Coordinates<G1Affine>>::from(p.coordinates()) { out.copy_from_slice(c.y().to_repr().as_ref()); }
    out
}

/// The hints of compressed points, decoded on the host by the library (no device): 32 zero bytes where `from_bytes` fails.
pub fn from_points(points32: &[u8]) -> Result<Vec<u8>, Error> {
    assert!(points32.len() % 32 == 0);
    let mut y = vec![0u8; points32.len()];
    let rc = unsafe { h2v_hints_from_points(points32.as_ptr(), points32.len() / 32, y.as_mut_ptr(), core::ptr::null_mut()) };
    if rc != 0 { Err(code(rc)) } else { Ok(y) }
}

/// (n_points, n_hinted, n_missed) of the last launch.
pub struct HintStats { pub points: usize, pub hinted: usize, pub missed: usize }

impl GpuStagedBatch {
    /// The hints of the current upload of `n` proofs: n x Np x 32 bytes, or None to drop them.  Uploaded and not launched since.
    pub fn set_hints(&mut self, n: usize, y32: Option<&[u8]>) -> Result<(), Error> {
        let rc = unsafe { h2v_batch_set_hints(self.handle(), n, y32.map_or(core::ptr::null(), |y| y.as_ptr())) };
        if rc != 0 { Err(code(rc)) } else { Ok(()) }
    }
    /// The same from device memory (row i at d_y32 + i * row_stride): device -> device on the batch's stream, no host wait.
    ///
    /// # Safety
    /// `d_y32` is device memory of the context's device holding the rows, kept alive until the stream has copied them.
    pub unsafe fn set_hints_device(&mut self, n: usize, d_y32: *const c_void, row_stride: usize) -> Result<(), Error> {
        let rc = h2v_batch_set_hints_device(self.handle(), n, d_y32, row_stride);
        if rc != 0 { Err(code(rc)) } else { Ok(()) }
    }
    /// The canonical y of the points of proofs [first, first + count) of the last launch, rows of `n_points` x 32 bytes.
    pub fn hints(&self, first: usize, count: usize, n_points: usize) -> Result<Vec<u8>, Error> {
        let mut y = vec![0u8; (32 * count * n_points).max(1)];
        let rc = unsafe { h2v_batch_hints(self.handle(), first, count, y.as_mut_ptr()) };
        y.truncate(32 * count * n_points);
        if rc != 0 { Err(code(rc)) } else { Ok(y) }
    }
    /// The same into device memory by one kernel on the batch's stream; waits for nothing.
    ///
    /// # Safety
    /// `d_y32` is device memory of the context's device with room for the rows.
    pub unsafe fn hints_device(&self, first: usize, count: usize, d_y32: *mut c_void, row_stride: usize) -> Result<(), Error> {
        let rc = h2v_batch_hints_device(self.handle(), first, count, d_y32, row_stride);
        if rc != 0 { Err(code(rc)) } else { Ok(()) }
    }
    pub fn hint_stats(&self) -> Result<HintStats, Error> {
        let (mut points, mut hinted, mut missed) = (0usize, 0usize, 0usize);
        let rc = unsafe { h2v_batch_hint_stats(self.handle(), &mut points, &mut hinted, &mut missed) };
        if rc != 0 { Err(code(rc)) } else { Ok(HintStats { points, hinted, missed }) }
    }
}
