//! `extern "C"` binding of include/h2v_guards.h — every proof's Guard out of a launched staged batch — for the halo2_verifier crate
//! (feature "mi355x").  UNCOMPILED in this repository, as ffi.rs is: the build image has no Rust toolchain.  The tested callers of the
//! same four entry points are halo2_verifier_amd/guards.py (ctypes) and include/h2v_guards.hpp; tests/test_guards_out_host.py checks
//! that every function the header declares is bound here.  ffi.rs stays the binding of include/h2v.h alone.
//!
//! Seam 2½ — the GPU drives, your strategy decides.  `GpuStagedBatch` runs `verify_proof` for all its proofs in one launch; `guards()`
//! hands each proof's `GuardKZG` to the caller's own `VerificationStrategy`, so a custom scaling scheme, Guards sorted into several
//! accumulators, or an `AccumulatorStrategy::with` resumed elsewhere keep working unchanged.  Term t of proof first + j lies at index
//! j * T + t of a channel.  Upload with UNIT draws (every draw 1) to get raw Guards: otherwise every scalar carries `mult`, the
//! product of the draws behind the proof inside its group.  SHPLONK: the reference's term order.  GWC: a commitment opened at several
//! points occurs once with its scalars summed — sum-equal to the reference's list, not term for term.  A proof whose status is not 0
//! has no Guard (its terms are zero scalars under the identity): `guards()` reports its error instead.
use super::ffi::*;
use super::strategy::GpuStagedBatch;
use crate::{
    plonk::Error,
    poly::{commitment::{Verifier, MSM}, kzg::{commitment::{KZGCommitmentScheme, ParamsKZG}, msm::DualMSM, strategy::GuardKZG}, strategy::VerificationStrategy},
};
use core::ffi::{c_int, c_void};
use ff::PrimeField;
use halo2curves::bn256::{Bn256, Fq, Fr, G1Affine};
use halo2curves::CurveAffine;

extern "C" {
    pub fn h2v_batch_guard_shape(b: *const h2v_batch, n_left_terms: *mut usize, n_right_terms: *mut usize) -> c_int;
    pub fn h2v_batch_guards_device(b: *mut h2v_batch, first: usize, count: usize, d_left_scalars32: *mut c_void, d_left_bases64: *mut c_void,
                                   d_right_scalars32: *mut c_void, d_right_bases64: *mut c_void, d_mult32: *mut c_void, d_status: *mut c_void) -> c_int;
    pub fn h2v_batch_guards(b: *mut h2v_batch, first: usize, count: usize, left_scalars32: *mut u8, left_bases64: *mut u8, right_scalars32: *mut u8,
                            right_bases64: *mut u8, mult32: *mut u8, per_proof_status: *mut c_int) -> c_int;
    pub fn h2v_batch_guards_append(b: *mut h2v_batch, first: usize, count: usize, left: *mut h2v_msm, right: *mut h2v_msm, n_failed: *mut usize) -> c_int;
}

/// The library's codes as `plonk::Error`: -1 .. -6 are the enum in declaration order (-4 is `Opening`); everything else — -7, an input
/// on which the reference panics, and the library's own refusals -16 .. -19 — has no variant and is reported as `Opening`, as
/// strategy.rs's `map_err` reports it.
fn code(rc: c_int) -> Error {
    match rc { -1 => Error::InvalidInstances, -2 => Error::ConstraintSystemFailure, -3 => Error::BoundsFailure,
               -5 => Error::Transcript("h2v"), -6 => Error::InstanceTooLarge, _ => Error::Opening }
}

/// The Guards of a range on the host: flat term arrays (proof after proof), the proofs' multipliers and statuses.
pub struct HostGuards {
    pub left_terms: usize, pub right_terms: usize, pub count: usize,
    pub left_scalars: Vec<u8>, pub left_bases: Vec<u8>, pub right_scalars: Vec<u8>, pub right_bases: Vec<u8>,
    pub mult: Vec<u8>, pub status: Vec<i32>,
}

fn scalar(b: &[u8]) -> Fr { let mut r = <Fr as PrimeField>::Repr::default(); r.as_mut().copy_from_slice(b); Fr::from_repr(r).unwrap() }
fn base(b: &[u8]) -> G1Affine {
    if b.iter().all(|&v| v == 0) { return G1Affine::default(); }   // the identity
    let coord = |s: &[u8]| { let mut r = <Fq as PrimeField>::Repr::default(); r.as_mut().copy_from_slice(s); Fq::from_repr(r).unwrap() };
    G1Affine::from_xy(coord(&b[..32]), coord(&b[32..])).unwrap()
}

impl GpuStagedBatch {
    /// (T_L, T_R): the terms of a proof's two channels under the plan of the upload
    pub fn guard_shape(&self) -> Result<(usize, usize), Error> {
        let (mut tl, mut tr) = (0usize, 0usize);
        let rc = unsafe { h2v_batch_guard_shape(self.handle(), &mut tl, &mut tr) };
        if rc != 0 { Err(code(rc)) } else { Ok((tl, tr)) }
    }
    /// The Guards of proofs [first, first + count) of the last launch as host arrays (h2v_batch_guards: one copy, one synchronise).
    pub fn guards_host(&mut self, first: usize, count: usize) -> Result<HostGuards, Error> {
        let (tl, tr) = self.guard_shape()?;
        let mut g = HostGuards { left_terms: tl, right_terms: tr, count,
                                 left_scalars: vec![0; 32 * count * tl], left_bases: vec![0; 64 * count * tl], right_scalars: vec![0; 32 * count * tr],
                                 right_bases: vec![0; 64 * count * tr], mult: vec![0; 32 * count], status: vec![0; count] };
        let rc = unsafe { h2v_batch_guards(self.handle(), first, count, g.left_scalars.as_mut_ptr(), g.left_bases.as_mut_ptr(), g.right_scalars.as_mut_ptr(),
                                           g.right_bases.as_mut_ptr(), g.mult.as_mut_ptr(), g.status.as_mut_ptr()) };
        if rc != 0 { Err(code(rc)) } else { Ok(g) }
    }
    /// Feed every proof of the range to `strategy`, as N x `verify_proof` would: `process` receives a closure that adds the proof's
    /// two term lists to the strategy's MSM and returns the Guard, or the proof's own error.  The strategy decides everything else —
    /// scaling, accumulation, the pairing.  `V` is the multi-open scheme of the batch's context (`VerifierSHPLONK` or `VerifierGWC`: both
    /// have `Guard = GuardKZG` and `MSMAccumulator = DualMSM`).  The strategy must return itself from `process` (`Output = Self`, as
    /// `AccumulatorStrategy` and strategies built like it do), because one value is fed N proofs in turn; a strategy that is consumed
    /// by one proof (`SingleStrategy`: `Output = ()`) takes one proof per value — make one per proof and call this with `count = 1`,
    /// or read `guards_host` and call its `process` yourself.
    pub fn guards<'params, V, S>(&mut self, params: &'params ParamsKZG<Bn256>, first: usize, count: usize, mut strategy: S) -> Result<S, Error>
    where V: Verifier<'params, KZGCommitmentScheme<Bn256>, Guard = GuardKZG<'params, Bn256>, MSMAccumulator = DualMSM<'params, Bn256>>,
          S: VerificationStrategy<'params, KZGCommitmentScheme<Bn256>, V, Output = S> {
        let _ = params;
        let g = self.guards_host(first, count)?;
        for j in 0..count {
            let status = g.status[j];
            strategy = strategy.process(|mut msm: DualMSM<'params, Bn256>| {
                if status != 0 { return Err(code(status)); }
                for t in 0..g.left_terms { let i = j * g.left_terms + t; msm.left.append_term(scalar(&g.left_scalars[32 * i..32 * i + 32]), base(&g.left_bases[64 * i..64 * i + 64]).into()); }
                for t in 0..g.right_terms { let i = j * g.right_terms + t; msm.right.append_term(scalar(&g.right_scalars[32 * i..32 * i + 32]), base(&g.right_bases[64 * i..64 * i + 64]).into()); }
                Ok(GuardKZG::new(msm))
            })?;
        }
        Ok(strategy)
    }
    /// The range's terms behind the end of two resident MSM objects, without a byte in between (h2v_batch_guards_append) -> the proofs
    /// of the range with a status.  Either handle may be null.
    pub unsafe fn guards_append(&mut self, first: usize, count: usize, left: *mut h2v_msm, right: *mut h2v_msm) -> Result<usize, Error> {
        let mut failed = 0usize;
        let rc = h2v_batch_guards_append(self.handle(), first, count, left, right, &mut failed);
        if rc != 0 { Err(code(rc)) } else { Ok(failed) }
    }
    /// Into device memory, by kernels on the batch's stream; waits for nothing.  Every pointer may be null (not wanted).
    /// Safety: every pointer given is device memory with room for what the call writes, 16-byte aligned, read only behind the batch's stream.
    pub unsafe fn guards_device(&mut self, first: usize, count: usize, d_left_scalars32: *mut c_void, d_left_bases64: *mut c_void, d_right_scalars32: *mut c_void,
                                d_right_bases64: *mut c_void, d_mult32: *mut c_void, d_status: *mut c_void) -> Result<(), Error> {
        let rc = h2v_batch_guards_device(self.handle(), first, count, d_left_scalars32, d_left_bases64, d_right_scalars32, d_right_bases64, d_mult32, d_status);
        if rc != 0 { Err(code(rc)) } else { Ok(()) }
    }
}
