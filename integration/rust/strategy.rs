//! GPU-backed drop-ins at the reference's two seams (UNCOMPILED here — no rustc in the build image).
//!
//! * `GpuBatchVerifier`        — whole-batch seam: N x `verify_proof` + `AccumulatorStrategy::finalize`
//!                               (halo2_verifier/src/lib.rs:33-49, poly/kzg/strategy.rs:125-140) in one call.
//!                               `with_seed` resumes an existing accumulator (`AccumulatorStrategy::with`), and
//!                               `finalize_identify` names the failing proofs, with or without a seed.
//! * `GpuStagedBatch`          — the staged interface (h2v_batch_*): proofs resident on the GPU, `upload` / `launch` / `finish`, and
//!                               `identify` on the finished launch — also after a fold (a shard of a sharded batch).
//! * `GpuMultiKeyVerifier`     — the same seam over several VerifyingKeys sharing the params: one context per key,
//!                               `push(key, proof, instances)`, one pairing at `finalize` (h2v_verify_batch_keys).
//! * `GpuResidentAccumulator`  — the incremental seam: an accumulator that stays on the GPU across `process` calls over any keys
//!                               sharing the params; `finalize` whenever the caller decides (h2v_accumulator_*).
//!                               `process_guards` takes the Guards of proofs that a CPU `verify_proof` went through.
//!                               `process_batch` takes the groups of a finished `GpuStagedBatch` as legs, from what its launch left on the GPU.
//!                               `merge` / `export_state` / `merge_states` fold several of them into one pairing.
//!                               Its leg journal (`journal_begin`, `check_legs`, `drop_legs`) finds the legs whose own pairing
//!                               fails and takes them out again.
//! * `GpuAccumulatorStrategy`  — trait seam: `impl VerificationStrategy` (poly/strategy.rs:12-31) over a resident accumulator:
//!                               `verify_proof` itself stays on the CPU, every Guard it returns is scaled in and added on the GPU
//!                               (h2v_accumulator_process_guards), `finalize` is the one pairing there.
//! * `GpuMsm`, `GpuDualMsm`    — the `MSM` trait row: `impl MSM<G1Affine>` over a term list resident on the GPU (h2v_msm_*), and the
//!                               two-channel object with the pairing; evaluation and check for many objects per launch.
use super::ffi::*;
use crate::{
    helpers::SerdeFormat,
    plonk::Error,
    poly::{
        commitment::MSM,
        kzg::{commitment::{KZGCommitmentScheme, ParamsKZG}, msm::DualMSM, multiopen::VerifierSHPLONK, strategy::GuardKZG},
        strategy::VerificationStrategy,
    },
    VerifyingKey,
};
use ff::{Field, PrimeField};
use group::{prime::PrimeCurveAffine, Curve, Group};
use halo2curves::bn256::{Bn256, Fr, G1Affine};
use halo2curves::CurveAffine;

fn map_err(rc: i32) -> Error {
    match rc { -1 => Error::InvalidInstances, -2 => Error::ConstraintSystemFailure, -3 => Error::BoundsFailure,
               -5 => Error::Transcript("h2v"), -6 => Error::InstanceTooLarge, _ => Error::Opening }
}

pub struct GpuBatchVerifier<'p> {
    ctx: *mut h2v_ctx,
    proofs: Vec<&'p [u8]>,
    instances: Vec<Vec<u8>>,
    col_lens: Vec<usize>,
    seed: Option<[(Vec<u8>, Vec<u8>); 2]>,   // (scalars, bases) of the left and the right channel
}

/// The terms of one `MSMKZG` channel as the C ABI takes them: 32-byte scalars, 64-byte x | y bases (all-zero = identity).
fn flat_terms(terms: &[(Fr, G1Affine)]) -> (Vec<u8>, Vec<u8>) {
    let (mut s, mut b) = (Vec::new(), Vec::new());
    for (k, p) in terms {
        s.extend_from_slice(k.to_repr().as_ref());
        let c = p.coordinates();
        if bool::from(c.is_some()) { let c = c.unwrap(); b.extend_from_slice(c.x().to_repr().as_ref()); b.extend_from_slice(c.y().to_repr().as_ref()); }
        else { b.extend_from_slice(&[0u8; 64]); }
    }
    (s, b)
}

impl<'p> GpuBatchVerifier<'p> {
    pub fn new(params: &ParamsKZG<Bn256>, vk: &VerifyingKey<G1Affine>, device: i32) -> Result<Self, Error> {
        let (mut pb, mut vb) = (Vec::new(), Vec::new());
        params.write_custom(&mut pb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
        vk.write(&mut vb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
        let mut ctx = core::ptr::null_mut();
        let rc = unsafe { h2v_ctx_create(pb.as_ptr(), pb.len(), H2V_SERDE_RAW_BYTES, vb.as_ptr(), vb.len(), H2V_SERDE_RAW_BYTES, device, &mut ctx) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(Self { ctx, proofs: Vec::new(), instances: Vec::new(), col_lens: Vec::new(), seed: None })
    }

    /// `AccumulatorStrategy::with(msm_accumulator)` (poly/kzg/strategy.rs:75-78): start from an existing `DualMSM`, given as the terms of
    /// its two channels.  `finalize_identify` then runs h2v_verify_batch_seeded_identify.
    pub fn with_seed(mut self, left: &[(Fr, G1Affine)], right: &[(Fr, G1Affine)]) -> Self {
        self.seed = Some([flat_terms(left), flat_terms(right)]);
        self
    }

    /// One `verify_proof(&params, &vk, strategy, &[instances], &mut Blake2bRead::init(proof))` call.
    pub fn push(&mut self, proof: &'p [u8], instances: &[&[Fr]]) {
        if self.col_lens.is_empty() { self.col_lens = instances.iter().map(|c| c.len()).collect(); }
        let mut flat = Vec::with_capacity(32 * instances.iter().map(|c| c.len()).sum::<usize>());
        for col in instances { for v in col.iter() { flat.extend_from_slice(v.to_repr().as_ref()); } }
        self.proofs.push(proof);
        self.instances.push(flat);
    }

    /// `strategy.finalize()`: true iff every proof is well formed and the single pairing check passes.
    pub fn finalize(self) -> Result<bool, Error> {
        let n = self.proofs.len();
        let ptrs: Vec<*const u8> = self.proofs.iter().map(|p| p.as_ptr()).collect();
        let lens: Vec<usize> = self.proofs.iter().map(|p| p.len()).collect();
        let iptrs: Vec<*const u8> = self.instances.iter().map(|i| i.as_ptr()).collect();
        let (mut status, mut ok) = (vec![0i32; n], 0i32);
        let rc = unsafe { h2v_verify_batch(self.ctx, n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(), self.col_lens.len(), self.col_lens.as_ptr(),
                                           core::ptr::null(), status.as_mut_ptr(), &mut ok, core::ptr::null_mut(), core::ptr::null_mut()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(ok == 1)
    }

    /// `finalize`, plus the verdict of every proof: `Ok(())` or the `Error` that `verify_proof` under `SingleStrategy` returns for it
    /// (`ConstraintSystemFailure` for the proofs whose own pairing fails).  When the batch passes this costs what `finalize` costs;
    /// otherwise the failing ranges of proofs are re-checked on the GPU until single proofs remain (h2v_verify_batch_identify).
    pub fn finalize_identify(self) -> Result<(bool, Vec<Result<(), Error>>), Error> {
        self.finalize_identify_seeded().map(|(ok, verdicts, _)| (ok, verdicts))
    }

    /// `finalize_identify`, plus the verdict of the seed alone (`true` without a seed and for an empty one).  The seed's terms belong to
    /// no proof and enter no proof's verdict: a failing batch whose proofs are all `Ok(())` and whose seed fails resumed a bad
    /// accumulator (h2v_verify_batch_seeded_identify).
    pub fn finalize_identify_seeded(self) -> Result<(bool, Vec<Result<(), Error>>, bool), Error> {
        let n = self.proofs.len();
        let ptrs: Vec<*const u8> = self.proofs.iter().map(|p| p.as_ptr()).collect();
        let lens: Vec<usize> = self.proofs.iter().map(|p| p.len()).collect();
        let iptrs: Vec<*const u8> = self.instances.iter().map(|i| i.as_ptr()).collect();
        let (mut status, mut ok, mut seed_ok, mut checks) = (vec![0i32; n.max(1)], 0i32, 1i32, 0usize);
        let rc = match &self.seed {
            Some([(ls, lb), (rs, rb)]) => unsafe {
                h2v_verify_batch_seeded_identify(self.ctx, n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(), self.col_lens.len(), self.col_lens.as_ptr(),
                                                 core::ptr::null(), ls.as_ptr(), lb.as_ptr(), ls.len() / 32, rs.as_ptr(), rb.as_ptr(), rs.len() / 32,
                                                 status.as_mut_ptr(), &mut ok, &mut seed_ok, core::ptr::null_mut(), core::ptr::null_mut(), &mut checks) },
            None => unsafe {
                h2v_verify_batch_identify(self.ctx, n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(), self.col_lens.len(), self.col_lens.as_ptr(),
                                          core::ptr::null(), status.as_mut_ptr(), &mut ok, core::ptr::null_mut(), core::ptr::null_mut(), &mut checks) },
        };
        if rc != 0 { return Err(map_err(rc)); }
        let verdicts = status[..n].iter().map(|&s| if s == 0 { Ok(()) } else { Err(map_err(s)) }).collect();
        Ok((ok == 1, verdicts, seed_ok == 1))
    }
}
impl<'p> Drop for GpuBatchVerifier<'p> { fn drop(&mut self) { unsafe { h2v_ctx_destroy(self.ctx) } } }

/// The staged interface on one context (h2v_batch_*): the proofs stay resident on the GPU between `upload`, `launch`, `finish` and
/// `identify`.  `groups` independent accumulator batches travel in one launch (h2v_batch_set_groups).  The context outlives the batch.
pub struct GpuStagedBatch { b: *mut h2v_batch, n: usize, groups: usize }

impl GpuStagedBatch {
    pub fn new(ctx: *mut h2v_ctx, max_proofs: usize, max_instance_values: usize, groups: usize) -> Result<Self, Error> {
        let mut b = core::ptr::null_mut();
        let rc = unsafe { h2v_batch_create(ctx, max_proofs, max_instance_values, &mut b) };
        if rc != 0 { return Err(map_err(rc)); }
        let me = Self { b, n: 0, groups };
        if groups != 1 { let rc = unsafe { h2v_batch_set_groups(me.b, groups) }; if rc != 0 { return Err(map_err(rc)); } }
        Ok(me)
    }
    /// `n` proofs of `proof_len` bytes each, their instance values (32 bytes each) and the draws from the shard's first proof to the end
    /// of the whole batch (empty: OS draws, unsharded only).
    pub fn upload(&mut self, n: usize, proofs_flat: &[u8], proof_len: usize, instances_flat: &[u8], col_lens: &[usize], rand_tail: &[u8]) -> Result<(), Error> {
        if proofs_flat.len() != n * proof_len || instances_flat.len() != n * col_lens.iter().sum::<usize>() * 32 || rand_tail.len() % 32 != 0 { return Err(Error::InvalidInstances); }
        let tail = if rand_tail.is_empty() { core::ptr::null() } else { rand_tail.as_ptr() };
        let rc = unsafe { h2v_batch_upload(self.b, n, proofs_flat.as_ptr(), proof_len, instances_flat.as_ptr(), col_lens.len(), col_lens.as_ptr(), tail, rand_tail.len() / 32) };
        if rc != 0 { return Err(map_err(rc)); }
        self.n = n;
        Ok(())
    }
    /// `upload` for inputs already in device memory (h2v_batch_upload_device): `n` proof rows `proof_stride` bytes apart at `d_proofs`,
    /// the flat instance values at `d_instances`, `n_tail` draws at `d_rand_tail` (null: OS draws, the one form that waits for the
    /// stream).  Device work only, on the batch's stream; a draw that is not canonical is reported by `finish`.
    /// Safety: the pointers are device memory that holds what the call reads, and stays untouched until `finish` has returned.
    pub unsafe fn upload_device(&mut self, n: usize, d_proofs: *const core::ffi::c_void, proof_stride: usize, d_instances: *const core::ffi::c_void, col_lens: &[usize],
                                d_rand_tail: *const core::ffi::c_void, n_tail: usize) -> Result<(), Error> {
        if proof_stride % 16 != 0 || (d_proofs as usize | d_instances as usize | d_rand_tail as usize) % 16 != 0 || (!d_rand_tail.is_null() && n_tail < n) { return Err(Error::InvalidInstances); }
        let rc = h2v_batch_upload_device(self.b, n, d_proofs, proof_stride, d_instances, col_lens.len(), col_lens.as_ptr(), d_rand_tail, if d_rand_tail.is_null() { 0 } else { n_tail });
        if rc != 0 { return Err(map_err(rc)); }
        self.n = n;
        Ok(())
    }
    pub fn launch(&mut self, with_pairing: bool) -> Result<(), Error> {
        let rc = unsafe { h2v_batch_launch(self.b, with_pairing as i32) };
        if rc != 0 { Err(map_err(rc)) } else { Ok(()) }
    }
    /// -> the verdict of every group and the status of every proof
    pub fn finish(&mut self) -> Result<(Vec<bool>, Vec<i32>), Error> {
        let (mut status, mut ok) = (vec![0i32; self.n.max(1)], vec![0i32; self.groups]);
        let rc = unsafe { h2v_batch_finish_groups(self.b, status.as_mut_ptr(), ok.as_mut_ptr(), core::ptr::null_mut(), core::ptr::null_mut(), self.groups) };
        if rc != 0 { return Err(map_err(rc)); }
        status.truncate(self.n);
        Ok((ok.iter().map(|&v| v == 1).collect(), status))
    }
    /// `finish` into device memory (h2v_batch_finish_device): the launch's results written by kernels on the batch's stream, nothing
    /// waited for; the stage does not change and the call may be repeated.  Every pointer may be null (not wanted): `n` i32 statuses,
    /// `groups` i32 verdicts, 64 bytes per group of either channel, `groups` u32 counts of failing proofs, the first `failed_cap`
    /// failing proofs' indices in ascending order, H2V_SUMMARY_WORDS u32.
    /// Safety: every pointer given is device memory with room for what the call writes, 16-byte aligned, and is read only behind the
    /// batch's stream.
    pub unsafe fn finish_device(&mut self, d_status: *mut core::ffi::c_void, d_group_ok: *mut core::ffi::c_void, d_left_xy: *mut core::ffi::c_void,
                                d_right_xy: *mut core::ffi::c_void, d_group_failed: *mut core::ffi::c_void, d_failed_index: *mut core::ffi::c_void, failed_cap: usize,
                                d_summary: *mut core::ffi::c_void) -> Result<(), Error> {
        if (d_status as usize | d_group_ok as usize | d_left_xy as usize | d_right_xy as usize | d_group_failed as usize | d_failed_index as usize | d_summary as usize) % 16 != 0
            || (!d_failed_index.is_null() && failed_cap == 0) { return Err(Error::InvalidInstances); }
        let rc = h2v_batch_finish_device(self.b, d_status, d_group_ok, d_left_xy, d_right_xy, d_group_failed, d_failed_index, if d_failed_index.is_null() { 0 } else { failed_cap }, d_summary);
        if rc != 0 { Err(map_err(rc)) } else { Ok(()) }
    }
    /// Which proofs of the finished launch fail the pairing (h2v_batch_identify): every proof's verdict as `verify_proof` under
    /// `SingleStrategy` returns it, the pairing of every group's own accumulators, and the number of range checks the search ran.
    /// `own_records`: the device address of the records h2v_batch_export_accumulators wrote for this launch — needed after a fold
    /// (h2v_batch_fold_check_enqueue), which overwrites the batch's own accumulators; null otherwise.
    pub fn identify(&mut self, own_records: *const core::ffi::c_void) -> Result<(Vec<Result<(), Error>>, Vec<bool>, usize), Error> {
        let (mut status, mut own, mut checks) = (vec![0i32; self.n.max(1)], vec![0i32; self.groups], 0usize);
        let rc = unsafe { h2v_batch_identify(self.b, own_records, status.as_mut_ptr(), own.as_mut_ptr(), &mut checks) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok((status[..self.n].iter().map(|&s| if s == 0 { Ok(()) } else { Err(map_err(s)) }).collect(), own.iter().map(|&v| v == 1).collect(), checks))
    }
    pub fn handle(&self) -> *mut h2v_batch { self.b }
}
impl Drop for GpuStagedBatch { fn drop(&mut self) { unsafe { h2v_batch_destroy(self.b) } } }

/// Whole-batch seam over several circuits: N x `verify_proof` with a different `vk` per call on ONE `AccumulatorStrategy`, then
/// `finalize` — one pairing for all of them (h2v_verify_batch_keys).  Every key shares the params.
pub struct GpuMultiKeyVerifier<'p> {
    ctxs: Vec<*mut h2v_ctx>,
    n_cols: Vec<usize>,
    keys: Vec<u32>,
    proofs: Vec<&'p [u8]>,
    instances: Vec<Vec<u8>>,
    col_lens: Vec<usize>,
}

impl<'p> GpuMultiKeyVerifier<'p> {
    /// One context per key (key index = position in `vks`), all over `params`.
    pub fn new(params: &ParamsKZG<Bn256>, vks: &[&VerifyingKey<G1Affine>], device: i32) -> Result<Self, Error> {
        let mut pb = Vec::new();
        params.write_custom(&mut pb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
        let mut me = Self { ctxs: Vec::new(), n_cols: Vec::new(), keys: Vec::new(), proofs: Vec::new(), instances: Vec::new(), col_lens: Vec::new() };
        for vk in vks {
            let mut vb = Vec::new();
            vk.write(&mut vb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
            let mut ctx = core::ptr::null_mut();
            let rc = unsafe { h2v_ctx_create(pb.as_ptr(), pb.len(), H2V_SERDE_RAW_BYTES, vb.as_ptr(), vb.len(), H2V_SERDE_RAW_BYTES, device, &mut ctx) };
            if rc != 0 { return Err(map_err(rc)); }   // (the contexts made so far go with `me`)
            me.ctxs.push(ctx);
            let mut ncols = 0usize;
            let rc = unsafe { h2v_ctx_proof_shape(ctx, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), &mut ncols) };
            if rc != 0 { return Err(map_err(rc)); }
            me.n_cols.push(ncols);
        }
        Ok(me)
    }

    /// One `verify_proof(&params, vks[key], strategy, &[instances], &mut Blake2bRead::init(proof))` call.
    pub fn push(&mut self, key: usize, proof: &'p [u8], instances: &[&[Fr]]) -> Result<(), Error> {
        if key >= self.ctxs.len() || instances.len() != self.n_cols[key] { return Err(Error::InvalidInstances); }
        let mut flat = Vec::with_capacity(32 * instances.iter().map(|c| c.len()).sum::<usize>());
        for col in instances { for v in col.iter() { flat.extend_from_slice(v.to_repr().as_ref()); } }
        self.col_lens.extend(instances.iter().map(|c| c.len()));
        self.keys.push(key as u32);
        self.proofs.push(proof);
        self.instances.push(flat);
        Ok(())
    }

    /// `strategy.finalize()`: true iff every proof is well formed and the single pairing check passes.
    pub fn finalize(self) -> Result<bool, Error> {
        let n = self.proofs.len();
        let ptrs: Vec<*const u8> = self.proofs.iter().map(|p| p.as_ptr()).collect();
        let lens: Vec<usize> = self.proofs.iter().map(|p| p.len()).collect();
        let iptrs: Vec<*const u8> = self.instances.iter().map(|i| i.as_ptr()).collect();
        let (mut status, mut ok) = (vec![0i32; n.max(1)], 0i32);
        let rc = unsafe { h2v_verify_batch_keys(self.ctxs.as_ptr(), self.ctxs.len(), self.keys.as_ptr(), n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(),
                                                self.n_cols.as_ptr(), self.col_lens.as_ptr(), core::ptr::null(), status.as_mut_ptr(), &mut ok,
                                                core::ptr::null_mut(), core::ptr::null_mut()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(ok == 1)
    }

    /// `finalize`, plus the verdict of every proof in push order: `Ok(())` or the `Error` that `verify_proof` under `SingleStrategy`
    /// with that proof's key returns for it (`ConstraintSystemFailure` for the proofs whose own pairing fails).  When the pairing passes
    /// this costs what `finalize` costs; otherwise the failing ranges of every key's proofs are re-checked on the GPU together until
    /// single proofs remain (h2v_verify_batch_keys_identify).
    pub fn finalize_identify(self) -> Result<(bool, Vec<Result<(), Error>>), Error> {
        let n = self.proofs.len();
        let ptrs: Vec<*const u8> = self.proofs.iter().map(|p| p.as_ptr()).collect();
        let lens: Vec<usize> = self.proofs.iter().map(|p| p.len()).collect();
        let iptrs: Vec<*const u8> = self.instances.iter().map(|i| i.as_ptr()).collect();
        let (mut status, mut ok, mut checks) = (vec![0i32; n.max(1)], 0i32, 0usize);
        let rc = unsafe { h2v_verify_batch_keys_identify(self.ctxs.as_ptr(), self.ctxs.len(), self.keys.as_ptr(), n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(),
                                                         self.n_cols.as_ptr(), self.col_lens.as_ptr(), core::ptr::null(), status.as_mut_ptr(), &mut ok,
                                                         core::ptr::null_mut(), core::ptr::null_mut(), &mut checks) };
        if rc != 0 { return Err(map_err(rc)); }
        let verdicts = status[..n].iter().map(|&s| if s == 0 { Ok(()) } else { Err(map_err(s)) }).collect();
        Ok((ok == 1, verdicts))
    }
}
impl<'p> Drop for GpuMultiKeyVerifier<'p> { fn drop(&mut self) { for &c in &self.ctxs { unsafe { h2v_ctx_destroy(c) } } } }

/// The incremental seam: `AccumulatorStrategy` as the reference uses it — `verify_proof` per proof as proofs arrive, any `vk` over the
/// same params on every call, `finalize` whenever the caller decides (poly/kzg/strategy.rs:125-140) — with the two accumulator points
/// resident on the GPU between calls (h2v_accumulator_*).  `process` feeds a run of proofs; `process(a); process(b); finalize()` equals
/// one `GpuMultiKeyVerifier` over `a` then `b`.
pub struct GpuResidentAccumulator {
    ctxs: Vec<*mut h2v_ctx>,
    n_cols: Vec<usize>,
    acc: *mut h2v_accumulator,
}

impl GpuResidentAccumulator {
    /// `AccumulatorStrategy::new(params)`: one context per key (key index = position in `vks`, at least one), an empty accumulator.
    pub fn new(params: &ParamsKZG<Bn256>, vks: &[&VerifyingKey<G1Affine>], device: i32) -> Result<Self, Error> {
        let mut pb = Vec::new();
        params.write_custom(&mut pb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
        let mut me = Self { ctxs: Vec::new(), n_cols: Vec::new(), acc: core::ptr::null_mut() };
        for vk in vks {
            let mut vb = Vec::new();
            vk.write(&mut vb, SerdeFormat::RawBytes).map_err(|_| Error::Opening)?;
            let mut ctx = core::ptr::null_mut();
            let rc = unsafe { h2v_ctx_create(pb.as_ptr(), pb.len(), H2V_SERDE_RAW_BYTES, vb.as_ptr(), vb.len(), H2V_SERDE_RAW_BYTES, device, &mut ctx) };
            if rc != 0 { return Err(map_err(rc)); }   // (what was made so far goes with `me`)
            me.ctxs.push(ctx);
            let mut ncols = 0usize;
            let rc = unsafe { h2v_ctx_proof_shape(ctx, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut(), &mut ncols) };
            if rc != 0 { return Err(map_err(rc)); }
            me.n_cols.push(ncols);
        }
        if me.ctxs.is_empty() { return Err(Error::InvalidInstances); }
        let rc = unsafe { h2v_accumulator_create(me.ctxs[0], &mut me.acc) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(me)
    }

    /// `AccumulatorStrategy::with(msm_accumulator)` / `DualMSM::add_msm`: adds the evaluated channels of `msm`, unscaled.
    pub fn add_msm(&mut self, left: &[(Fr, G1Affine)], right: &[(Fr, G1Affine)]) -> Result<(), Error> {
        let ((ls, lb), (rs, rb)) = (flat_terms(left), flat_terms(right));
        let rc = unsafe { h2v_accumulator_add_msm(self.acc, ls.as_ptr(), lb.as_ptr(), left.len(), rs.as_ptr(), rb.as_ptr(), right.len()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }

    /// The trait seam in runs: one Guard per `verify_proof` that ran on the CPU, as the terms `(left, right)` of its `DualMSM`, in
    /// order; every Guard is joined under a fresh OS draw — n x (`DualMSM::scale`, then the Guard's terms; kzg/strategy.rs:125-136,
    /// msm.rs:173-183) in one call (h2v_accumulator_process_guards).  An `Err` leaves the accumulator as it was.
    pub fn process_guards(&mut self, guards: &[(&[(Fr, G1Affine)], &[(Fr, G1Affine)])]) -> Result<(), Error> {
        let (mut lc, mut rc_, mut ls, mut lb, mut rs, mut rb) = (Vec::new(), Vec::new(), Vec::new(), Vec::new(), Vec::new(), Vec::new());
        for (left, right) in guards {
            let ((s0, b0), (s1, b1)) = (flat_terms(left), flat_terms(right));
            lc.push(left.len()); rc_.push(right.len());
            ls.extend(s0); lb.extend(b0); rs.extend(s1); rb.extend(b1);
        }
        let rc = unsafe { h2v_accumulator_process_guards(self.acc, guards.len(), lc.as_ptr(), rc_.as_ptr(), ls.as_ptr(), lb.as_ptr(), rs.as_ptr(), rb.as_ptr(),
                                                         core::ptr::null()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }

    /// The groups of a finished staged batch as legs of this strategy, in group order (h2v_accumulator_process_batch): per group
    /// `DualMSM::scale` by its draws, then the sum of its Guards' terms (kzg/strategy.rs:125-136, msm.rs:173-183) as the launch left it on
    /// the device — what `process` once per group over that group's proofs and draws leaves.  `batch` has finished (`finish` /
    /// `finish_groups` has returned), lives on this device over these params, and is only read.  With the journal on every group leaves
    /// an entry.  Returns `(n_proofs_added, n_failed_added)`.  An `Err` leaves the accumulator as it was.
    pub fn process_batch(&mut self, batch: &GpuStagedBatch) -> Result<(usize, usize), Error> {
        let (mut n, mut f) = (0usize, 0usize);
        let rc = unsafe { h2v_accumulator_process_batch(self.acc, batch.b, &mut n, &mut f) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok((n, f))
    }

    /// `process_batch` ENQUEUED (h2v_accumulator_feed_batch, feed.rs): `batch` is launched or finished; its groups become legs on the
    /// device, behind its launch.  Waits for nothing; the batch may be uploaded again at once.  Counters, journal entries and the
    /// feed's report follow at `settle` — or at any other call on this accumulator, which settles first.
    pub fn feed_batch(&mut self, batch: &GpuStagedBatch) -> Result<(), Error> {
        let rc = unsafe { super::feed::h2v_accumulator_feed_batch(self.acc, batch.b) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }
    /// Waits for the enqueued feeds and commits them -> one report per feed since the last `settle`, in feed order.
    pub fn settle(&mut self) -> Result<Vec<super::feed::FeedReport>, Error> {
        unsafe { super::feed::settle_raw(self.acc) }.map_err(map_err)
    }
    /// (feeds not settled yet, feeds not reported yet): host state only
    pub fn pending(&self) -> Result<(usize, usize), Error> {
        let (mut u, mut r) = (0usize, 0usize);
        let rc = unsafe { super::feed::h2v_accumulator_pending(self.acc, &mut u, &mut r) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok((u, r))
    }

    /// One `verify_proof(&params, vks[key], strategy, &[instances], &mut Blake2bRead::init(proof))` call per item, in order:
    /// `(key, proof, instances)`.  Returns the verdict of every proof of this call (`Ok(())` or the `Error` of its `verify_proof`).
    /// An `Err` of the call itself leaves the accumulator as it was.
    pub fn process(&mut self, items: &[(usize, &[u8], &[&[Fr]])]) -> Result<Vec<Result<(), Error>>, Error> {
        let n = items.len();
        let (mut keys, mut col_lens, mut flats) = (Vec::with_capacity(n), Vec::new(), Vec::with_capacity(n));
        for (key, _, instances) in items {
            if *key >= self.ctxs.len() || instances.len() != self.n_cols[*key] { return Err(Error::InvalidInstances); }
            let mut flat = Vec::with_capacity(32 * instances.iter().map(|c| c.len()).sum::<usize>());
            for col in instances.iter() { for v in col.iter() { flat.extend_from_slice(v.to_repr().as_ref()); } }
            col_lens.extend(instances.iter().map(|c| c.len()));
            keys.push(*key as u32);
            flats.push(flat);
        }
        let ptrs: Vec<*const u8> = items.iter().map(|(_, p, _)| p.as_ptr()).collect();
        let lens: Vec<usize> = items.iter().map(|(_, p, _)| p.len()).collect();
        let iptrs: Vec<*const u8> = flats.iter().map(|i| i.as_ptr()).collect();
        let (mut status, mut ok) = (vec![0i32; n.max(1)], 0i32);
        let rc = unsafe { h2v_accumulator_process(self.acc, self.ctxs.as_ptr(), self.ctxs.len(), keys.as_ptr(), n, ptrs.as_ptr(), lens.as_ptr(), iptrs.as_ptr(),
                                                  self.n_cols.as_ptr(), col_lens.as_ptr(), core::ptr::null(), status.as_mut_ptr(), &mut ok) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(status[..n].iter().map(|&s| if s == 0 { Ok(()) } else { Err(map_err(s)) }).collect())
    }

    /// `strategy.finalize()`: true iff every processed proof was well formed and the single pairing check passes.  The accumulator is
    /// not consumed: processing may go on afterwards.
    pub fn finalize(&mut self) -> Result<bool, Error> {
        let mut ok = 0i32;
        let rc = unsafe { h2v_accumulator_finalize(self.acc, &mut ok, core::ptr::null_mut(), core::ptr::null_mut()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(ok == 1)
    }

    /// Begin (or checkpoint) the leg journal: `capacity` entries, the base included, in `[2, H2V_ACC_JOURNAL_MAX]`; 0 turns it off.
    /// The base is the accumulator as it stands — the `DualMSM` an `AccumulatorStrategy::with` would resume (poly/kzg/strategy.rs:76-78).
    pub fn journal_begin(&mut self, capacity: usize) -> Result<(), Error> {
        if capacity == 1 || capacity > H2V_ACC_JOURNAL_MAX { return Err(Error::InvalidInstances); }
        let rc = unsafe { h2v_accumulator_journal_begin(self.acc, capacity) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }

    /// `DualMSM::check` (poly/kzg/msm.rs:185-203) of every journal entry's own sum, side by side: `(n_proofs, n_failed, pairing_ok)` per
    /// entry, the base first.  Empty with the journal off.
    pub fn check_legs(&mut self) -> Result<Vec<(usize, usize, bool)>, Error> {
        let mut n = 0usize;
        let rc = unsafe { h2v_accumulator_check_legs(self.acc, 0, &mut n, core::ptr::null_mut(), core::ptr::null_mut(), core::ptr::null_mut()) };
        if rc != 0 { return Err(map_err(rc)); }
        let (mut proofs, mut failed, mut ok) = (vec![0usize; n.max(1)], vec![0usize; n.max(1)], vec![0i32; n.max(1)]);
        let rc = unsafe { h2v_accumulator_check_legs(self.acc, n, &mut n, proofs.as_mut_ptr(), failed.as_mut_ptr(), ok.as_mut_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok((0..n).map(|e| (proofs[e], failed[e], ok[e] == 1)).collect())
    }

    /// Take journal entries out again (distinct, none 0, each below the entry count): the accumulator becomes what it would be had the
    /// dropped calls never been made — `DualMSM::scale` and `add_msm` (poly/kzg/msm.rs:173-183) over the kept entries.
    pub fn drop_legs(&mut self, legs: &[usize]) -> Result<(), Error> {
        let rc = unsafe { h2v_accumulator_drop_legs(self.acc, legs.as_ptr(), legs.len()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }

    /// One pairing for several strategies: `(L, R) += sum_k c_k (L_k, R_k)` with a fresh OS draw `c_k` per source, the counters added
    /// (h2v_accumulator_merge) — per source `DualMSM::scale` then `add_msm` (poly/kzg/msm.rs:173-183) on a copy; the sources are not
    /// changed.  With the journal on every source leaves an entry that `check_legs` tests and `drop_legs` takes out.  Returns the
    /// draws used, 32 bytes per source.  At most `H2V_ACC_MERGE_MAX` sources, all on this device and over these params.
    pub fn merge(&mut self, sources: &[&GpuResidentAccumulator]) -> Result<Vec<u8>, Error> {
        if sources.len() > H2V_ACC_MERGE_MAX { return Err(Error::InvalidInstances); }
        let handles: Vec<*mut h2v_accumulator> = sources.iter().map(|s| s.acc).collect();
        let mut draws = vec![0u8; 32 * sources.len().max(1)];
        let rc = unsafe { h2v_accumulator_merge(self.acc, handles.as_ptr(), handles.len(), core::ptr::null(), draws.as_mut_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        draws.truncate(32 * sources.len());
        Ok(draws)
    }

    /// The strategy as `H2V_ACC_STATE_BYTES` bytes (h2v_accumulator_export_state), for a `merge_states` on another device or in
    /// another process.  A state carries no SRS: the importer cannot check it.
    pub fn export_state(&mut self) -> Result<[u8; H2V_ACC_STATE_BYTES], Error> {
        let mut out = [0u8; H2V_ACC_STATE_BYTES];
        let rc = unsafe { h2v_accumulator_export_state(self.acc, out.as_mut_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(out)
    }

    /// `merge` over exported states (h2v_accumulator_merge_states), with fresh OS draws; returns the draws used.
    pub fn merge_states(&mut self, states: &[[u8; H2V_ACC_STATE_BYTES]]) -> Result<Vec<u8>, Error> {
        if states.len() > H2V_ACC_MERGE_MAX { return Err(Error::InvalidInstances); }
        let flat: Vec<u8> = states.iter().flat_map(|s| s.iter().copied()).collect();
        let mut draws = vec![0u8; 32 * states.len().max(1)];
        let rc = unsafe { h2v_accumulator_merge_states(self.acc, flat.as_ptr(), states.len(), core::ptr::null(), draws.as_mut_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        draws.truncate(32 * states.len());
        Ok(draws)
    }
}
impl Drop for GpuResidentAccumulator {
    fn drop(&mut self) {
        unsafe { h2v_accumulator_destroy(self.acc) }   // (the accumulator goes before the context it lives on; null is allowed)
        for &c in &self.ctxs { unsafe { h2v_ctx_destroy(c) } }
    }
}

/// The terms of one `MSMKZG` channel as it holds them (scalars, projective bases; poly/kzg/msm.rs:17-24) in the C ABI's layout.
fn flat_channel(scalars: &[Fr], bases: &[<G1Affine as CurveAffine>::CurveExt]) -> (Vec<u8>, Vec<u8>) {
    let terms: Vec<(Fr, G1Affine)> = scalars.iter().zip(bases.iter()).map(|(s, b)| (*s, b.to_affine())).collect();
    flat_terms(&terms)
}

/// Trait seam: the reference's own `verify_proof` stays the driver on the CPU, and the strategy it is handed is a resident accumulator
/// on the GPU.  `process` is `AccumulatorStrategy::process` (kzg/strategy.rs:125-136) with the scale and the addition on the device:
/// `f` gets an empty `DualMSM::new(params)` and returns its Guard, whose terms go, with a fresh draw, to
/// h2v_accumulator_process_guards — scale (L, R) by the draw, add the Guard's two evaluated channels.  Nothing of the accumulation is
/// kept on the host, and no earlier scalar is touched again.  `finalize` is the one pairing (h2v_accumulator_finalize).
pub struct GpuAccumulatorStrategy<'params> { params: &'params ParamsKZG<Bn256>, ctx: *mut h2v_ctx, acc: *mut h2v_accumulator }

impl<'params> VerificationStrategy<'params, KZGCommitmentScheme<Bn256>, VerifierSHPLONK<'params, Bn256>> for GpuAccumulatorStrategy<'params> {
    type Output = Self;
    fn new(params: &'params ParamsKZG<Bn256>) -> Self {
        let mut pb = Vec::new();
        params.write_custom(&mut pb, SerdeFormat::RawBytes).expect("vec write");
        let mut me = Self { params, ctx: core::ptr::null_mut(), acc: core::ptr::null_mut() };   // (what was made goes with `me` if an assert fails)
        let rc = unsafe { h2v_ctx_create(pb.as_ptr(), pb.len(), H2V_SERDE_RAW_BYTES, core::ptr::null(), 0, 0, 0, &mut me.ctx) };
        assert_eq!(rc, 0, "h2v_ctx_create");
        let rc = unsafe { h2v_accumulator_create(me.ctx, &mut me.acc) };
        assert_eq!(rc, 0, "h2v_accumulator_create");
        me
    }
    fn process(self, f: impl FnOnce(DualMSM<'params, Bn256>) -> Result<GuardKZG<'params, Bn256>, Error>) -> Result<Self, Error> {
        let guard = f(DualMSM::new(self.params))?;   // (an Err drops `self`: the accumulator and the context go with it)
        let msm = &guard.msm_accumulator;
        let (ls, lb) = flat_channel(&msm.left.scalars(), &msm.left.bases());
        let (rs, rb) = flat_channel(&msm.right.scalars(), &msm.right.bases());
        let (nl, nr) = (ls.len() / 32, rs.len() / 32);
        let draw = Fr::random(getrandom_or_panic::getrandom_or_panic()).to_repr();
        let rc = unsafe { h2v_accumulator_process_guards(self.acc, 1, &nl, &nr, ls.as_ptr(), lb.as_ptr(), rs.as_ptr(), rb.as_ptr(), draw.as_ref().as_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(self)
    }
    fn finalize(self) -> bool {
        let mut ok = 0i32;
        let rc = unsafe { h2v_accumulator_finalize(self.acc, &mut ok, core::ptr::null_mut(), core::ptr::null_mut()) };
        rc == 0 && ok == 1
    }
}
impl<'params> Drop for GpuAccumulatorStrategy<'params> {
    fn drop(&mut self) {
        unsafe { h2v_accumulator_destroy(self.acc) }   // (the accumulator goes before the context it lives on; null is allowed)
        if !self.ctx.is_null() { unsafe { h2v_ctx_destroy(self.ctx) } }
    }
}

/// The reference's `MSM<G1Affine>` (poly/commitment.rs:56-79) as `MSMKZG` implements it (poly/kzg/msm.rs:17-95), with the terms resident
/// on the GPU (h2v_msm_*): hold one where a term list lives across calls — a `GuardKZG::msm_accumulator` to manipulate, an
/// `AccumulatorStrategy::with(msm)` to resume, Guards combined under the caller's own scheme.  Where Guards are only fed once, feed them
/// (`GpuResidentAccumulator::process_guards`): that is the faster path.  The trait's methods cannot fail, so a refused call panics with
/// the library's code; `ctx` outlives the object.  Evaluating MANY objects per launch is `GpuMsm::eval_many`.
#[derive(Debug)]
pub struct GpuMsm { ctx: *mut h2v_ctx, m: *mut h2v_msm }
unsafe impl Send for GpuMsm {}
unsafe impl Sync for GpuMsm {}

fn point_from_xy(xy: &[u8]) -> <G1Affine as CurveAffine>::CurveExt {
    if xy.iter().all(|&b| b == 0) { return <G1Affine as CurveAffine>::CurveExt::identity(); }
    let (mut x, mut y) = (<<G1Affine as CurveAffine>::Base as PrimeField>::Repr::default(), <<G1Affine as CurveAffine>::Base as PrimeField>::Repr::default());
    x.as_mut().copy_from_slice(&xy[..32]); y.as_mut().copy_from_slice(&xy[32..64]);
    let (x, y) = (<G1Affine as CurveAffine>::Base::from_repr(x).unwrap(), <G1Affine as CurveAffine>::Base::from_repr(y).unwrap());
    G1Affine::from_xy(x, y).unwrap().to_curve()
}

impl GpuMsm {
    /// `MSMKZG::new()`: no term.
    pub fn new(ctx: *mut h2v_ctx) -> Result<Self, Error> {
        let mut m = core::ptr::null_mut();
        let rc = unsafe { h2v_msm_create(ctx, &mut m) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(Self { ctx, m })
    }
    pub fn len(&self) -> usize {
        let mut n = 0usize;
        let rc = unsafe { h2v_msm_len(self.m, &mut n) };
        assert_eq!(rc, 0, "h2v_msm_len");
        n
    }
    /// `append_term` x n in one call; an `Err` (a base off the curve) leaves the object as it was.
    pub fn append_terms(&mut self, terms: &[(Fr, G1Affine)]) -> Result<(), Error> {
        let (s, b) = flat_terms(terms);
        let rc = unsafe { h2v_msm_append_terms(self.m, s.as_ptr(), b.as_ptr(), terms.len()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }
    /// `eval` for many objects, one pooled launch per 1024 of them: the points and `check` (is the identity) per object.
    pub fn eval_many(msms: &[&GpuMsm]) -> Result<Vec<(<G1Affine as CurveAffine>::CurveExt, bool)>, Error> {
        let hs: Vec<*mut h2v_msm> = msms.iter().map(|m| m.m).collect();
        let (mut xy, mut ident) = (vec![0u8; 64 * hs.len()], vec![0i32; hs.len()]);
        let rc = unsafe { h2v_msm_eval_many(hs.as_ptr(), hs.len(), xy.as_mut_ptr(), ident.as_mut_ptr()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok((0..hs.len()).map(|i| (point_from_xy(&xy[64 * i..64 * i + 64]), ident[i] == 1)).collect())
    }
    pub fn handle(&self) -> *mut h2v_msm { self.m }
}

impl Clone for GpuMsm {
    /// create + add_msm: the copy is independent of its source
    fn clone(&self) -> Self {
        let mut c = GpuMsm::new(self.ctx).expect("h2v_msm_create");
        MSM::<G1Affine>::add_msm(&mut c, self);
        c
    }
}

impl MSM<G1Affine> for GpuMsm {
    fn append_term(&mut self, scalar: Fr, point: <G1Affine as CurveAffine>::CurveExt) {
        self.append_terms(&[(scalar, point.to_affine())]).expect("h2v_msm_append_terms");
    }
    fn add_msm(&mut self, other: &Self) {
        let rc = unsafe { h2v_msm_add_msm(self.m, other.m) };
        assert_eq!(rc, 0, "h2v_msm_add_msm");
    }
    fn scale(&mut self, factor: Fr) {
        let rc = unsafe { h2v_msm_scale(self.m, factor.to_repr().as_ref().as_ptr()) };
        assert_eq!(rc, 0, "h2v_msm_scale");
    }
    fn check(&self) -> bool { GpuMsm::eval_many(&[self]).expect("h2v_msm_eval_many")[0].1 }
    fn eval(&self) -> <G1Affine as CurveAffine>::CurveExt { GpuMsm::eval_many(&[self]).expect("h2v_msm_eval_many")[0].0 }
    fn bases(&self) -> Vec<<G1Affine as CurveAffine>::CurveExt> {
        let n = self.len();
        let mut b = vec![0u8; 64 * n];
        let rc = unsafe { h2v_msm_terms(self.m, 0, n, core::ptr::null_mut(), b.as_mut_ptr()) };
        assert_eq!(rc, 0, "h2v_msm_terms");
        (0..n).map(|i| point_from_xy(&b[64 * i..64 * i + 64])).collect()
    }
    fn scalars(&self) -> Vec<Fr> {
        let n = self.len();
        let mut s = vec![0u8; 32 * n];
        let rc = unsafe { h2v_msm_terms(self.m, 0, n, s.as_mut_ptr(), core::ptr::null_mut()) };
        assert_eq!(rc, 0, "h2v_msm_terms");
        (0..n).map(|i| { let mut r = <Fr as PrimeField>::Repr::default(); r.as_mut().copy_from_slice(&s[32 * i..32 * i + 32]); Fr::from_repr(r).unwrap() }).collect()
    }
}
impl Drop for GpuMsm { fn drop(&mut self) { unsafe { h2v_msm_destroy(self.m) } } }   // (before its context; null is allowed)

/// `DualMSM` (poly/kzg/msm.rs:146-204) over two resident channels.  `check` borrows where the reference consumes: the object may be
/// scaled, extended and checked again.  Many at once: `GpuDualMsm::check_many`.
#[derive(Debug, Clone)]
pub struct GpuDualMsm { pub left: GpuMsm, pub right: GpuMsm }

impl GpuDualMsm {
    pub fn new(ctx: *mut h2v_ctx) -> Result<Self, Error> { Ok(Self { left: GpuMsm::new(ctx)?, right: GpuMsm::new(ctx)? }) }
    pub fn scale(&mut self, e: Fr) { self.left.scale(e); self.right.scale(e); }
    pub fn add_msm(&mut self, other: &Self) {
        MSM::<G1Affine>::add_msm(&mut self.left, &other.left);
        MSM::<G1Affine>::add_msm(&mut self.right, &other.right);
    }
    pub fn check(&self) -> Result<bool, Error> { Ok(Self::check_many(&[self])?[0]) }
    /// `DualMSM::check` for many objects: per 512 of them one pooled MSM over the 2 k channels and one pairing launch.
    pub fn check_many(duals: &[&GpuDualMsm]) -> Result<Vec<bool>, Error> {
        let ls: Vec<*mut h2v_msm> = duals.iter().map(|d| d.left.m).collect();
        let rs: Vec<*mut h2v_msm> = duals.iter().map(|d| d.right.m).collect();
        let mut ok = vec![0i32; duals.len()];
        let rc = unsafe { h2v_dual_msm_check_many(ls.as_ptr(), rs.as_ptr(), duals.len(), ok.as_mut_ptr(), core::ptr::null_mut(), core::ptr::null_mut()) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(ok.iter().map(|&v| v == 1).collect())
    }
}
// (Drop: the two channels' own)

impl GpuResidentAccumulator {
    /// `add_msm` with both channels resident (h2v_accumulator_add_msms): evaluated in one pooled launch, added unscaled.
    pub fn add_msms(&mut self, msm: &GpuDualMsm) -> Result<(), Error> {
        let rc = unsafe { h2v_accumulator_add_msms(self.acc, msm.left.m, msm.right.m) };
        if rc != 0 { return Err(map_err(rc)); }
        Ok(())
    }
}
