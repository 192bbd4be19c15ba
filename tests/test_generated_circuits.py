"""The plan compiler (csrc/vkplan.hip: compile_plan) against the oracle on GENERATED circuits, without a GPU.  The hand-written
families (vector_mul, two_phase_shuffle, wide) leave whole branches of the compiler unreached; oracle/prover.hpp's circuit_generated
draws a circuit's whole shape from a seed — fixed and instance columns in the permutation, rotated instance and fixed queries, advice
rotations out to -(blinding_factors + 1), three phases, challenges of every phase including never-squeezed ones, constant terms,
arbitrary coefficients and exponents, lookups of 1..3 composite expressions, several arguments under two circuit instances, every
relation of chunk to the permutation's size, cs_degree up to 9, unqueried columns, 0..3 instance columns of unequal and zero length.

For each of the 24 pinned cases (tests/generated_cases.py):
  * the oracle's prover and verifier — written independently of each other — agree: the honest proof is accepted, a proof over a
    witness with one wrong result cell is rejected as a constraint failure (not as a transcript or opening error);
  * the VK survives RawBytes -> Processed -> RawBytes byte for byte;
  * tests/cpp/plan_host.hip's race, equivalence and status-order checks of the 2/3/4-stream programs pass;
  * the SINGLE-STREAM program itself is the reference's arithmetic: plan_host --dump writes the compiled plan, verify_reference.vm_run
    interprets plan.code exactly over the proof's scalars, the instance values and the oracle's challenges, and the scalars it stores
    must equal the oracle's Guard term by term — with the instance evaluations unrolled into the program and with them taken from the
    instance kernel's reference (instance_kernel_threshold = 1).  This is the test that localises a compiler fault without a GPU.
The union of the cases' feature masks must cover every bit under SHPLONK and under GWC."""
import ctypes
import os
import struct
import subprocess

import pytest

import circuits
import generated_cases as gc
import verify_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2_verifier_amd", "csrc")
R = circuits.R_MOD
N = len(gc.CASES)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan") / "plan_host"
    cmd = ["hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-o", str(out),
           os.path.join(ROOT, "tests", "cpp", "plan_host.hip"), os.path.join(CSRC, "vkplan.hip"), os.path.join(CSRC, "params.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("hipcc failed: " + r.stderr[-2000:])
    return str(out)


_cases = {}


def case(i):
    """(setup, honest proof, instances) of case i, made once"""
    if i not in _cases:
        s = gc.make_setup(i)
        proof, inst = gc.prove(s, i, 0)
        _cases[i] = (s, proof, inst)
    return _cases[i]


def test_the_pinned_cases_are_24_with_k_5_to_7():
    assert N == 24 and {k for k, _ in gc.CASES} == {5, 6, 7} and len(set(gc.CASES)) == N


@pytest.mark.parametrize("i", range(N), ids=gc.IDS)
def test_oracle_accepts_the_honest_and_rejects_the_tampered_proof(i):
    s, proof, inst = case(i)
    assert circuits.oracle_verify_single(s, proof, inst) == 0
    bad, bad_inst = gc.prove(s, i, 0, tamper=True)
    assert bad_inst == inst and len(bad) == len(proof) and bad != proof
    assert circuits.oracle_verify_single(s, bad, inst) == gc.CONSTRAINT_FAILURE


def test_every_feature_occurs_under_both_multiopen_schemes():
    masks = {circuits.SHPLONK: 0, circuits.GWC: 0}
    for i in range(N):
        masks[gc.INSTANTIATIONS[i % 4][0]] |= case(i)[0].features
    for mo, mask in masks.items():
        missing = [name for name in circuits.GF_NAMES if circuits.GF[name] & circuits.GF_ALL & ~mask]
        assert not missing, f"multiopen {mo}: no pinned case has {missing}"
    assert {case(i)[0].circuit_instances for i in range(N)} == {1, 2}


@pytest.mark.parametrize("i", range(N), ids=gc.IDS)
def test_vk_round_trips_through_the_processed_format(i):
    s = case(i)[0]
    buf = ctypes.create_string_buffer(len(s.vk) + 64)
    n = s.L.h2o_vk_convert(s.vk, len(s.vk), circuits.RAW, 0, buf, len(buf))
    assert 0 < n < len(s.vk)
    processed = buf.raw[:n]
    n = s.L.h2o_vk_convert(processed, len(processed), 0, circuits.RAW, buf, len(buf))
    assert buf.raw[:n] == s.vk


def _files(tmp_path, s):
    vk, params = tmp_path / "vk", tmp_path / "params"
    vk.write_bytes(s.vk); params.write_bytes(s.params)
    return [str(vk), str(params), str(s.multiopen), str(s.transcript), str(s.circuit_instances)]


@pytest.mark.parametrize("i", range(N), ids=gc.IDS)
def test_multi_stream_programs_pass_plan_host(exe, tmp_path, i):
    s, _, inst = case(i)
    lens = [str(len(c)) for c in inst]
    for guard in ([0, 1] if s.multiopen == circuits.GWC else [0]):
        r = subprocess.run([exe] + _files(tmp_path, s) + [str(guard)] + lens, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        ok = [l.split()[0] for l in r.stdout.split("\n") if l.startswith("K=") and " ok:" in l]
        assert ok == ["K=2", "K=3", "K=4"] and "single ok:" in r.stdout


class Dump:
    """plan_host --dump's words (tests/cpp/plan_host.hip)"""
    def __init__(self, data):
        w = struct.unpack(f"<{len(data) // 4}I", data)
        self.w, self.at = w, 0
        assert self.word() == 0x50563248
        self.code = [tuple(self.take(4)) for _ in range(self.word())]
        self.consts = [self.fr() for _ in range(self.word())]
        self.point_offsets, self.scalar_offsets, self.squeeze_order = self.list(), self.list(), self.list()
        self.n_points, self.n_shared = self.word(), self.word()
        self.right_term_order, self.left_term_order, self.guard_term_order = self.terms(), self.terms(), self.terms()
        self.inst_queries = [(self.word(), self.word(), self.fr()) for _ in range(self.word())]
        self.wide_instances, self.proof_len, self.n_challenges, self.x_chal, self.domain_k = (self.word() for _ in range(5))
        assert self.at == len(w)

    def take(self, n):
        self.at += n
        return self.w[self.at - n:self.at]

    def word(self): return self.take(1)[0]
    def list(self): return list(self.take(self.word()))
    def terms(self): return [tuple(self.take(2)) for _ in range(self.word())]
    def fr(self): return sum(x << (32 * j) for j, x in enumerate(self.take(8)))


def _dump(exe, tmp_path, s, inst, guard, threshold):
    out = tmp_path / f"plan_{guard}_{threshold}"
    r = subprocess.run([exe, "--dump", str(out), str(threshold)] + _files(tmp_path, s) + [str(guard)] + [str(len(c)) for c in inst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return Dump(out.read_bytes())


def _interpret(d, proof, inst, oracle_chal):
    """plan.code over this proof, with the oracle's challenges in squeeze order -> (right scalars, left scalars, guard scalars)"""
    ival = lambda b: int.from_bytes(b, "little")
    flat = [ival(v) for col in inst for v in col]
    assert len(set(d.squeeze_order)) == len(d.squeeze_order) and d.n_challenges == len(oracle_chal)
    chal = [ival(oracle_chal[cid]) for cid in d.squeeze_order]     # a challenge that is never squeezed has no position
    insteval = []
    if d.wide_instances:
        n, w = 1 << d.domain_k, vr.omega_of(d.domain_k)
        x = chal[d.x_chal]
        for base, length, w_start in d.inst_queries:
            rot = next(r for r in range(-8, 9) if pow(w, -r % n, R) == w_start)
            insteval.append(vr.instance_eval(flat[base:base + length], rot, x, d.domain_k))
    else:
        assert not d.inst_queries
    env = vr.VmEnv([ival(proof[o:o + 32]) for o in d.scalar_offsets], flat, chal, insteval, 1)
    out = vr.vm_run(d.code, d.consts, env, d.n_points, len(d.guard_term_order), d.n_shared)
    assert out["status"] == 0
    right = [out["shared"][j] if sh else out["msm"][j] for sh, j in d.right_term_order]
    left = [out["left"][j] for _, j in d.left_term_order]
    return right, left, out["guard"]


@pytest.mark.parametrize("threshold", [0, 1], ids=["program", "instance-kernel"])
@pytest.mark.parametrize("i", range(N), ids=gc.IDS)
def test_single_stream_program_computes_the_oracles_guard(exe, tmp_path, i, threshold):
    s, proof, inst = case(i)
    rc, g = circuits.oracle_guard(s, proof, inst)
    assert rc == 0
    ival = lambda b: int.from_bytes(b, "little")
    want_right, want_left = [ival(x) for x in g["right_scalars"]], [ival(x) for x in g["left_scalars"]]
    d = _dump(exe, tmp_path, s, inst, 0, threshold)
    assert d.proof_len == len(proof)
    assert bool(d.wide_instances) == (threshold == 1 and sum(len(c) for c in inst) > 0)
    right, left, _ = _interpret(d, proof, inst, g["challenges"])
    assert left == want_left
    if s.multiopen == circuits.SHPLONK:
        assert right == want_right
    else:
        # the oracle repeats a commitment once per query (gwc.rs:96-116); the MSM carries it once, scalars summed, at its first appearance
        summed = {}
        for sc, base in zip(want_right, g["right_bases"]):
            summed[base] = (summed.get(base, 0) + sc) % R
        assert right == list(summed.values())
        dg = _dump(exe, tmp_path, s, inst, 1, threshold)
        right_g, left_g, guard = _interpret(dg, proof, inst, g["challenges"])
        assert guard == want_right and (right_g, left_g) == (right, left)
