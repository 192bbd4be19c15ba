"""The GPU path on the generated circuits of tests/generated_cases.py (oracle/prover.hpp: circuit_generated): every plan the compiler
makes for them — fixed and instance columns in the permutation, rotated instance and fixed queries, three phases, never-squeezed
challenges, lookups of 1..3 composite expressions, every chunk / cs_degree relation, 0..3 instance columns — must give the oracle's
Guard, statuses and accumulator points.  tests/test_generated_circuits.py holds the same cases on the CPU (the oracle's prover and
verifier agree on them; the single-stream program equals the oracle's Guard), so a failure here and not there points at the kernels or
the multi-stream schedule, one in both at the compiler."""
import random

import pytest

import circuits
import generated_cases as gc

pytestmark = pytest.mark.gpu
R_MOD = circuits.R_MOD
N = len(gc.CASES)


def _ctx(s, **kw):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances, **kw)


@pytest.mark.parametrize("i", range(N), ids=gc.IDS)
def test_generated_circuit_matches_the_oracle(i):
    s = gc.make_setup(i)
    rnd = random.Random(7000 + i)
    pairs = [gc.prove(s, i, w) for w in range(6)] + [gc.prove(s, i, 6, tamper=True), gc.prove(s, i, 7)]
    P, I = [p for p, _ in pairs], [inst for _, inst in pairs]
    b = bytearray(P[7]); pos = rnd.randrange(len(b)); b[pos] ^= 1 << rnd.randrange(8); P[7] = bytes(b)   # an honest proof with one flipped bit
    ctx = _ctx(s)
    # the Guard of an honest proof, term for term, and the challenges (a never-squeezed user challenge is zero)
    rc, got = ctx.guard_msm(P[0], I[0])
    erc, exp = circuits.oracle_guard(s, P[0], I[0])
    assert rc == 0 and erc == 0
    for key in ("challenges", "right_scalars", "right_bases", "left_scalars", "left_bases"):
        assert got[key] == exp[key], key
    if s.features & circuits.GF["CHALLENGE_UNSQUEEZED"]:
        assert b"\0" * 32 in exp["challenges"]
    each = ctx.verify_each(P, I)
    assert each == [circuits.oracle_verify_single(s, p, inst) for p, inst in zip(P, I)]
    assert each[:6] == [0] * 6 and each[6] == gc.CONSTRAINT_FAILURE and each[7] != 0
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    exp_batch = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp_batch[0] is False and ctx.verify_batch(P, I, rand) == exp_batch
    exp_good = circuits.oracle_verify_batch(s, P[:6], I[:6], rand[:6])
    assert exp_good[0] is True and ctx.verify_batch(P[:6], I[:6], rand[:6]) == exp_good
    ctx.close()
    if sum(s.col_lens) > 0:   # the same batches with the instance evaluations from k_instance_eval (rotated instance queries: w_start)
        ctx = _ctx(s, instance_kernel_threshold=1)
        assert ctx.verify_batch(P, I, rand) == exp_batch
        assert ctx.verify_batch(P[:6], I[:6], rand[:6]) == exp_good
        ctx.close()
    s.free()


def test_one_accumulator_takes_the_proofs_of_all_k6_keys():
    """N x verify_proof on ONE AccumulatorStrategy over the generated keys that share params (the k = 6 cases under one known-s SRS): keys of
    both multi-open schemes, both transcripts and 1 or 2 circuit instances in one pairing (h2v_verify_batch_keys), against the oracle's
    Guards folded with the same draws."""
    import halo2_verifier_amd as h2v
    idx = [i for i, (k, _) in enumerate(gc.CASES) if k == 6]
    assert len(idx) == 8
    setups = [gc.make_setup(i) for i in idx]
    assert all(s.params == setups[0].params for s in setups) and len({s.vk for s in setups}) == len(setups)
    ctxs = [_ctx(s) for s in setups]
    items, key_of_proof = [], []
    for w in range(2):
        for key, (i, s) in enumerate(zip(idx, setups)):
            proof, inst = gc.prove(s, i, 10 + w)
            items.append((s, proof, inst)); key_of_proof.append(key)
    rnd = random.Random(66)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True and exp[1] == [0] * len(items)
    assert h2v.verify_batch_keys(ctxs, key_of_proof, [p for _, p, _ in items], [inst for _, _, inst in items], rand) == exp
    # one tampered proof among them
    s, i = setups[3], idx[3]
    bad = list(items)
    bad[3] = (s,) + gc.prove(s, i, 10, tamper=True)
    exp = circuits.oracle_accumulate(bad, rand)
    assert exp[0] is False
    assert h2v.verify_batch_keys(ctxs, key_of_proof, [p for _, p, _ in bad], [inst for _, _, inst in bad], rand) == exp
    for c in ctxs:
        c.close()
    for s in setups:
        s.free()
