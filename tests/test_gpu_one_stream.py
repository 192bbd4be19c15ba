"""A launch lives on ONE stream (csrc/batch.hip): the scalar canonicity check runs in front of the decompression on the launch's own
stream, the multipliers are the upload's, and the end of a launch — whole accumulators, affine bytes, the result block's way to the
host — is done by extra workgroups of the pairing launch.  What must not change:
  * a non-canonical scalar (Fr::from_repr fails, transcript/mod.rs:168-176) at the first, the last and a middle scalar slot of the
    first and the last proof of a group gives that proof the status the CPU oracle gives (which the library gave before the check
    moved), leaves every other proof alone, and the group's accumulators and verdict are the oracle's;
  * eight grouped batches launched back to back on eight caller streams, twice over (the second launch keeps the multipliers and the
    MSM descriptors of the first), and finished in REVERSE order give, batch by batch, exactly what each gives alone."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

GROUPS = 4
PER_GROUP = 6


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 8 * GROUPS * PER_GROUP, seed=31415, threads=16)
    yield s, P, I
    s.free()


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _scalar_slots(s, P, I):
    """the 32-byte slots of a proof that hold scalars: the oracle reads r - 1 there (and rejects it in a point's place)"""
    slots = []
    for k in range(len(P[0]) // 32):
        b = bytearray(P[0]); b[32 * k:32 * k + 32] = (R_MOD - 1).to_bytes(32, "little")
        if circuits.oracle_verify_batch(s, [bytes(b)], I[:1], [1])[1][0] == 0:
            slots.append(k)
    return slots


def _oracle_groups(s, P, I, rand, groups):
    gs = len(P) // groups
    ok, st, left, right = [], [], [], []
    for g in range(groups):
        o = circuits.oracle_verify_batch(s, P[g * gs:(g + 1) * gs], I[g * gs:(g + 1) * gs], rand[g * gs:(g + 1) * gs])
        ok.append(o[0]); st += o[1]; left.append(o[2]); right.append(o[3])
    return ok, st, left, right


# what replaces the scalar: all ones (top word above r's), r itself and r + 1 (top word EQUAL to r's: the check's full comparison),
# and 2^256 - 2^224 + low words of r (top word above, the rest like r)
BAD_VALUES = [(1 << 256) - 1, R_MOD, R_MOD + 1, ((1 << 256) - (1 << 224)) | (R_MOD & ((1 << 224) - 1))]


def test_non_canonical_scalars_get_the_oracles_statuses(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0 = pool
    n = GROUPS * PER_GROUP
    P0, I0 = P0[:n], I0[:n]
    slots = _scalar_slots(s, P0, I0)
    assert len(slots) >= 3
    where = [slots[0], slots[len(slots) // 2], slots[-1]]
    rnd = random.Random(77)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    ctx = _ctx(s)
    b = h2v.Batch(ctx, n, 8, groups=GROUPS)
    cases = [(g, p, k) for g in (0, GROUPS - 1) for p in (0, PER_GROUP - 1) for k in where]
    for i, (g, p, k) in enumerate(cases):
        P = list(P0)
        at = g * PER_GROUP + p
        pb = bytearray(P[at]); pb[32 * k:32 * k + 32] = BAD_VALUES[i % len(BAD_VALUES)].to_bytes(32, "little"); P[at] = bytes(pb)
        flat, inst = _flat(P, I0)
        b.upload(flat, 1024, inst, [8], _rand_bytes(rand))
        b.launch()
        got = b.finish_groups()
        exp = _oracle_groups(s, P, I0, rand, GROUPS)
        assert exp[1][at] == int(h2v.PlonkError.Transcript) and sum(1 for v in exp[1] if v) == 1
        assert got[1] == exp[1], (g, p, k, got[1])
        assert got[0] == exp[0] and got[2] == exp[2] and got[3] == exp[3], (g, p, k)
        assert got[0] == [gg != g for gg in range(GROUPS)]
    # r - 1 in a scalar slot is canonical (its top word equals r's): no status, the pairing rejects the group
    P = list(P0)
    pb = bytearray(P[0]); pb[32 * where[1]:32 * where[1] + 32] = (R_MOD - 1).to_bytes(32, "little"); P[0] = bytes(pb)
    flat, inst = _flat(P, I0)
    b.upload(flat, 1024, inst, [8], _rand_bytes(rand))
    b.launch()
    got = b.finish_groups()
    exp = _oracle_groups(s, P, I0, rand, GROUPS)
    assert got[1] == [0] * n and got == (exp[0], exp[1], exp[2], exp[3]) and got[0][0] is False
    b.close()
    ctx.close()


def test_eight_batches_on_eight_streams_finished_in_reverse(pool):
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    n = GROUPS * PER_GROUP
    ctx = _ctx(s)
    rnd = random.Random(88)
    inputs = []
    for k in range(8):
        Pk, Ik = list(P[k * n:(k + 1) * n]), I[k * n:(k + 1) * n]
        if k % 3 == 1:   # a wrong proof (one bit of an evaluation), in a group of its own choice
            at = (k % GROUPS) * PER_GROUP + k % PER_GROUP
            pb = bytearray(Pk[at]); pb[700] ^= 1; Pk[at] = bytes(pb)
        rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
        if k % 4 == 2:
            rand[(k % GROUPS) * PER_GROUP + 2] = 0   # a zero draw: the two proofs in front of it count for nothing
        inputs.append(_flat(Pk, Ik) + (_rand_bytes(rand),))
    alone = []
    for flat, inst, rb in inputs:
        b = h2v.Batch(ctx, n, 8, groups=GROUPS)
        b.upload(flat, 1024, inst, [8], rb)
        b.launch()
        alone.append(b.finish_groups())
        b.close()
    assert any(not all(a[0]) for a in alone) and any(all(a[0]) for a in alone)
    streams = [torch.cuda.Stream(device=0) for _ in range(8)]
    batches = [h2v.Batch(ctx, n, 8, stream=st.cuda_stream, groups=GROUPS) for st in streams]
    for b, (flat, inst, rb) in zip(batches, inputs):
        b.upload(flat, 1024, inst, [8], rb)
    for rounds in range(2):
        for b in batches:
            b.launch()
        got = [None] * 8
        for k in reversed(range(8)):
            got[k] = batches[k].finish_groups()
        for k in range(8):
            assert got[k] == alone[k], (rounds, k)
    # the ranges of a finished launch are still re-checked on the resident scalars (the launch left them alone)
    oks, lefts, rights = batches[0].recheck([(0, PER_GROUP), (PER_GROUP, PER_GROUP)])
    assert oks == alone[0][0][:2] and lefts == alone[0][2][:2] and rights == alone[0][3][:2]
    for b in batches:
        b.close()
    torch.cuda.synchronize()
    ctx.close()
