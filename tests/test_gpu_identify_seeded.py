"""Which proofs made a SEEDED batch fail (h2v_verify_batch_seeded_identify: Context.verify_batch_identify(seed=...),
AccumulatorStrategy.with_accumulator(...).finalize_identify()).  The seed's terms belong to no proof: the statuses are, proof for proof,
what SingleStrategy gives for this call's proofs, the seed's own verdict is reported beside them, and the batch's result stays
h2v_verify_batch_seeded's.  The bad proofs decode and pass the transcript: only the pairing rejects them."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 256, seed=9173, threads=16)
    ctx = _ctx(s)
    yield s, P, I, ctx
    ctx.close()
    s.free()


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript)


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _neg(pt):
    b = bytearray(pt); b[31] ^= 0x40   # the sign bit of a compressed G1 point: -P
    return bytes(b)


def _make_bad(P, I, i, kind):
    """Proof i made pairing-only bad (decodes, transcript clean) in one of four ways.  -> (proof, instances)"""
    p, inst = bytearray(P[i]), [list(c) for c in I[i]]
    other = P[(i + 1) % len(P)] if P[(i + 1) % len(P)] != P[i] else P[(i + 2) % len(P)]
    if kind == 0:     # a wrong public input
        v = (int.from_bytes(inst[0][0], "little") + 1) % R_MOD
        inst[0][0] = v.to_bytes(32, "little")
    elif kind == 1:   # the sign of h2 flipped
        p[-1] ^= 0x40
    elif kind == 2:   # the first commitment is another proof's
        p[0:32] = other[0:32]
    else:             # ... and its negation
        p[0:32] = _neg(other[0:32])
    return bytes(p), inst


def _spoil(P, I, bad, early=()):
    """Copies of (P, I) with pairing-only bad proofs at `bad` (kinds in turn) and early failures (x >= p) at `early`"""
    P, I = list(P), list(I)
    for k, i in enumerate(sorted(bad)):
        P[i], I[i] = _make_bad(P, I, i, k % 4)
    for i in early:
        b = bytearray(P[i]); b[-33] = 0xff; P[i] = bytes(b)   # top byte of h1: x >= p
    return P, I



def _halves(pool, bad, seed=73, n=64):
    s, P0, I0, ctx = pool
    P, I = _spoil(P0[:n], I0[:n], bad)
    rnd = random.Random(seed)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    h = n // 2
    _, st, L, R = ctx.verify_batch(P[:h], I[:h], rand[:h])
    assert st == [0] * h
    return P, I, rand, h, (([1], [L]), ([1], [R]))


def test_bad_proofs_in_the_seeded_half(pool):
    s, _, _, ctx = pool
    bad = [32, 40, 63]
    P, I, rand, h, seed = _halves(pool, bad)
    ok, st, left, right = ctx.verify_batch_identify(P[h:], I[h:], rand[h:], seed=seed)
    assert (ok, st.count(0) + st.count(-2)) == (False, h)
    ref = ctx.verify_batch(P[h:], I[h:], rand[h:], seed=seed)
    assert (ok, left, right) == (ref[0], ref[2], ref[3])
    assert (ok, left, right) == tuple(circuits.oracle_verify_batch(s, P, I, rand)[k] for k in (0, 2, 3))   # resumed == one batch over both halves
    assert st == ctx.verify_each(P[h:], I[h:]) == [-2 if h + i in bad else 0 for i in range(h)]
    for i in bad:
        assert circuits.oracle_verify_single(s, P[i], I[i]) == -2
    assert ctx.last_seed_ok is True and ctx.last_range_checks > 0


def test_a_failing_seed_is_no_proofs_fault(pool):
    s, _, _, ctx = pool
    P, I, rand, h, seed = _halves(pool, [7], seed=79)
    assert circuits.oracle_pairing_check(s, seed[0][1][0], seed[1][1][0]) is False
    ok, st, left, right = ctx.verify_batch_identify(P[h:], I[h:], rand[h:], seed=seed)
    ref = ctx.verify_batch(P[h:], I[h:], rand[h:], seed=seed)
    assert (ok, left, right) == (ref[0], ref[2], ref[3]) and ok is False
    assert st == [0] * h == [circuits.oracle_verify_single(s, p, i) for p, i in zip(P[h:], I[h:])]
    assert ctx.last_seed_ok is False and ctx.last_range_checks == 0


def test_an_empty_seed(pool):
    s, _, _, ctx = pool
    P, I, rand, h, _ = _halves(pool, [35], seed=83)
    empty = (([], []), ([], []))
    ok, st, left, right = ctx.verify_batch_identify(P[h:], I[h:], rand[h:], seed=empty)
    ref = ctx.verify_batch_identify(P[h:], I[h:], rand[h:])
    assert (ok, st, left, right) == ref and st == [-2 if h + i == 35 else 0 for i in range(h)]
    assert (ok, left, right) == tuple(circuits.oracle_verify_batch(s, P[h:], I[h:], rand[h:])[k] for k in (0, 2, 3))
    assert ctx.last_seed_ok is True
    # a passing batch: nothing to search
    ok, st, _, _ = ctx.verify_batch_identify(P[h + 4:], I[h + 4:], rand[h + 4:], seed=empty)
    assert ok is True and st == [0] * (h - 4) and ctx.last_range_checks == 0


def test_zero_draws_are_refused(pool):
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    P, I, rand, h, seed = _halves(pool, [], seed=89, n=16)
    rand[h + 2] = 0
    with pytest.raises(h2v.H2VError) as e:
        ctx.verify_batch_identify(P[h:], I[h:], rand[h:], seed=seed)
    assert e.value.code == -16
    assert ctx.verify_batch(P[h:], I[h:], rand[h:], seed=seed)[1] == [0] * h   # (the plain seeded call takes them)


def test_the_strategy_mirror(pool):
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    bad = [50]
    P, I, rand, h, seed = _halves(pool, bad, seed=97)
    params, vk = h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes)
    strat = h2v.AccumulatorStrategy.with_accumulator(params, seed[0], seed[1], rand=rand[h:])
    for p, i in zip(P[h:], I[h:]):
        strat = h2v.verify_proof(params, vk, strat, i, p)
    assert strat.finalize_identify() is False
    assert strat.statuses == [-2 if h + i in bad else 0 for i in range(h)]
    assert strat.last_seed_ok is True and strat.last_range_checks > 0
    full = circuits.oracle_verify_batch(s, P, I, rand)
    assert (strat.left_xy, strat.right_xy) == (full[2], full[3])
    # several keys with a seed stay refused, as finalize() refuses them
    s4 = circuits.setup_vector_mul(8, 4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 1, seed=5, threads=1)
    strat = h2v.verify_proof(params, h2v.VerifyingKey(s4.vk, h2v.SerdeFormat.RawBytes), strat, I4[0], P4[0])
    strat.rand = None
    with pytest.raises(ValueError):
        strat.finalize_identify()
    with pytest.raises(ValueError):
        strat.finalize()
    s4.free()
