"""Which proofs made a batch fail: h2v_verify_batch_identify (batch, then a search over ranges re-checked on the resident scalars) and
h2v_batch_recheck (the pairing check of arbitrary ranges of a finished launch).  Identification must give, proof for proof, what
SingleStrategy gives (h2v_verify_each, the CPU oracle), leave the batch's own result exactly as h2v_verify_batch gives it, and a
re-checked range must be bit for bit the oracle's AccumulatorStrategy over that range.  The bad proofs decode and pass the transcript:
only the pairing rejects them."""
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


def _cycle(P, I, n):
    return [P[i % len(P)] for i in range(n)], [I[i % len(I)] for i in range(n)]


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
    """Copies of (P, I) with pairing-only bad proofs at `bad` (kinds in turn) and early failures at `early`: x >= p, a short proof."""
    P, I = list(P), list(I)
    for k, i in enumerate(sorted(bad)):
        P[i], I[i] = _make_bad(P, I, i, k % 4)
    for k, i in enumerate(sorted(early)):
        if k % 2 == 0:
            b = bytearray(P[i]); b[-33] = 0xff; P[i] = bytes(b)   # top byte of h1: x >= p
        else:
            P[i] = P[i][:500]                                     # the reader runs dry
    return P, I


def test_bad_proofs_are_rejected_by_the_pairing_only(pool):
    s, P, I, _ = pool
    for kind in range(4):
        p, inst = _make_bad(P, I, 5, kind)
        assert circuits.oracle_verify_single(s, p, inst) == -2, kind


@pytest.mark.parametrize("case", ["none", "first", "last", "adjacent", "scattered7", "scattered33", "all64"])
def test_identify_equals_single_strategy(pool, case):
    s, P0, I0, ctx = pool
    n = 64 if case == "all64" else 1024
    rnd = random.Random(sum(map(ord, case)))
    bad = {"none": [], "first": [0], "last": [n - 1], "adjacent": [500, 501], "scattered7": rnd.sample(range(n), 7),
           "scattered33": rnd.sample(range(n), 33), "all64": list(range(64))}[case]
    free = [i for i in range(n) if i not in bad]
    early = rnd.sample(free, {"adjacent": 2, "scattered7": 1}.get(case, 0))   # x >= p; a short proof (adjacent only: the oracle's batch takes equal lengths)
    P, I = _spoil(*_cycle(P0, I0, n), bad, early)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    ok, st, left, right = ctx.verify_batch_identify(P, I, rand)
    checks = ctx.last_range_checks
    assert st == ctx.verify_each(P, I)
    for i in bad:
        assert st[i] == -2 == circuits.oracle_verify_single(s, P[i], I[i])
    assert [i for i in range(n) if st[i] == -2] == sorted(bad)
    ref = ctx.verify_batch(P, I, rand)
    assert (ok, left, right) == (ref[0], ref[2], ref[3])
    assert [i for i in range(n) if ref[1][i]] == [i for i in range(n) if st[i] not in (0, -2)] == sorted(early)
    assert ok == (not bad and not early)
    if case == "none":
        assert checks == 0
    if case in ("first", "last"):
        assert 0 < checks <= 64   # 32 pieces of 32, then the failing piece's 32 proofs
    if case == "scattered7":
        assert (ok, left, right) == tuple(circuits.oracle_verify_batch(s, P, I, rand)[k] for k in (0, 2, 3))


def _staged(ctx, P, I, rand, groups=1):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, len(P), 8, groups=groups)
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    b.launch()
    return b


def test_rechecked_ranges_equal_the_oracle(pool):
    s, P0, I0, ctx = pool
    n, cut = 64, 40
    rnd = random.Random(7)
    ranges = [(0, 64), (39, 1), (5, 40), (30, 20), (63, 1), (45, 3), (41, 1), (40, 24)]
    for bad in ([], [42]):
        P, I = _spoil(P0[:n], I0[:n], bad)
        rand = [rnd.randrange(1, R_MOD) for _ in range(cut)] + [1] * (n - cut)   # every range ends at or after `cut`: the draws after it are 1
        b = _staged(ctx, P, I, rand)
        b.finish()
        oks, lefts, rights = b.recheck(ranges)
        for (f, c), ok, l, r in zip(ranges, oks, lefts, rights):
            assert (ok, l, r) == tuple(circuits.oracle_verify_batch(s, P[f:f + c], I[f:f + c], rand[f:f + c])[k] for k in (0, 2, 3)), (f, c)
            assert ok == (not any(f <= i < f + c for i in bad))
        # random draws: the verdicts
        rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
        flat, inst = _flat(P, I)
        b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
        b.launch()
        b.finish()
        many = [(f, c) for f in range(0, n, 3) for c in (1, 2, 7) if f + c <= n]
        oks, _, _ = b.recheck(many)
        assert oks == [not any(f <= i < f + c for i in bad) for f, c in many]
        b.close()


def test_grouped_launch(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0, ctx = pool
    G, gs = 4, 64
    P, I = _spoil(P0[:G * gs], I0[:G * gs], [2 * gs + 17])
    rnd = random.Random(11)
    rand = [rnd.randrange(1, R_MOD) for _ in range(G * gs)]
    b = _staged(ctx, P, I, rand, groups=G)
    ok, st, _, _ = b.finish_groups()
    assert ok == [True, True, False, True] and st == [0] * (G * gs)
    ranges = [(0, 64), (64, 64), (192, 64), (128, 64), (128, 16), (144, 16), (145, 1), (146, 5), (130, 16)]
    oks, _, _ = b.recheck(ranges)
    assert oks == [True, True, True, False, True, False, False, True, False]
    for bad_range in ([(120, 16)], [(0, 65)], [(250, 7)], [(3, 0)]):
        with pytest.raises(h2v.H2VError) as e:
            b.recheck(bad_range)
        assert e.value.code == -16
    b.close()


def test_the_launch_results_survive_a_recheck(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0, ctx = pool
    G, gs = 2, 32
    P, I = _spoil(P0[:G * gs], I0[:G * gs], [40])
    rnd = random.Random(13)
    rand = [rnd.randrange(1, R_MOD) for _ in range(G * gs)]
    b = h2v.Batch(ctx, G * gs, 8, groups=G)
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    with pytest.raises(h2v.H2VError):
        b.recheck([(0, 4)])            # nothing launched
    b.launch()
    with pytest.raises(h2v.H2VError):
        b.recheck([(0, 4)])            # launched, not finished
    first = b.finish_groups()
    oks, lefts, rights = b.recheck([(0, 32), (32, 32), (40, 1)])
    assert oks == [True, False, False]
    assert (lefts[:2], rights[:2]) == (first[2], first[3])   # a whole group re-checked is the launch's own accumulation
    assert b.finish_groups() == first
    b.launch()
    assert b.finish_groups() == first
    assert b.recheck([(0, 32), (32, 32), (40, 1)]) == (oks, lefts, rights)
    b.close()


def test_zero_draw(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0, ctx = pool
    n = 64
    P, I = list(P0[:n]), list(I0[:n])
    rnd = random.Random(17)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    rand[10] = 0                       # zeroes the multipliers of proofs 0 .. 9
    b = _staged(ctx, P, I, rand)
    b.finish()
    for r in ([(0, 5)], [(9, 1)], [(5, 20)]):
        with pytest.raises(h2v.H2VError) as e:
            b.recheck(r)
        assert e.value.code == -16
    oks, _, _ = b.recheck([(10, 5), (10, 54)])
    assert oks == [True, True]
    b.close()
    with pytest.raises(h2v.H2VError) as e:
        ctx.verify_batch_identify(P, I, rand)
    assert e.value.code == -16


def test_gwc_keccak_plan():
    s = circuits.setup_vector_mul(8, 8).set_options(circuits.GWC, circuits.KECCAK256)
    P0, I0 = circuits.prove_vector_mul_batch(s, 48, seed=23, threads=8)
    ctx = _ctx(s)
    P, I = list(P0), list(I0)
    for i, kind in ((3, 0), (17, 2), (30, 3)):
        P[i], I[i] = _make_bad(P0, I0, i, kind)
    b = bytearray(P[8]); b[-1] ^= 0x40; P[8] = bytes(b)        # last opening point: sign flipped
    b = bytearray(P[21]); b[-33] = 0xff; P[21] = bytes(b)      # top byte of the second-to-last point: x >= p
    rnd = random.Random(29)
    rand = [rnd.randrange(1, R_MOD) for _ in range(48)]
    ok, st, left, right = ctx.verify_batch_identify(P, I, rand)
    assert st == ctx.verify_each(P, I) == [circuits.oracle_verify_single(s, p, i) for p, i in zip(P, I)]
    assert [st[i] for i in (3, 8, 17, 30)] == [-2] * 4
    ref = ctx.verify_batch(P, I, rand)
    assert (ok, left, right) == (ref[0], ref[2], ref[3])
    ctx.close(); s.free()


def test_lookup_and_shuffle_circuits():
    s = circuits.setup_wide(8, A=8, F=5, L_=1, Sh=1, deg=3)
    ctx = _ctx(s)
    good, inst = circuits.prove_wide(s, witness_seed=3)
    bad, inst_b = circuits.prove_wide(s, witness_seed=3, tamper=True)
    P = [good, bad, good, good, good, bad, good, good, good, good, good, bad]
    I = [inst_b if p == bad else inst for p in P]
    rnd = random.Random(31)
    rand = [rnd.randrange(1, R_MOD) for _ in range(len(P))]
    ok, st, _, _ = ctx.verify_batch_identify(P, I, rand)
    assert not ok and st == ctx.verify_each(P, I) == [-2 if p == bad else 0 for p in P]
    ctx.close(); s.free()
    s = circuits.setup_shuffle(8, 4, 32)
    ctx = _ctx(s)
    good, inst = circuits.prove_shuffle(s, data_seed=5)
    bad, _ = circuits.prove_shuffle(s, data_seed=5, break_it=True)
    P = [good] * 9 + [bad] + [good] * 6
    ok, st, _, _ = ctx.verify_batch_identify(P, [inst] * len(P), [rnd.randrange(1, R_MOD) for _ in P])
    assert not ok and st == ctx.verify_each(P, [inst] * len(P)) == [-2 if p == bad else 0 for p in P]
    ctx.close(); s.free()
