"""The pooled batch path under PROGRAMMED draws, bit for bit against the exact linear reference (tests/batch_reference.py).

Uniform random draws never make the pooled multi-problem MSM meet a term repeated many times or beside its negation in one bucket, a
bucket spread over many chunks (the team and heavy fix-ups of a multi-problem launch), empty upper windows, zero multipliers, or window
sums, accumulator pieces and whole accumulators equal to the identity (k_pair_lines, the whole-point pairing, the affine conversion, the
sharded fold).  Programmed draws do: under SHPLONK the left-channel scalars of a batch ARE its multipliers (suffix products of the
draws), so draws_for() puts chosen scalars into the pooled left MSM.  Patterns:
  random        uniform draws (control)
  ones          every multiplier 1: distinct proofs -> every left entry in one bucket of window 0; one proof repeated -> every term of
                the right channel n times, buckets spanning many chunks
  alternating   every draw r - 1 (multipliers +-1): adjacent duplicated pairs cancel -> identity accumulators, verdict True
  zero_at k     a zero draw: the proofs before k drop out
  programmed    multipliers = edge scalars of the GLV split and the signed recoding, each several times
Every case compares (ok, statuses, left, right) of every group with the reference AND asserts that it reached what it was built for
(identity accumulators are 64 zero bytes, the designed verdict, the programmed multipliers), so a wrong reference cannot make it vacuous."""
import random

import pytest

import batch_reference as br
import circuits
import oracle_lib
from circuits import R_MOD

pytestmark = pytest.mark.gpu

POOL = 1024


@pytest.fixture(scope="module")
def pool():
    """1024 distinct proofs of the bench VK shape, and one Context on them"""
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, POOL, seed=20263, threads=16)
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


def _rb(draws):
    return b"".join(int(d).to_bytes(32, "little") for d in draws)


def _neg(pt):
    b = bytearray(pt); b[31] ^= 0x40   # the sign bit of a compressed G1 point: -P
    return bytes(b)


def _case(kind, n, seed=0, start=0):
    """(proof indices into the pool, draws, designed verdict, designed identity) of one group of n proofs"""
    distinct = [(start + i) % POOL for i in range(n)]
    if kind == "random":
        return distinct, br.pattern_draws("random", n, seed), True, False
    if kind == "ones":
        return distinct, br.pattern_draws("ones", n), True, False
    if kind == "ones_repeated":
        return [start % POOL] * n, br.pattern_draws("ones", n), True, False
    if kind == "alternating":
        return distinct, br.pattern_draws("alternating", n), True, False
    if kind == "alternating_pairs":
        assert n % 2 == 0
        return [(start + i // 2) % POOL for i in range(n)], br.pattern_draws("alternating", n), True, True
    if kind.startswith("zero_at_"):
        k = {"1": 1, "half": n // 2, "last": n - 1}[kind[len("zero_at_"):]]
        return distinct, br.pattern_draws("zero_at", n, seed, k=k), True, False
    if kind == "programmed":
        return distinct, br.pattern_draws("programmed", n, seed), True, False
    raise ValueError(kind)


def _check(got, exp, verdict=None, identity=False):
    """got == exp bit for bit, and the case reached its design"""
    assert got == exp
    ok, st, left, right = got
    if verdict is not None:
        assert ok is verdict
    if identity:
        assert left == right == br.ZERO
    else:
        assert left != br.ZERO


def _batch(ctx, P, I, draws, groups=1, via="upload"):
    import halo2_verifier_amd as h2v
    n = len(P)
    b = h2v.Batch(ctx, n, 8, groups=groups)
    flat, inst = _flat(P, I)
    if via == "upload":
        b.upload(flat, len(P[0]), inst, [8], _rb(draws))
        b.launch()
    else:
        b.upload_launch(flat, len(P[0]), inst, [8], _rb(draws))
    return b


def _run(ctx, P, I, draws, via):
    if via == "verify_batch":
        return ctx.verify_batch(P, I, draws)
    b = _batch(ctx, P, I, draws, via=via)
    try:
        return b.finish()
    finally:
        b.close()


def _kinds(n):
    k = ["random", "ones", "ones_repeated", "alternating", "programmed"]
    if n % 2 == 0:
        k.append("alternating_pairs")
    if n >= 3:
        k += ["zero_at_1", "zero_at_half", "zero_at_last"]
    return k


@pytest.mark.parametrize("n", [1, 2, 3, 64, 1024, 1025])
@pytest.mark.parametrize("via", ["verify_batch", "upload", "upload_launch"])
def test_one_group_every_pattern(pool, n, via):
    s, P, I, ctx = pool
    for kind in _kinds(n):
        idx, draws, verdict, ident = _case(kind, n, seed=n, start=3 * n)
        Pn, In = [P[i] for i in idx], [I[i] for i in idx]
        exp = br.expected([(s, P[i], I[i]) for i in idx], draws)
        _check(_run(ctx, Pn, In, draws, via), exp, verdict, ident)
        if kind == "programmed":
            assert br.multipliers(draws) == br.programmed_multipliers(n, offset=n)
        if kind == "zero_at_1" and via == "verify_batch":
            assert br.multipliers(draws)[:1] == [0] and all(br.multipliers(draws)[1:])
        if kind == "random" and via == "verify_batch":
            z = [0] + draws[1:]            # the first draw scales nothing: zero there gives the same result
            assert ctx.verify_batch(Pn, In, z) == exp


def test_cut_problems_of_an_8192_proof_batch(pool):
    """8192 proofs: the problems are cut into sub-problems and merged again (msm_merge_windows); one proof repeated with every
    multiplier 1 skews every sub-problem."""
    s, P, I, ctx = pool
    n = 8192
    for kind in ("ones_repeated", "programmed", "alternating_pairs"):
        idx, draws, verdict, ident = _case(kind, n, seed=5, start=77)
        exp = br.expected([(s, P[i], I[i]) for i in idx], draws)
        _check(ctx.verify_batch([P[i] for i in idx], [I[i] for i in idx], draws), exp, verdict, ident)


def _grouped(pool, kinds, gs, via="upload"):
    """One grouped launch, group g built as kinds[g]: the results against the reference per group, and each group's design"""
    s, P, I, ctx = pool
    G = len(kinds)
    idx, draws, designs = [], [], []
    for g, kind in enumerate(kinds):
        i, d, v, z = _case(kind, gs, seed=g, start=37 * g)
        idx += i; draws += d; designs.append((v, z))
    b = _batch(ctx, [P[i] for i in idx], [I[i] for i in idx], draws, groups=G, via=via)
    got = b.finish_groups()
    b.close()
    exp = br.expected_groups([(s, P[i], I[i]) for i in idx], draws, G)
    for g, (v, z) in enumerate(designs):
        _check((got[0][g], got[1][g * gs:(g + 1) * gs], got[2][g], got[3][g]), (exp[0][g], exp[1][g * gs:(g + 1) * gs], exp[2][g], exp[3][g]), v, z)
    return got


def test_grouped_patterns_do_not_leak(pool):
    _grouped(pool, ["alternating_pairs", "random", "zero_at_half", "programmed"], 256)
    _grouped(pool, ["programmed", "alternating_pairs", "ones_repeated", "alternating_pairs"], 256, via="upload_launch")


MIX = ["alternating_pairs", "random", "ones_repeated", "zero_at_half", "programmed", "ones", "alternating", "zero_at_last"]


@pytest.mark.parametrize("G,gs", [(24, 1024),    # one wave per window, Fr program as two streams
                                  (66, 256)])    # more than 64 groups: whole accumulators, whole-point pairing
def test_throughput_launch_shapes_with_patterns(pool, G, gs):
    _grouped(pool, [MIX[g % len(MIX)] for g in range(G)], gs)


KNOBS = [dict(pairing_one_stream=1), dict(frvm_streams=1), dict(pairing_one_stream=1, frvm_streams=1), dict(frvm_streams=2), dict(frvm_streams=3),
         dict(frvm_streams=2, frvm_lds_kb=36), dict(frvm_streams=4, frvm_lds_kb=78), dict(msm_global_sort=1), dict(msm_parts=1, frvm_streams=1),
         dict(msm_window_threads=64, msm_window_slots=3), dict(msm_window_threads=64, msm_window_wpw=2), dict(msm_window_threads=128, msm_window_wpw=2),
         dict(msm_window_threads=256),
         dict(msm_parts=1), dict(msm_parts=2), dict(msm_parts=6), dict(msm_no_term_split=1)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_tuning_variants(pool, knobs):
    s, P, I, ctx = pool
    ctx.set_tuning(**knobs)
    try:
        for n in (64, 1024):
            for kind in ("alternating_pairs", "ones_repeated", "programmed"):
                idx, draws, verdict, ident = _case(kind, n, seed=1, start=n)
                exp = br.expected([(s, P[i], I[i]) for i in idx], draws)
                _check(ctx.verify_batch([P[i] for i in idx], [I[i] for i in idx], draws), exp, verdict, ident)
    finally:
        ctx.set_tuning()


def test_replaced_commitments_meet_their_negation(pool):
    """Commitments replaced by another proof's and by its negation (kinds 2 and 3 of test_gpu_identify._make_bad): P and -P in one
    bucket of one pooled problem with equal scalars.  Only the pairing rejects."""
    s, P, I, ctx = pool
    n = 64
    for kind in ("ones", "alternating", "ones_repeated"):
        idx, draws, _, _ = _case(kind, n, start=500)
        Pn, In = [P[i] for i in idx], [I[i] for i in idx]
        for j, bad in enumerate((5, 6, 40, 41)):
            p = bytearray(Pn[bad])
            other = P[(idx[bad] + 1) % POOL]
            p[0:32] = other[0:32] if j % 2 == 0 else _neg(other[0:32])
            Pn[bad] = bytes(p)
        exp = br.expected([(s, p, i) for p, i in zip(Pn, In)], draws)
        _check(ctx.verify_batch(Pn, In, draws), exp, False)
        assert exp[1] == [0] * n


def test_per_proof_shapes(pool):
    """h2v_verify_batch_shapes (the gathered-multiplier path): per-proof instance lengths, a cancelling pattern and a programmed one"""
    s, _, _, ctx = pool
    lens = [8, 5, 0, 3]
    rnd = random.Random(9)
    Pd, Id = [], []
    for j in range(16):
        m = lens[j % 4]
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=900 + j)
        Pd.append(p); Id.append(inst)
    n = 64
    pairs = [(i // 2) % 16 for i in range(n)]
    for idx, draws, ident in ((pairs, br.pattern_draws("alternating", n), True), ([i % 16 for i in range(n)], br.pattern_draws("programmed", n, 2), False)):
        Pn, In = [Pd[i] for i in idx], [Id[i] for i in idx]
        _check(ctx.verify_batch(Pn, In, draws), br.expected([(s, p, i) for p, i in zip(Pn, In)], draws), True, ident)


def test_two_keys_interleaved(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    t = circuits.setup_vector_mul(8, 4)
    try:
        Q, J = circuits.prove_vector_mul_batch(t, 32, seed=44, threads=16)
        ctx_t = _ctx(t)
        n = 64
        # (a) adjacent duplicated pairs, the keys alternating pair by pair, draws r - 1: everything cancels
        items = [(s, P[j // 2], I[j // 2]) if (j // 2) % 2 == 0 else (t, Q[j // 2 % 32], J[j // 2 % 32]) for j in range(n)]
        # (b) keys interleaved proof by proof, one duplicated pair within key 0, programmed draws
        items_b = [(s, P[j], I[j]) if j % 2 == 0 else (t, Q[j // 2], J[j // 2]) for j in range(n)]
        items_b[11] = items_b[10]
        for its, draws, ident in ((items, br.pattern_draws("alternating", n), True), (items_b, br.pattern_draws("programmed", n, 4), False)):
            keys = [0 if it[0] is s else 1 for it in its]
            got = h2v.verify_batch_keys([ctx, ctx_t], keys, [p for _, p, _ in its], [i for _, _, i in its], draws)
            _check(got, br.expected(its, draws), True, ident)
        ctx_t.close()
    finally:
        t.free()


def test_seeded(pool):
    s, P, I, ctx = pool
    n = 64
    idx = list(range(100, 100 + n))
    items = [(s, P[i], I[i]) for i in idx]
    Pn, In = [P[i] for i in idx], [I[i] for i in idx]
    m = br.programmed_multipliers(n)
    draws = br.draws_for(m, first=pow(m[0], -1, R_MOD))        # the product of all draws is 1
    _, _, left, right = br.expected(items, draws)
    neg = lambda pt: oracle_lib.g1_msm(s.L, [R_MOD - 1], [pt])
    seed = (neg(left), neg(right))
    got = ctx.verify_batch(Pn, In, draws, seed=(([1], [seed[0]]), ([1], [seed[1]])))
    _check(got, br.expected(items, draws, seed=seed), True, True)
    # a zero first draw zeroes the seed: the batch's own accumulators
    z = [0] + draws[1:]
    got = ctx.verify_batch(Pn, In, z, seed=(([1], [seed[0]]), ([1], [seed[1]])))
    _check(got, br.expected(items, z, seed=seed), True)
    assert got[2:] == (left, right)


@pytest.mark.parametrize("R", [2, 8])
def test_sharded_with_a_cancelling_shard(pool, R):
    """distributed.verify_batch_sharded_local: shard 1 holds adjacent duplicated pairs whose second draw is r - 1, so its record is the
    identity; the other shards' draws are random."""
    from halo2_verifier_amd import distributed as h2d
    s, P, I, ctx = pool
    n = 512
    sh = n // R
    idx = [(9 + i) % POOL for i in range(n)]
    draws = br.pattern_draws("random", n, R)
    for i in range(sh, 2 * sh):
        idx[i] = 600 + (i - sh) // 2
        if (i - sh) % 2:
            draws[i] = R_MOD - 1
    items = [(s, P[i], I[i]) for i in idx]
    assert br.expected(items[sh:2 * sh], draws[sh:2 * sh])[2:] == (br.ZERO, br.ZERO)
    got = h2d.verify_batch_sharded_local(ctx, [P[i] for i in idx], [I[i] for i in idx], draws, R)
    _check(got, br.expected(items, draws), True)


def test_recheck_programmed_ranges(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    n, k = 256, 100
    idx = list(range(300, 300 + n))
    m = br.programmed_multipliers(n)
    draws = br.draws_for(m)
    items = [(s, P[i], I[i]) for i in idx]
    b = _batch(ctx, [P[i] for i in idx], [I[i] for i in idx], draws)
    _check(b.finish(), br.expected(items, draws), True)
    ranges = [(0, n), (0, 1), (17, 40), (n - 1, 1), (128, 128), (3, 9)]
    oks, lefts, rights = b.recheck(ranges)
    for (f, c), ok, l, r in zip(ranges, oks, lefts, rights):
        assert (ok, l, r) == br.expected_range(items, draws, f, c) and ok, (f, c)
    # a zero draw at k: the proofs before k have multiplier 0; a range over one of them is refused, a range from k on is checked
    z = list(draws); z[k] = 0
    b.close()
    b = _batch(ctx, [P[i] for i in idx], [I[i] for i in idx], z)
    _check(b.finish(), br.expected(items, z), True)
    with pytest.raises(h2v.H2VError):
        b.recheck([(k - 1, 2)])
    oks, lefts, rights = b.recheck([(k, 30), (k, n - k)])
    assert [(o, l, r) for o, l, r in zip(oks, lefts, rights)] == [br.expected_range(items, z, k, 30), br.expected_range(items, z, k, n - k)]
    b.close()
