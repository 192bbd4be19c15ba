"""The resident accumulator (h2v_accumulator_*): an AccumulatorStrategy that lives on the GPU across calls.

The reference's strategy is incremental — verify_proof takes a key and instances on every call, finalize() runs the one pairing
whenever the caller decides, with() resumes an accumulation (kzg/strategy.rs:69-140).  A process call of n proofs with draws
r_0 .. r_{n-1} is n x (scale the accumulator by the draw, add the Guard):

    (L, R) <- M (L, R) + sum_i (prod_{j > i} r_j) Guard_i,     M = r_0 .. r_{n-1}

so process(A); process(B); finalize() must equal ONE accumulation over A + B with the draws concatenated — verdict, statuses and both
accumulator points, bit for bit — for any cut.  Expected values come from the CPU oracle (circuits.oracle_verify_batch,
circuits.oracle_accumulate, batch_reference.expected) and from the library's own one-call entry points."""
import ctypes
import random

import pytest

import batch_reference
import circuits
import oracle_lib
from circuits import R_MOD

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
ZERO = bytes(64)


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _legs(ctx, P, I, rand, cuts, acc=None):
    """process the proofs of one key in legs cut at `cuts` (a cut may repeat: an empty leg), then finalize
    -> (ok, statuses, left, right) as Context.verify_batch returns them"""
    import halo2_verifier_amd as h2v
    own = acc is None
    if own:
        acc = h2v.Accumulator(ctx)
    st, all_ok = [], True
    bounds = [0] + list(cuts) + [len(P)]
    for a, b in zip(bounds, bounds[1:]):
        st += acc.process(ctx, None, P[a:b], I[a:b], rand[a:b])
        all_ok = all_ok and acc.last_all_ok
    ok, left, right = acc.finalize()
    assert all_ok == (not any(st))
    if own:
        acc.close()
    return ok, st, left, right


def _key_legs(ctxs, setups, items, rand, bounds):
    """process items = [(setup, proof, instances)] over several keys in legs [bounds[j], bounds[j + 1]), every leg given every context"""
    import halo2_verifier_amd as h2v
    acc = h2v.Accumulator(ctxs[0])
    keys = [next(k for k, s in enumerate(setups) if s is it[0]) for it in items]
    st = []
    for a, b in zip(bounds, bounds[1:]):
        st += acc.process(ctxs, keys[a:b], [p for _, p, _ in items[a:b]], [i for _, _, i in items[a:b]], rand[a:b])
    ok, left, right = acc.finalize()
    counters = acc.read()[2:]
    acc.close()
    return (ok, st, left, right), counters


def _mixed_lens(s, lens, seed):
    rnd = random.Random(seed)
    P, I = [], []
    for j, m in enumerate(lens):
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=seed * 100 + j)
        P.append(p); I.append(inst)
    return P, I


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 24, seed=555, threads=8)
    ctx = _ctx(s)
    yield s, P, I, ctx
    ctx.close()
    s.free()


@pytest.fixture(scope="module")
def two_keys():
    """vector-mul with n_mul 8 and 4 over one params, 32 proofs each, and a context per key"""
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params and s8.vk != s4.vk
    P8, I8 = circuits.prove_vector_mul_batch(s8, 32, seed=31, threads=8)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 32, seed=32, threads=8)
    c8, c4 = _ctx(s8), _ctx(s4)
    yield s8, s4, list(zip(P8, I8)), list(zip(P4, I4)), c8, c4
    c8.close(); c4.close()
    s8.free(); s4.free()


def test_legs_equal_one_accumulation(pool):
    s, P, I, ctx = pool
    rand = _draws(24, 1)
    whole = ctx.verify_batch(P, I, rand)
    assert whole[0] is True and circuits.oracle_verify_batch(s, P, I, rand) == whole
    for cuts in ((1,), (7,), (23,), (5, 11), (7, 7), ()):   # two legs at three cuts, three legs 5 / 6 / 13, an empty process in the middle, one leg
        assert _legs(ctx, P, I, rand, cuts) == whole, cuts


def test_several_keys_and_shapes_per_leg(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    Pm, Im = _mixed_lens(s8, [8, 5, 8, 3, 5, 0, 8, 3], 9)
    first = [(s8, p, i) for p, i in zip(Pm, Im)] + [(s8, p, i) for p, i in A[8:]]   # per-proof shapes inside the first key
    items = []
    for x, y in zip(first, [(s4, p, i) for p, i in B]):
        items += [x, y]
    assert len(items) == 64
    rand = _draws(64, 2)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    keys = [0 if it[0] is s8 else 1 for it in items]
    assert h2v.verify_batch_keys([c8, c4], keys, [p for _, p, _ in items], [i for _, _, i in items], rand) == exp
    bounds = [0, 10, 11, 64]
    got, counters = _key_legs([c8, c4], [s8, s4], items, rand, bounds)
    assert got == exp and counters == (64, 0)
    got, _ = _key_legs([c4, c8], [s4, s8], items, rand, bounds)     # the contexts listed the other way round
    assert got == exp


def test_scale_edge_cases_programmed_through_the_draws(pool):
    """The scale kernel multiplies the resident points by M, the product of a call's draws: a leg of ONE proof whose draw is v makes
    M = v.  1, r - 1 against the same proof (the scaled accumulator meets its negative: both points the identity), 0 (everything
    before drops out), then every GLV edge scalar and every programmed value, leg after leg on one accumulator."""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    L_ = oracle_lib.load()
    d3 = _draws(3, 3)
    for v in (1, 0):
        items = [(s, p, i) for p, i in zip(P[:4], I[:4])]
        exp = batch_reference.expected(items, d3 + [v])
        assert exp[0] is True
        assert _legs(ctx, P[:4], I[:4], d3 + [v], (3,)) == exp, v
    # r - 1: leg 2 repeats leg 1's single proof
    acc = h2v.Accumulator(ctx)
    d = _draws(1, 4)
    st = acc.process(ctx, None, P[:1], I[:1], d) + acc.process(ctx, None, P[:1], I[:1], [R_MOD - 1])
    exp = batch_reference.expected([(s, P[0], I[0])] * 2, d + [R_MOD - 1])
    assert exp == (True, [0, 0], ZERO, ZERO)
    assert st == [0, 0] and acc.read() == (ZERO, ZERO, 2, 0) and acc.finalize() == (True, ZERO, ZERO)
    acc.close()
    # the value lists, none left out: (L, R) <- v (L, R) + Guard_p, tracked as coefficients of the distinct proofs' own Guards
    values = batch_reference.glv_edge_scalars() + batch_reference.programmed_values()
    assert len(values) > 100 and all(0 < v < R_MOD for v in values)
    singles = [batch_reference.single(s, P[j], I[j]) for j in range(4)]
    assert all(rc == 0 for rc, _, _ in singles)
    coef = [0, 0, 0, 0]
    acc = h2v.Accumulator(ctx)
    lead = _draws(3, 5)
    assert acc.process(ctx, None, P[:3], I[:3], lead) == [0, 0, 0]
    for j, m in enumerate(batch_reference.multipliers(lead)):
        coef[j] = m
    for t, v in enumerate(values):
        j = t % 4
        assert acc.process(ctx, None, [P[j]], [I[j]], [v]) == [0]
        coef = [c * v % R_MOD for c in coef]
        coef[j] = (coef[j] + 1) % R_MOD
        left, right, n, failed = acc.read()
        terms = [(c, k) for k, c in enumerate(coef) if c]
        exp_left = oracle_lib.g1_msm(L_, [c for c, _ in terms], [singles[k][1] for _, k in terms])
        exp_right = oracle_lib.g1_msm(L_, [c for c, _ in terms], [singles[k][2] for _, k in terms])
        assert (left, right, n, failed) == (exp_left, exp_right, 4 + t, 0), (t, hex(v))
    ok, left, right = acc.finalize()
    assert ok is True and circuits.oracle_pairing_check(s, left, right)
    acc.close()


def _raw_process(acc, ctxs, keys, proofs, instances, ncols, col_lens, rand=None):
    """h2v_accumulator_process with every argument as given (no checks on the Python side) -> rc"""
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    n = len(proofs)
    PA = ctypes.c_char_p * max(n, 1)
    ca = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    ka = (ctypes.c_uint32 * max(n, 1))(*keys)
    pl = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    ia = PA(*[b"".join(v for col in inst for v in col) for inst in instances])
    nca = (ctypes.c_size_t * len(ncols))(*ncols)
    cl = (ctypes.c_size_t * max(len(col_lens), 1))(*col_lens)
    rb = b"".join(r.to_bytes(32, "little") for r in rand) if rand is not None else None
    st = (ctypes.c_int * max(n, 1))()
    ok = ctypes.c_int(0)
    return lib.h2v_accumulator_process(acc._h, ca, len(ctxs), ka, n, PA(*proofs), pl, ia, nca, cl, rb, st, ctypes.byref(ok))


def test_failure_and_atomicity(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    P, I = [p for p, _ in A[:10]], [i for _, i in A[:10]]
    rand = _draws(10, 6)
    bad = list(P)
    bad[7] = bad[7][:-96] + b"\xff" * 32 + bad[7][-64:]      # a non-canonical scalar: the last evaluation, in leg 2
    exp = circuits.oracle_verify_batch(s8, bad, I, rand)
    assert exp[0] is False and exp[1][7] == -5 and sum(1 for v in exp[1] if v) == 1
    acc = h2v.Accumulator(c8)
    st = acc.process(c8, None, bad[:5], I[:5], rand[:5])
    assert acc.last_all_ok is True
    st += acc.process(c8, None, bad[5:], I[5:], rand[5:])
    assert acc.last_all_ok is False and st == exp[1]
    ok, left, right = acc.finalize()
    assert (ok, left, right) == (exp[0], exp[2], exp[3])
    assert acc.read() == (exp[2], exp[3], 10, 1)
    # refused calls return their error and leave the points and the counters as they were
    before = acc.read()
    Pk = [p for p, _ in A[:4]] + [p for p, _ in B[:4]]
    Ik = [i for _, i in A[:4]] + [i for _, i in B[:4]]
    keys, col_lens = [0] * 4 + [1] * 4, [8] * 4 + [4] * 4
    assert _raw_process(acc, [c8, c4], keys[:-1] + [2], Pk, Ik, [1, 1], col_lens, _draws(8, 7)) == BAD_ARGUMENT     # a key index out of range
    assert acc.read() == before
    other = circuits.setup_vector_mul(8, 4, s_seed=43)                                                              # params over another s
    co = _ctx(other)
    assert _raw_process(acc, [c8, co], keys, Pk, Ik, [1, 1], col_lens, _draws(8, 7)) == BAD_ARGUMENT
    assert acc.read() == before
    assert _raw_process(acc, [co], [0] * 4, Pk[4:], Ik[4:], [1], col_lens[4:], _draws(4, 7)) == BAD_ARGUMENT        # ... also as the only context
    assert acc.read() == before
    keys65, lens65 = [0] * 64 + [1], list(range(64)) + [4]                                                          # 65 (key, shape) groups
    I65 = [[[circuits.le32(1)] * m] for m in lens65]
    assert _raw_process(acc, [c8, c4], keys65, [Pk[0]] * 65, I65, [1, 1], lens65) == UNSUPPORTED
    assert acc.read() == before
    with pytest.raises(h2v.H2VError) as e:                                                                          # a draw that is not canonical
        acc.process(c8, None, P[:2], I[:2], [1, R_MOD])
    assert e.value.code == BAD_ARGUMENT and acc.read() == before
    # and the accumulator still works: the same accumulation, continued, against the one-call reference
    more = _draws(3, 8)
    st = acc.process([c8, c4], [0, 1, 0], [P[0], B[0][0], P[1]], [I[0], B[0][1], I[1]], more)
    items = [(s8, p, i) for p, i in zip(bad, I)] + [(s8, P[0], I[0]), (s4, *B[0]), (s8, P[1], I[1])]
    exp = circuits.oracle_accumulate(items, rand + more)
    ok, left, right = acc.finalize()
    assert (ok, exp[1][:10] + st, left, right) == exp and acc.read()[2:] == (13, 1)
    acc.close()
    co.close(); other.free()


def test_seeds(pool, two_keys, srs):
    import halo2_verifier_amd as h2v
    import srs_util
    s, P, I, ctx = pool
    L_ = oracle_lib.load()
    n = 9
    rand = _draws(n, 9)
    other = ctx.verify_batch(P[n:n + 6], I[n:n + 6], _draws(6, 10))
    assert other[0] is True
    seed_l, seed_r = other[2], other[3]
    # A: another accepted batch's (L, R) on an empty accumulator, then process
    acc = h2v.Accumulator(ctx)
    acc.add_msm(([1], [seed_l]), ([1], [seed_r]))
    assert acc.read() == (seed_l, seed_r, 0, 0)
    st = acc.process(ctx, None, P[:n], I[:n], rand)
    ok, left, right = acc.finalize()
    want = ctx.verify_batch(P[:n], I[:n], rand, seed=(([1], [seed_l]), ([1], [seed_r])))
    assert want[0] is True and (ok, st, left, right) == want
    acc.close()
    # B: the seed as split term lists, with a zero scalar and an identity base
    rnd = random.Random(11)
    pts = [srs_util.g1_xy(p) for p in srs.g[:6]]
    a, b = rnd.randrange(1, R_MOD), rnd.randrange(1, R_MOD)
    left_terms = ([a, (1 - a) % R_MOD, 0, 5], [seed_l, seed_l, pts[1], bytes(64)])
    right_terms = ([b, (1 - b) % R_MOD], [seed_r, seed_r])
    acc = h2v.Accumulator(ctx)
    acc.add_msm(left_terms, right_terms)
    st = acc.process(ctx, None, P[:n], I[:n], rand)
    assert (*acc.finalize()[:1], st, *acc.finalize()[1:]) == ctx.verify_batch(P[:n], I[:n], rand, seed=(left_terms, right_terms)) == want
    # E: malformed seeds are refused and change nothing
    before = acc.read()
    for seed in ((([1], [b"\x01" * 64]), ([], [])), (([R_MOD], [pts[0]]), ([], [])), (([1], [seed_l]), ([1], [b"\x02" * 64]))):
        with pytest.raises(h2v.H2VError) as e:
            acc.add_msm(*seed)
        assert e.value.code == BAD_ARGUMENT and acc.read() == before
    acc.close()
    # C: read() from one accumulator, add_msm into a fresh one, continue: the uninterrupted run
    whole = ctx.verify_batch(P[:n], I[:n], rand)
    first = h2v.Accumulator(ctx)
    st = first.process(ctx, None, P[:4], I[:4], rand[:4])
    l1, r1, _, _ = first.read()
    first.close()
    second = h2v.Accumulator(ctx)
    second.add_msm(([1], [l1]), ([1], [r1]))
    st += second.process(ctx, None, P[4:n], I[4:n], rand[4:])
    ok, left, right = second.finalize()
    assert (ok, st, left, right) == whole
    second.close()
    # D: a seeded accumulation over TWO keys (the queued mirrors refuse it): oracle_accumulate plus M x seed
    s8, s4, A, B, c8, c4 = two_keys
    assert s8.params == s.params
    items = []
    for x, y in zip([(s8, p, i) for p, i in A[:6]], [(s4, p, i) for p, i in B[:6]]):
        items += [x, y]
    rand2 = _draws(12, 12)
    exp = circuits.oracle_accumulate(items, rand2)
    M = 1
    for r in rand2:
        M = M * r % R_MOD
    exp_left = oracle_lib.g1_msm(L_, [M, 1], [seed_l, exp[2]])
    exp_right = oracle_lib.g1_msm(L_, [M, 1], [seed_r, exp[3]])
    acc = h2v.Accumulator(c8)
    acc.add_msm(([1], [seed_l]), ([1], [seed_r]))
    st = acc.process([c8, c4], [0, 1] * 6, [p for _, p, _ in items], [i for _, _, i in items], rand2[:12])
    assert st == exp[1] == [0] * 12
    assert acc.finalize() == (True, exp_left, exp_right) and circuits.oracle_pairing_check(s8, exp_left, exp_right)
    acc.close()


def test_lifecycle(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    rand = _draws(24, 13)
    whole = ctx.verify_batch(P, I, rand)
    assert whole[0] is True
    acc = h2v.Accumulator(ctx)
    assert acc.finalize() == (True, ZERO, ZERO) and acc.read() == (ZERO, ZERO, 0, 0)       # an empty DualMSM
    assert acc.process(ctx, None, [], [], []) == [] and acc.read() == (ZERO, ZERO, 0, 0)
    st = acc.process(ctx, None, P[:9], I[:9], rand[:9])
    part = acc.finalize()
    assert part == acc.finalize()                                                        # not consumed: the same answer again
    assert (part[0], st, *part[1:]) == ctx.verify_batch(P[:9], I[:9], rand[:9])
    st += acc.process(ctx, None, P[9:], I[9:], rand[9:])                                 # processing after finalize continues
    assert (acc.finalize()[0], st, *acc.finalize()[1:]) == whole
    acc.close()
    acc.close()
    # two accumulators used alternately on one context, the context's own one-shot call (same scratch batch) between their legs
    rand_b = _draws(24, 14)
    whole_b = ctx.verify_batch(P[::-1], I[::-1], rand_b)
    a, b = h2v.Accumulator(ctx), h2v.Accumulator(ctx)
    Pb, Ib = P[::-1], I[::-1]
    st_a, st_b = [], []
    for lo, hi in ((0, 6), (6, 7), (7, 24)):
        st_a += a.process(ctx, None, P[lo:hi], I[lo:hi], rand[lo:hi])
        assert ctx.verify_batch(P[:3], I[:3], rand[:3])[0] is True
        st_b += b.process(ctx, None, Pb[lo:hi], Ib[lo:hi], rand_b[lo:hi])
    fa, fb = a.finalize(), b.finalize()
    assert (fa[0], st_a, *fa[1:]) == whole and (fb[0], st_b, *fb[1:]) == whole_b
    a.close(); b.close()
    h2v.Accumulator(ctx).close()                                                         # never processed
    # a context without a VerifyingKey carries an accumulator
    bare = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes))
    acc = h2v.Accumulator(bare)
    st = acc.process(ctx, None, P, I, rand)
    assert (acc.finalize()[0], st, *acc.finalize()[1:]) == whole
    bare.close()                                                                         # (closes the accumulator first)


@pytest.mark.parametrize("mo,tr,m", [(circuits.GWC, circuits.KECCAK256, 1), (circuits.SHPLONK, circuits.BLAKE2B, 2)])
def test_other_instantiations(mo, tr, m):
    s = circuits.setup_vector_mul(8, 6).set_options(mo, tr).set_circuit_instances(m)
    if m == 1:
        P, I = circuits.prove_vector_mul_batch(s, 9, seed=77, threads=4)
    else:
        pairs = [circuits.prove_vector_mul_multi(s, m, seed=100 + i, rng_seed=7 + i) for i in range(9)]
        P, I = [p for p, _ in pairs], [i for _, i in pairs]
    ctx = _ctx(s)
    rand = _draws(9, 17)
    whole = ctx.verify_batch(P, I, rand)
    assert whole[0] is True and whole == circuits.oracle_verify_batch(s, P, I, rand)
    assert _legs(ctx, P, I, rand, (4,)) == whole
    ctx.close()
    s.free()
