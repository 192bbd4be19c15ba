"""The resident MSM object (h2v_msm_*, h2v_dual_msm_check_many, h2v_accumulator_add_msms) on the GPU, through the Python mirror (MSMKZG,
DualMSM, eval_many, dual_check_many, Accumulator.add_msms), against the CPU oracle's MSM and pairing, and cross-checked against the
one-shot entry points (h2v_msm_g1, h2v_pairing_check) over the same terms.  Read-backs are compared with Python integers.

Contexts: the MSM workspace of a context only grows, in every dimension (problems, terms per problem), so the cases with many problems
and the cases with large problems run on contexts of their own."""
import ctypes
import random

import pytest

import circuits
import oracle_lib
import srs_util
from srs_util import R_MOD, g1_xy

pytestmark = pytest.mark.gpu

FIRST_CAPACITY = 256   # csrc/msm_object.h H2V_MSM_FIRST_CAPACITY


def _ctx(srs):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(srs.params_raw, h2v.SerdeFormat.RawBytes))


@pytest.fixture(scope="module")
def ctx(srs):
    c = _ctx(srs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_big(srs):
    c = _ctx(srs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_many(srs):
    c = _ctx(srs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts(srs):
    return [g1_xy(p) for p in srs.g]


def _msm(ctx, scalars, bases):
    import halo2_verifier_amd as h2v
    m = h2v.MSMKZG(ctx)
    if scalars:
        m.append_terms(scalars, bases)
    return m


def _terms(rnd, pts, n):
    scalars = [rnd.randrange(R_MOD) for _ in range(n)]
    bases = [pts[rnd.randrange(len(pts))] for _ in range(n)]
    if n > 3:
        scalars[0], scalars[1], scalars[2] = 0, R_MOD - 1, 1
    if n > 5:
        bases[4] = bytes(64)   # the identity
        bases[5] = bases[3]    # a repeated base
    return scalars, bases


def _snapshot(m):
    return len(m), m.scalars(), m.bases()


# ---------------------------------------------------------------- eval

@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33, 1000])
def test_eval_matches_oracle(ctx, pts, oracle, n):
    scalars, bases = _terms(random.Random(3000 + n), pts, n)
    with _msm(ctx, scalars, bases) as m:
        assert len(m) == n
        exp = oracle_lib.g1_msm(oracle, scalars, bases)
        assert m.eval() == exp
        assert ctx.msm_g1(scalars, bases) == exp
        assert m.check() is (exp == bytes(64))
        assert m.scalars() == scalars and m.bases() == bases


def test_eval_at_the_lds_sort_limit(ctx_big, pts, oracle):
    """16 384 terms: the largest problem that is not cut"""
    scalars, bases = _terms(random.Random(3100), pts, 16384)
    with _msm(ctx_big, scalars, bases) as m:
        exp = oracle_lib.g1_msm(oracle, scalars, bases)
        assert m.eval() == exp and ctx_big.msm_g1(scalars, bases) == exp


@pytest.mark.parametrize("n", [16385, 49153])
def test_eval_cut_problems(ctx_big, pts, oracle, n):
    """16 385: the first size cut into sub-problems; 49 153 = 3 x 16 384 + 1: msm_merge_windows with a one-term tail.  The 256 SRS bases
    cycled: the exact point is the oracle's 256-term MSM of the per-base sums of the scalars mod r."""
    rnd = random.Random(3200 + n)
    scalars = [rnd.randrange(R_MOD) for _ in range(n)]
    scalars[5], scalars[n - 1], scalars[16383] = 0, R_MOD - 1, 1
    bases = [pts[i % len(pts)] for i in range(n)]
    sums = [sum(scalars[j::len(pts)]) % R_MOD for j in range(len(pts))]
    exp = oracle_lib.g1_msm(oracle, sums, pts)
    with _msm(ctx_big, scalars, bases) as m:
        assert m.eval() == exp
        assert ctx_big.msm_g1(scalars, bases) == exp
        assert len(m) == n and m.scalars(n - 2, 2) == scalars[n - 2:] and m.bases(16382, 3) == bases[16382:16385]


@pytest.mark.parametrize("kind", ["zero_scalars", "one_scalar", "p_and_minus_p", "s_and_r_minus_s"])
def test_eval_skewed_inputs(ctx, srs, pts, oracle, kind):
    rnd = random.Random(3300)
    n = 5000
    if kind == "zero_scalars":
        scalars, bases = [0] * n, [pts[rnd.randrange(len(pts))] for _ in range(n)]
    elif kind == "one_scalar":      # every term in the same bucket of every window
        k = rnd.randrange(R_MOD)
        scalars, bases = [k] * n, [pts[rnd.randrange(len(pts))] for _ in range(n)]
    elif kind == "p_and_minus_p":
        p = srs.g[7]
        scalars, bases = [5, 5], [g1_xy(p), g1_xy((p[0], srs_util.P - p[1]))]
    else:
        s = rnd.randrange(1, R_MOD)
        scalars, bases = [s, R_MOD - s], [pts[9], pts[9]]
    exp = oracle_lib.g1_msm(oracle, scalars, bases)
    with _msm(ctx, scalars, bases) as m:
        assert m.eval() == exp and ctx.msm_g1(scalars, bases) == exp
        if kind != "one_scalar":
            assert exp == bytes(64) and m.check() is True
        else:
            assert m.check() is False


# ---------------------------------------------------------------- eval_many

def test_eval_many_mixed_sizes(ctx_big, pts, oracle):
    """0, 1 and 20 000 terms in one call: the launch is cut by its largest problem, and the empty object is the zero term"""
    import halo2_verifier_amd as h2v
    rnd = random.Random(3400)
    n = 20000
    scalars = [rnd.randrange(R_MOD) for _ in range(n)]
    bases = [pts[i % len(pts)] for i in range(n)]
    big = oracle_lib.g1_msm(oracle, [sum(scalars[j::len(pts)]) % R_MOD for j in range(len(pts))], pts)
    one = (rnd.randrange(1, R_MOD), pts[3])
    ms = [_msm(ctx_big, [], []), _msm(ctx_big, [one[0]], [one[1]]), _msm(ctx_big, scalars, bases)]
    try:
        xy, ident = h2v.eval_many(ms)
        assert xy == [bytes(64), oracle_lib.g1_msm(oracle, [one[0]], [one[1]]), big]
        assert ident == [True, False, False]
        assert ctx_big.msm_g1([one[0]], [one[1]]) == xy[1]
    finally:
        for m in ms:
            m.close()


def test_eval_many_crosses_the_problem_limit(ctx_many, pts, oracle):
    """1025 objects of 1 - 3 terms: more than MSM_MAX_PROBLEMS, so two launches; and the same object twice in one call"""
    import halo2_verifier_amd as h2v
    rnd = random.Random(3500)
    ms, exp = [], []
    try:
        for i in range(1025):
            k = 1 + i % 3
            scalars = [rnd.randrange(R_MOD) for _ in range(k)]
            bases = [pts[rnd.randrange(len(pts))] for _ in range(k)]
            ms.append(_msm(ctx_many, scalars, bases))
            exp.append(oracle_lib.g1_msm(oracle, scalars, bases))
        xy, ident = h2v.eval_many(ms)
        assert xy == exp and ident == [False] * 1025
        xy, ident = h2v.eval_many([ms[7], ms[1024], ms[7]])
        assert xy == [exp[7], exp[1024], exp[7]]
    finally:
        for m in ms:
            m.close()


# ---------------------------------------------------------------- scale

def test_scale(ctx, pts, oracle):
    rnd = random.Random(3600)
    scalars, bases = _terms(rnd, pts, 700)
    f = rnd.randrange(2, R_MOD)
    with _msm(ctx, scalars, bases) as m:
        before = m.eval()
        m.scale(f)
        assert m.scalars() == [s * f % R_MOD for s in scalars] and m.bases() == bases
        assert m.eval() == oracle_lib.g1_msm(oracle, [f], [before])
        m.scale(f.to_bytes(32, "little"))
        assert m.scalars() == [s * f * f % R_MOD for s in scalars]
        m.scale(0)
        assert len(m) == 700 and m.scalars() == [0] * 700 and m.check() is True and m.eval() == bytes(64)
    with _msm(ctx, [], []) as e:
        e.scale(f)   # an empty object: a no-op
        assert len(e) == 0 and e.check() is True


# ---------------------------------------------------------------- append / add_msm / clone

def test_order_growth_and_clone(ctx, pts, oracle):
    import halo2_verifier_amd as h2v
    rnd = random.Random(3700)
    chunks = [_terms(rnd, pts, k) for k in (200, 1, 150, 300, 700)]   # 200, 201, 351 (> 256: grows), 651 (> 512: grows), 1351 (> 1024: grows)
    all_s, all_b = [], []
    with h2v.MSMKZG(ctx) as m, h2v.MSMKZG(ctx) as a, h2v.MSMKZG(ctx) as b:
        for s, bs in chunks[:3]:
            before = (list(all_s), list(all_b))
            m.append_terms(s, bs) if len(s) > 1 else m.append_term(s[0], bs[0])
            all_s += s; all_b += bs
            assert m.scalars(0, len(before[0])) == before[0] and m.bases(0, len(before[1])) == before[1]   # growth keeps the contents
            assert len(m) == len(all_s)
        assert 200 < FIRST_CAPACITY < len(m)
        a.append_terms(*chunks[3]); b.append_terms(*chunks[4])
        for src, (s, bs) in ((a, chunks[3]), (b, chunks[4])):
            before = _snapshot(m)
            m.add_msm(src)
            all_s += s; all_b += bs
            assert (len(m), m.scalars(), m.bases()) == (len(all_s), all_s, all_b)
            assert m.scalars(0, before[0]) == before[1]
            assert _snapshot(src) == (len(s), s, bs)   # the source is not changed
        assert m.eval() == oracle_lib.g1_msm(oracle, all_s, all_b) == ctx.msm_g1(all_s, all_b)
        m.add_msm(h2v.MSMKZG(ctx))   # an empty source: a no-op
        assert len(m) == len(all_s)
        # a clone is independent of its source, both ways
        c = m.clone()
        try:
            assert _snapshot(c) == (len(all_s), all_s, all_b)
            c.scale(2)
            c.append_term(1, pts[0])
            assert _snapshot(m) == (len(all_s), all_s, all_b)
            m.scale(3)
            assert c.scalars() == [s * 2 % R_MOD for s in all_s] + [1]
        finally:
            c.close()


# ---------------------------------------------------------------- AccumulatorStrategy::process by hand

@pytest.fixture(scope="module")
def pool():
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 5, seed=71, threads=4)
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    guards = []
    for p, inst in zip(P, I):
        rc, g = ctx.guard_msm(p, inst)
        assert rc == 0
        guards.append(g)
    rnd = random.Random(72)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    yield s, ctx, guards, rand
    ctx.close()
    s.free()


def _ints(raw):
    return [int.from_bytes(b, "little") for b in raw]


def test_accumulator_strategy_by_hand(pool):
    import halo2_verifier_amd as h2v
    s, ctx, guards, rand = pool
    with h2v.DualMSM(ctx) as D:
        for r, g in zip(rand, guards):
            D.scale(r)
            D.add_msm(g)
        exp_l, exp_r = [], []
        for i, g in enumerate(guards):
            w = 1
            for r in rand[i + 1:]:
                w = w * r % R_MOD
            exp_l += [v * w % R_MOD for v in _ints(g["left_scalars"])]
            exp_r += [v * w % R_MOD for v in _ints(g["right_scalars"])]
        assert D.left.scalars() == exp_l and D.right.scalars() == exp_r
        assert D.left.bases() == [b for g in guards for b in g["left_bases"]]
        acc = h2v.Accumulator(ctx)
        acc.process_guards(guards, rand)
        exp = acc.finalize()
        acc.close()
        ok, lefts, rights = h2v.dual_check_many([D])
        assert (ok[0], lefts[0], rights[0]) == exp and exp[0] is True
        assert D.check() is True
        assert ctx.pairing_check(lefts[0], rights[0]) is True and circuits.oracle_pairing_check(s, lefts[0], rights[0]) is True


def test_dual_check_many_names_the_tampered_guard(pool):
    import halo2_verifier_amd as h2v
    s, ctx, guards, rand = pool
    duals = []
    try:
        for i, g in enumerate(guards):
            g = dict(g)
            if i == 3:
                rs = list(g["right_scalars"])
                rs[2] = ((int.from_bytes(rs[2], "little") + 1) % R_MOD).to_bytes(32, "little")
                g["right_scalars"] = rs
            d = h2v.DualMSM(ctx)
            d.add_msm(g)
            duals.append(d)
        ok, lefts, rights = h2v.dual_check_many(duals)
        assert ok == [True, True, True, False, True]
        for i in range(5):
            assert ctx.pairing_check(lefts[i], rights[i]) is ok[i] and circuits.oracle_pairing_check(s, lefts[i], rights[i]) is ok[i]
        assert ctx.guards_check_each(guards) == [True] * 5
        # two empty channels pass; the same object on both sides is allowed
        e = h2v.DualMSM(ctx)
        duals.append(e)
        assert h2v.dual_check_many([e]) == ([True], [bytes(64)], [bytes(64)])
        same = h2v.DualMSM(ctx, duals[0].left, duals[0].left)
        ok2, l2, r2 = h2v.dual_check_many([same])
        assert l2 == r2 == [lefts[0]] and ok2 == [ctx.pairing_check(lefts[0], lefts[0])]
    finally:
        for d in duals:
            d.close()


@pytest.mark.parametrize("journal", [0, 4])
def test_accumulator_add_msms_equals_add_msm(pool, journal):
    import halo2_verifier_amd as h2v
    s, ctx, guards, rand = pool
    g = guards[1]
    left, right = (g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"])
    a, b = h2v.Accumulator(ctx, journal=journal), h2v.Accumulator(ctx, journal=journal)
    with h2v.DualMSM(ctx) as D:
        D.add_msm(g)
        for acc in (a, b):
            acc.process_guards(guards[:1], rand[:1])
        a.add_msm(left, right)
        b.add_msms(D)
        a.add_msm(left, ([], []))
        b.add_msms((D.left, None))
        assert a.read() == b.read() and a.check_legs() == b.check_legs() and a.finalize() == b.finalize()
        assert len(a.check_legs()) == (4 if journal else 0)
        if journal:   # a full journal refuses before any device work, and nothing changes
            before, snap = b.read(), (_snapshot(D.left), _snapshot(D.right))
            with pytest.raises(h2v.H2VError) as e:
                b.add_msms(D)
            assert e.value.code == -19 and b.read() == before and len(b.check_legs()) == 4
            assert (_snapshot(D.left), _snapshot(D.right)) == snap
    a.close(); b.close()


# ---------------------------------------------------------------- refusals: each leaves length and read-back as they were

def test_refusals_change_nothing(ctx, srs, pts):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import _lib
    rnd = random.Random(3800)
    scalars, bases = _terms(rnd, pts, 10)
    with _msm(ctx, scalars, bases) as m:
        snap = _snapshot(m)
        more_s, more_b = _terms(rnd, pts, 300)
        off_curve = g1_xy((1, 3))
        x_too_large = (srs_util.P + 1).to_bytes(32, "little") + (2).to_bytes(32, "little")
        for bad_scalar, bad_base in ((R_MOD, None), (None, off_curve), (None, x_too_large)):
            s2, b2 = list(more_s), list(more_b)
            if bad_scalar is not None:
                s2[155] = bad_scalar
            if bad_base is not None:
                b2[155] = bad_base
            b2[200] = off_curve   # a later bad term: the lowest one is named
            with pytest.raises(h2v.H2VError) as e:
                m.append_terms(s2, b2)
            assert e.value.code == -16 and "term 155:" in str(e.value), str(e.value)
            assert _snapshot(m) == snap
        with pytest.raises(h2v.H2VError) as e:
            m.scale(R_MOD)
        assert e.value.code == -16 and _snapshot(m) == snap
        with pytest.raises(h2v.H2VError) as e:
            m.add_msm(m)
        assert e.value.code == -16 and _snapshot(m) == snap
        lib = _lib.load_library()
        buf = ctypes.create_string_buffer(32 * 16)
        for first, count in ((0, 11), (10, 1), (11, 0), (2 ** 63, 2 ** 63)):
            assert lib.h2v_msm_terms(m._h, first, count, buf, None) == -16
        assert lib.h2v_msm_terms(m._h, 10, 0, buf, None) == 0
        assert _snapshot(m) == snap
        # objects of two contexts over different params
        s2 = circuits.setup_vector_mul(8, 8, s_seed=99)
        other = h2v.Context(h2v.ParamsKZG(s2.params, h2v.SerdeFormat.RawBytes))
        try:
            with _msm(other, scalars, bases) as o:
                for call in (lambda: m.add_msm(o), lambda: h2v.eval_many([m, o]), lambda: h2v.dual_check_many([h2v.DualMSM(ctx, m, o)])):
                    with pytest.raises(h2v.H2VError) as e:
                        call()
                    assert e.value.code == -16 and "params" in str(e.value)
                acc = h2v.Accumulator(ctx)
                with pytest.raises(h2v.H2VError) as e:
                    acc.add_msms((o, None))
                assert e.value.code == -16 and acc.read()[:2] == (bytes(64), bytes(64))
                acc.close()
                assert _snapshot(o) == (10, scalars, bases)
        finally:
            other.close()
            s2.free()
        assert _snapshot(m) == snap
        # null arguments through the raw signatures
        h = ctypes.c_void_p()
        n = ctypes.c_size_t(0)
        ok = (ctypes.c_int * 1)()
        arr = (ctypes.c_void_p * 1)(m._h)
        null_arr = (ctypes.c_void_p * 1)(None)
        for rc in (lib.h2v_msm_create(None, ctypes.byref(h)), lib.h2v_msm_create(ctx._h, None), lib.h2v_msm_append_terms(None, b"", b"", 0),
                   lib.h2v_msm_append_terms(m._h, None, bases[0], 1), lib.h2v_msm_append_terms(m._h, bytes(32), None, 1), lib.h2v_msm_add_msm(m._h, None),
                   lib.h2v_msm_add_msm(None, m._h), lib.h2v_msm_scale(m._h, None), lib.h2v_msm_scale(None, bytes(32)), lib.h2v_msm_len(m._h, None),
                   lib.h2v_msm_len(None, ctypes.byref(n)), lib.h2v_msm_terms(None, 0, 0, None, None), lib.h2v_msm_eval_many(None, 1, None, None),
                   lib.h2v_msm_eval_many(null_arr, 1, None, None), lib.h2v_dual_msm_check_many(arr, arr, 1, None, None, None),
                   lib.h2v_dual_msm_check_many(arr, null_arr, 1, ok, None, None), lib.h2v_dual_msm_check_many(None, arr, 1, ok, None, None),
                   lib.h2v_accumulator_add_msms(None, m._h, m._h)):
            assert rc == -16
        lib.h2v_msm_destroy(None)   # allowed
        assert lib.h2v_msm_eval_many(None, 0, None, None) == 0 and lib.h2v_dual_msm_check_many(None, None, 0, None, None, None) == 0
        assert _snapshot(m) == snap
        # and the object still works
        m.append_terms(more_s, more_b)
        assert _snapshot(m) == (310, scalars + more_s, bases + more_b)
