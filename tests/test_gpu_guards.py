"""Guards at the trait seam: h2v_accumulator_process_guards and h2v_guards_check_each.

A CPU verify_proof (circuits.oracle_guard) makes each proof's Guard, the pair of term lists it would hand its strategy; the resident
accumulator takes n of them with n draws,

    (L, R) <- M (L, R) + sum_i (prod_{j > i} r_j) (sum_t ls_it lb_it, sum_t rs_it rb_it),     M = r_0 .. r_{n-1}

which is h2v_accumulator_process with the Guard supplied instead of computed.  Expected values come from the oracle
(oracle_verify_batch, oracle_accumulate, oracle_pairing_check, oracle_verify_single) and from big integers (msm_reference); the Guards
never come from the library under test."""
import ctypes
import os
import random

import pytest

import circuits
import msm_reference as ref
import oracle_lib
import srs_util
from circuits import R_MOD, le32

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
ZERO = bytes(64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(s, vk=True):
    import halo2_verifier_amd as h2v
    params = h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes)
    if not vk:
        return h2v.Context(params)
    return h2v.Context(params, h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes), multiopen=s.multiopen, transcript=s.transcript,
                       circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _guards(s, P, I):
    out = []
    for p, i in zip(P, I):
        rc, g = circuits.oracle_guard(s, p, i)
        assert rc == 0
        out.append(((g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"])))
    return out


def _tampered(guard):
    """the Guard with its first right scalar raised by 1"""
    (ls, lb), (rs, rb) = guard
    rs = [le32((int.from_bytes(rs[0], "little") + 1) % R_MOD)] + list(rs[1:])
    return (ls, lb), (rs, rb)


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 24, seed=555, threads=8)
    ctx, bare = _ctx(s), _ctx(s, vk=False)
    yield s, P, I, ctx, bare, _guards(s, P, I)
    ctx.close(); bare.close()
    s.free()


# ---- 1. equals process, equals the oracle
def test_guards_equal_process_and_the_oracle(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    rand = _draws(24, 1)
    whole = ctx.verify_batch(P, I, rand)
    assert whole[0] is True and circuits.oracle_verify_batch(s, P, I, rand) == whole
    for c in (ctx, bare):   # (the accumulator's context needs no VerifyingKey)
        acc = h2v.Accumulator(c)
        acc.process_guards(G, rand)
        assert acc.finalize() == (whole[0], whole[2], whole[3])
        assert acc.read()[2:] == (24, 0)
        acc.close()
    for cuts in ((1,), (7,), (23,), (5, 11), (7, 7)):
        for first_is_guards in (False, True):   # the legs alternate between proof bytes and Guards
            acc = h2v.Accumulator(bare)
            bounds = [0] + list(cuts) + [24]
            for leg, (a, b) in enumerate(zip(bounds, bounds[1:])):
                if (leg % 2 == 0) == first_is_guards:
                    acc.process_guards(G[a:b], rand[a:b])
                else:
                    assert not any(acc.process(ctx, None, P[a:b], I[a:b], rand[a:b]))
            assert acc.finalize() == (whole[0], whole[2], whole[3]), (cuts, first_is_guards)
            assert acc.read()[2:] == (24, 0)
            acc.close()


def test_guard_msm_dicts_and_os_draws(pool):
    """the dicts Context.guard_msm returns are accepted; rand=None draws on the library's side; n = 0 changes nothing"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    dicts = []
    for p, i in zip(P[:3], I[:3]):
        rc, g = ctx.guard_msm(p, i)
        assert rc == 0
        dicts.append(g)
    rand = _draws(3, 2)
    exp = ctx.verify_batch(P[:3], I[:3], rand)
    acc = h2v.Accumulator(bare)
    acc.process_guards([], [])
    assert acc.read() == (ZERO, ZERO, 0, 0)
    acc.process_guards(dicts, rand)
    assert acc.finalize() == (exp[0], exp[2], exp[3])
    acc.process_guards(G[3:9])   # OS draws: good Guards stay good
    assert acc.finalize()[0] is True and acc.read()[2:] == (9, 0)
    acc.close()


# ---- 2. other Guard shapes
@pytest.mark.parametrize("shape", ["gwc_keccak", "two_instances"])
def test_other_guard_shapes(shape):
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 4)
    if shape == "gwc_keccak":
        s.set_options(circuits.GWC, circuits.KECCAK256)
        P, I = [], []
        for j in range(5):
            p, inst = circuits.prove_vector_mul(s, [j + 1] * 4, [j + 2] * 4, rng_seed=70 + j)
            P.append(p); I.append(inst)
    else:
        s.set_circuit_instances(2)
        P, I = [], []
        for j in range(5):
            p, inst = circuits.prove_vector_mul_multi(s, 2, seed=80 + j, rng_seed=90 + j)
            P.append(p); I.append(inst)
    G = _guards(s, P, I)
    if shape == "gwc_keccak":
        assert len(G[0][0][0]) > 1   # GWC: several left terms, a base once per query
    rand = _draws(5, 3)
    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is True
    ctx = _ctx(s, vk=False)
    acc = h2v.Accumulator(ctx)
    acc.process_guards(G[:2], rand[:2])
    acc.process_guards(G[2:], rand[2:])
    assert acc.finalize() == (exp[0], exp[2], exp[3])
    assert ctx.guards_check_each(G) == [True] * 5
    acc.close(); ctx.close()
    s.free()


def test_two_keys_in_one_call():
    import halo2_verifier_amd as h2v
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 5, seed=31, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 5, seed=32, threads=4)
    items = []
    for a, b in zip(zip(P8, I8), zip(P4, I4)):
        items += [(s8,) + a, (s4,) + b]
    rand = _draws(10, 4)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    G = [_guards(s, [p], [i])[0] for s, p, i in items]
    ctx = _ctx(s8, vk=False)
    acc = h2v.Accumulator(ctx)
    acc.process_guards(G, rand)
    assert acc.finalize() == (exp[0], exp[2], exp[3])
    acc.close(); ctx.close()
    s8.free(); s4.free()


# ---- 3. programmed Guards, no prover
class _SrsSetup:
    """what circuits.oracle_pairing_check reads of a setup, over the golden SRS"""
    def __init__(self):
        self.L = oracle_lib.load()
        self.srs = srs_util.load_srs(os.path.join(ROOT, "tests", "golden", "kzg_bn254_8.srs"))
        self.params = self.srs.params_raw


@pytest.fixture(scope="module")
def programmed():
    import halo2_verifier_amd as h2v
    s = _SrsSetup()
    g0, g1 = s.srs.g[0], s.srs.g[1]
    # base k: (point, its coefficients over (g0, g1)); None: the identity under whatever scalar
    bases = [(g0, (1, 0)), (g1, (0, 1)), (ref.mul(2, g0), (2, 0)), (ref.mul(3, g1), (0, 3)), (ref.neg(g0), (R_MOD - 1, 0)), (ref.mul(5, g0), (5, 0)),
             (None, (0, 0))]
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes))
    yield s, g0, g1, bases, ctx
    ctx.close()


def _expected(g0, g1, bases, guards, rand, start=(None, None)):
    """(left, right) after process_guards over programmed guards — a guard is (left terms, right terms), a term (scalar, base index) —
    from `start`, by big integers: the coefficients of g0 and g1 on either side"""
    mult, run = [1] * len(guards), 1
    for i in range(len(guards) - 1, -1, -1):
        mult[i] = run
        run = run * rand[i] % R_MOD
    out = []
    for side in range(2):
        c0 = c1 = 0
        for guard, m in zip(guards, mult):
            for sc, b in guard[side]:
                c0 += sc * m * bases[b][1][0]; c1 += sc * m * bases[b][1][1]
        pt = ref.add(ref.mul(c0 % R_MOD, g0), ref.mul(c1 % R_MOD, g1))
        out.append(ref.add(ref.mul(run, start[side]), pt))
    return out


def _bytes_guard(bases, guard):
    return tuple(([le32(sc) for sc, _ in side], [ref.affine_bytes(bases[b][0]) for _, b in side]) for side in guard)


def _run_programmed(programmed, guards, rand, start=None):
    import halo2_verifier_amd as h2v
    s, g0, g1, bases, ctx = programmed
    acc = h2v.Accumulator(ctx)
    st = (None, None)
    if start:   # a non-empty accumulator in front: (7 g0, 9 g1)
        st = (ref.mul(7, g0), ref.mul(9, g1))
        acc.add_msm(([7], [ref.affine_bytes(g0)]), ([9], [ref.affine_bytes(g1)]))
    acc.process_guards([_bytes_guard(bases, g) for g in guards], rand)
    ok, left, right = acc.finalize()
    n = acc.read()[2]
    acc.close()
    exp = _expected(g0, g1, bases, guards, rand, st)
    assert (left, right) == (ref.affine_bytes(exp[0]), ref.affine_bytes(exp[1]))
    assert ok == circuits.oracle_pairing_check(s, left, right)
    assert n == len(guards)
    return ok, left, right


def test_programmed_edge_guards(programmed):
    IDENT = 6
    guards = [
        ([(5, 0)], []),                                   # an empty right side
        ([], []),                                         # both sides empty
        ([(11, IDENT)], [(13, IDENT), (3, 1)]),           # an all-zero base under a non-zero scalar
        ([(0, 0), (4, 1)], [(0, 2)]),                     # a zero scalar
        ([(6, 2), (7, 2)], [(8, 3), (9, 3), (1, 3)]),     # one base twice (and three times)
        ([(21, 0), (21, 4)], [(2, 5)]),                   # P and -P cancel
        ([(R_MOD - 1, 1)], [(R_MOD - 1, 0), (R_MOD - 1, 3)]),   # the scalar r - 1
    ]
    for start in (False, True):
        _run_programmed(programmed, guards, _draws(len(guards), 5), start)
        for r in (0, 1, R_MOD - 1):   # the draws 0, 1 and r - 1, in the middle and at both ends
            for at in (0, 3, len(guards) - 1):
                rand = _draws(len(guards), 6)
                rand[at] = r
                _run_programmed(programmed, guards, rand, start)
    # the left channel cancels to the identity as a whole
    ok, left, right = _run_programmed(programmed, [([(21, 0), (21, 4)], [])], [9])
    assert (left, right) == (ZERO, ZERO)
    # n = 1 with one term
    _run_programmed(programmed, [([(3, 1)], [])], [1])
    _run_programmed(programmed, [([], [(3, 1)])], [R_MOD - 1], True)


def test_programmed_257_guards(programmed):
    """257 Guards of 0 .. 5 terms a side: past MULT_TILE and the conversion kernel's workgroup of 256, with guard boundaries that line
    up with neither"""
    rnd = random.Random(7)
    guards = []
    for i in range(257):
        guards.append(tuple([(rnd.randrange(R_MOD), rnd.randrange(7)) for _ in range((i * 7 + 3 * side) % 6)] for side in range(2)))
    assert sum(len(g[0]) for g in guards) > 512 and len(guards[0][0]) == 0
    _run_programmed(programmed, guards, _draws(257, 8), True)


# ---- 4. the MSM's cut
def test_right_channel_past_the_msm_cut(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    per = len(G[0][1][0])   # right terms of one Guard
    n = 16384 // per + 1
    assert (n - 1) * per <= 16384 < n * per
    idx = [i % 24 for i in range(n)]
    rand = _draws(n, 9)
    exp = circuits.oracle_accumulate([(s, P[i], I[i]) for i in idx], rand)
    assert exp[0] is True
    acc = h2v.Accumulator(bare)
    acc.process_guards([G[i] for i in idx], rand)
    assert acc.finalize() == (exp[0], exp[2], exp[3])
    acc.close()


# ---- 5. refusals change nothing
def _replace(guard, side, term, scalar=None, base=None):
    sides = [[list(guard[0][0]), list(guard[0][1])], [list(guard[1][0]), list(guard[1][1])]]
    if scalar is not None:
        sides[side][0][term] = scalar
    if base is not None:
        sides[side][1][term] = base
    return (sides[0][0], sides[0][1]), (sides[1][0], sides[1][1])


BAD_TERMS = {
    "scalar_r": dict(scalar=le32(R_MOD)),
    "off_curve": dict(base=le32(1) + le32(3)),
    "x_geq_p": dict(base=le32(srs_util.P) + le32(2)),
}


@pytest.mark.parametrize("kind", sorted(BAD_TERMS))
def test_refusals_change_nothing(pool, kind):
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    acc = h2v.Accumulator(bare, journal=8)
    acc.process_guards(G[:4], _draws(4, 10))
    before = (acc.read(), acc.check_legs())
    verdicts = [7, 7, 7]
    call = G[4:7]
    for side, name in ((0, "left"), (1, "right")):
        for g, term in ((0, 0), (2, len(call[2][side][0]) - 1)):   # the first and the last term of the side
            bad = list(call)
            bad[g] = _replace(call[g], side, term, **BAD_TERMS[kind])
            with pytest.raises(h2v.H2VError) as e:
                acc.process_guards(bad, _draws(3, 11))
            assert e.value.code == BAD_ARGUMENT and f"guard {g}," in str(e.value) and f"{name} side" in str(e.value), str(e.value)
            assert (acc.read(), acc.check_legs()) == before
            # guards_check_each: the same refusal, and guard_ok untouched
            ok = (ctypes.c_int * 3)(*verdicts)
            assert bare._lib.h2v_guards_check_each(bare._h, *h2v.verifier._guards_args(bad), ok) == BAD_ARGUMENT
            assert list(ok) == verdicts and f"guard {g}," in h2v._lib.last_error() and f"{name} side" in h2v._lib.last_error()
    acc.process_guards(call, _draws(3, 11))   # the accumulator goes on
    assert acc.finalize()[0] is True and acc.read()[2:] == (7, 0) and len(acc.check_legs()) == 3
    acc.close()


def test_scalar_r_reaches_guards_check_each(pool):
    """(a scalar given as 32 bytes passes the Python mirror as it is: the library refuses it)"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    bad = [G[0], _replace(G[1], 1, 2, scalar=le32(R_MOD))]
    with pytest.raises(h2v.H2VError) as e:
        bare.guards_check_each(bad)
    assert e.value.code == BAD_ARGUMENT and "guard 1," in str(e.value) and "right side" in str(e.value)


def test_other_refusals(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    acc = h2v.Accumulator(bare, journal=3)
    acc.process_guards(G[:2], _draws(2, 12))
    before = (acc.read(), acc.check_legs())
    lib = bare._lib
    args = list(h2v.verifier._guards_args(G[2:4]))
    rand = b"".join(le32(r) for r in _draws(2, 13))
    for null_at in (1, 2, 3, 4, 5, 6):   # a null array that the counts say is read
        a = list(args)
        a[null_at] = None
        assert lib.h2v_accumulator_process_guards(acc._h, *a, rand) == BAD_ARGUMENT
        assert lib.h2v_guards_check_each(bare._h, *a, (ctypes.c_int * 2)()) == BAD_ARGUMENT
    assert lib.h2v_accumulator_process_guards(acc._h, *args, le32(5) + le32(R_MOD)) == BAD_ARGUMENT   # a draw equal to r
    assert lib.h2v_accumulator_process_guards(acc._h, (1 << 20) + 1, *args[1:], rand) == BAD_ARGUMENT
    assert (acc.read(), acc.check_legs()) == before
    acc.process_guards(G[2:4], _draws(2, 13))   # the journal is full now: the base and two entries
    before = (acc.read(), acc.check_legs())
    with pytest.raises(h2v.H2VError) as e:
        acc.process_guards(G[4:6], _draws(2, 14))
    assert e.value.code == UNSUPPORTED
    assert (acc.read(), acc.check_legs()) == before
    acc.process_guards([], [])   # no entry: not refused
    acc.close()


# ---- 6. journal
def test_journal_names_and_drops_a_guards_leg(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx, bare, G = pool
    rand = _draws(24, 15)
    acc = h2v.Accumulator(bare, journal=8, keep_inputs=True)
    assert not any(acc.process(ctx, None, P[:8], I[:8], rand[:8]))
    leg = list(G[8:16])
    leg[5] = _tampered(leg[5])
    acc.process_guards(leg, rand[8:16])
    acc.process_guards(G[16:], rand[16:])
    assert acc.finalize()[0] is False
    assert acc.check_legs() == [(0, 0, True), (8, 0, True), (8, 0, False), (8, 0, True)]
    assert bare.guards_check_each(leg) == [i != 5 for i in range(8)]
    assert acc.identify() == {2: [0 if i != 5 else -2 for i in range(8)]}
    acc.drop_legs([2])
    fresh = h2v.Accumulator(bare)
    fresh.process(ctx, None, P[:8], I[:8], rand[:8])
    fresh.process_guards(G[16:], rand[16:])
    assert acc.read() == fresh.read() and acc.finalize() == fresh.finalize() and acc.finalize()[0] is True
    assert acc.check_legs() == [(0, 0, True), (8, 0, True), (8, 0, True)]
    acc.close(); fresh.close()


# ---- 7. guards_check_each
def test_check_each_equals_the_oracle_proof_by_proof(pool):
    s, P, I, ctx, bare, G = pool
    It = list(I)
    for i in (2, 11, 23):   # a wrong public input: verify_proof still returns its Guard, whose own check fails
        col = list(I[i][0])
        col[0] = le32((int.from_bytes(col[0], "little") + 1) % R_MOD)
        It[i] = [col]
    Gt = _guards(s, P, It)
    exp = [circuits.oracle_verify_single(s, p, i) == 0 for p, i in zip(P, It)]
    assert exp == [i not in (2, 11, 23) for i in range(24)]
    assert bare.guards_check_each(Gt) == exp
    assert ctx.guards_check_each(Gt[:1]) == exp[:1] and bare.guards_check_each([]) == []


def test_check_each_across_the_512_guard_launch(pool, programmed):
    s, P, I, ctx, bare, G = pool
    guards = [G[i % 24] for i in range(513)]
    for i in (0, 511, 512):
        guards[i] = _tampered(guards[i])
    assert bare.guards_check_each(guards) == [i not in (0, 511, 512) for i in range(513)]
    # an empty Guard: whatever the oracle's pairing gives for two identities; among programmed Guards on the golden SRS
    ps, g0, g1, bases, pctx = programmed
    prog = [([(5, 0)], [(5, 0)]), ([], []), ([(3, 1)], []), ([(21, 0), (21, 4)], [(4, 6)])]
    exp = []
    for g in prog:
        l, r = _expected(g0, g1, bases, [g], [1])
        exp.append(circuits.oracle_pairing_check(ps, ref.affine_bytes(l), ref.affine_bytes(r)))
    assert pctx.guards_check_each([_bytes_guard(bases, g) for g in prog]) == exp
    assert exp[1] == circuits.oracle_pairing_check(ps, ZERO, ZERO)
