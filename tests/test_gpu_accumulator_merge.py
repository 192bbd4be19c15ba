"""Merging resident accumulators (h2v_accumulator_merge / export_state / merge_states): one pairing for K accumulators.

    (L, R) <- (L, R) + sum_k c_k (L_k, R_k),     n_proofs += sum_k n_proofs_k,     n_failed += sum_k n_failed_k

Every expected value comes from the CPU oracle and is compared bit for bit: batch_reference.expected gives each accumulator's own
points, oracle_lib.g1_msm over [1, c_1 ..] and the affine points gives the merged points, circuits.oracle_pairing_check the
verdicts.  The wide path (up to H2V_ACC_MERGE_MAX = 512 sources) goes through merge_states over states the test composes from
oracle points in the documented layout: no 512 accumulator objects are created (each owns a stream)."""
import ctypes
import random

import pytest

import batch_reference
import circuits
import merge_reference as mr
import oracle_lib
from circuits import R_MOD
from test_gpu_accumulator_journal import Leg, _ctx, _draws, _oracle, _process
from test_gpu_identify import _make_bad

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
ZERO = bytes(64)


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 32, seed=909, threads=8)
    ctx = _ctx(s)
    yield s, P, I, ctx
    ctx.close()
    s.free()


@pytest.fixture(scope="module")
def lib():
    return oracle_lib.load()


_MEMO = {}


def _legs(pool, sizes, seed, start=0):
    s, P, I, _ = pool
    draws = _draws(sum(sizes), seed)
    legs, at = [], 0
    for m in sizes:
        legs.append(Leg([(s, P[(start + at + j) % len(P)], I[(start + at + j) % len(P)]) for j in range(m)], draws[at:at + m]))
        at += m
    return legs


def _own(pool, legs):
    """the oracle's accumulation over these legs alone -> (points ok and no status, statuses, left, right), computed once per set of legs"""
    key = tuple((tuple(it[1] for it in l.items), tuple(l.draws)) for l in legs)
    if key not in _MEMO:
        _MEMO[key] = _oracle(legs, pool[0]) if legs else (True, [], ZERO, ZERO)
    return _MEMO[key]


def _fed(pool, legs, journal=0):
    """an accumulator fed these legs; journal: begun AFTER the legs, which are its base"""
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    acc = h2v.Accumulator(ctx)
    for leg in legs:
        _process(acc, [(s, ctx)], leg)
    if journal:
        acc.journal_begin(journal)
    return acc


def _merged(lib, dst, srcs, draws):
    """the oracle's merge: dst and srcs as (left, right, n_proofs, n_failed) -> the same"""
    left = oracle_lib.g1_msm(lib, [1] + list(draws), [dst[0]] + [x[0] for x in srcs])
    right = oracle_lib.g1_msm(lib, [1] + list(draws), [dst[1]] + [x[1] for x in srcs])
    return left, right, dst[2] + sum(x[2] for x in srcs), dst[3] + sum(x[3] for x in srcs)


def _state_of(own):
    _, st, left, right = own
    return left, right, len(st), sum(1 for v in st if v)


def _check(pool, acc, want):
    """read() and finalize() of acc against the oracle's (left, right, n_proofs, n_failed)"""
    assert acc.read() == want
    ok = circuits.oracle_pairing_check(pool[0], want[0], want[1]) and not want[3]
    assert acc.finalize() == (ok, want[0], want[1])
    return ok


def _raw(name, *args):
    from halo2_verifier_amd import _lib
    return getattr(_lib.load_library(), name)(*args)


def _handles(accs):
    return (ctypes.c_void_p * max(len(accs), 1))(*[a._h.value for a in accs])


def _scalars(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


# ---------------------------------------------------------------------------------------------------------------- merge equals the oracle
@pytest.mark.parametrize("K,dst_fed", [(1, False), (2, True), (3, False), (9, True)])
def test_merged_accumulators_equal_the_oracle(pool, lib, K, dst_fed):
    src_legs = [_legs(pool, [1 + (k + j) % 3 for j in range(1 + k % 3)], seed=300 + k, start=3 * k) for k in range(K)]
    dst_legs = _legs(pool, [2, 1], seed=299, start=7) if dst_fed else []
    srcs = [_fed(pool, legs) for legs in src_legs]
    dst = _fed(pool, dst_legs)
    before = [a.read() for a in srcs]
    assert before == [_state_of(_own(pool, legs)) for legs in src_legs]
    draws = _draws(K, 310 + K)
    used = dst.merge(srcs, draws)
    assert used == [d.to_bytes(32, "little") for d in draws]
    want = _merged(lib, _state_of(_own(pool, dst_legs)), before, draws)
    assert _check(pool, dst, want) is True
    assert [a.read() for a in srcs] == before                       # the sources are unchanged
    for a, legs in zip(srcs, src_legs):
        assert a.finalize()[0] is True
    # OS draws: returned, non-zero, and the points are the oracle's merge under them
    fresh = _fed(pool, [])
    used = fresh.merge(srcs)
    cs = [int.from_bytes(c, "little") for c in used]
    assert len(cs) == K and all(0 < c < R_MOD for c in cs) and len(set(cs)) == K
    assert _check(pool, fresh, _merged(lib, (ZERO, ZERO, 0, 0), before, cs)) is True
    for a in srcs + [dst, fresh]:
        a.close()


# ---------------------------------------------------------------------------------------------------------------- the wide path
def _oracle_states(pool, lib, K, seed):
    """K states over oracle points: multiples of one accepted accumulator (so every state passes the pairing), some identities"""
    ok, st, left, right = _own(pool, _legs(pool, [3], seed=77, start=1))
    assert ok is True
    rnd = random.Random(seed)
    states, tuples = [], []
    for k in range(K):
        m = 0 if k % 17 == 5 else rnd.randrange(1, R_MOD)
        t = (oracle_lib.g1_msm(lib, [m], [left]), oracle_lib.g1_msm(lib, [m], [right]), k % 5, 0)
        tuples.append(t)
        states.append(mr.pack_state(*t))
    return states, tuples


@pytest.mark.parametrize("K", [63, 64, 65, 130, 512])
def test_wide_merge_through_states(pool, lib, K):
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    states, tuples = _oracle_states(pool, lib, K, seed=K)
    draws = _draws(K, 400 + K)
    base_legs = _legs(pool, [2], seed=401, start=11)
    dst = _fed(pool, base_legs, journal=K + 1)
    assert dst.merge_states(states, draws) == [d.to_bytes(32, "little") for d in draws]
    want = _merged(lib, _state_of(_own(pool, base_legs)), tuples, draws)
    assert _check(pool, dst, want) is True
    legs = dst.check_legs()
    assert legs == [(2, 0, True)] + [(t[2], 0, True) for t in tuples]
    # the journal's slots hold c_k (L_k, R_k): dropping every source but the last gives base + c_K state_K
    dst.drop_legs(list(range(1, K)))
    assert _check(pool, dst, _merged(lib, _state_of(_own(pool, base_legs)), tuples[-1:], draws[-1:])) is True
    dst.close()


def test_more_than_merge_max_is_refused(pool, lib):
    states, _ = _oracle_states(pool, lib, 2, seed=1)
    dst = _fed(pool, _legs(pool, [1], seed=402))
    before = dst.read()
    many = b"".join(states[k % 2] for k in range(513))
    assert _raw("h2v_accumulator_merge_states", dst._h, many, 513, _scalars([1] * 513), None) == BAD_ARGUMENT
    with pytest.raises(ValueError):
        dst.merge_states([states[0]] * 513, [1] * 513)
    assert dst.read() == before
    dst.close()


def test_state_round_trip(pool):
    legs = _legs(pool, [3, 2], seed=410, start=4)
    src, dst = _fed(pool, legs), _fed(pool, [])
    state = src.export_state()
    left, right, n, f = src.read()
    assert state == mr.pack_state(left, right, n, f) and len(state) == 152
    import halo2_verifier_amd as h2v
    assert h2v.Accumulator.unpack_state(state) == (left, right, n, f) and h2v.Accumulator.pack_state(left, right, n, f) == state
    dst.merge_states([state], [1])
    assert dst.export_state() == state and dst.read() == src.read()
    assert dst.finalize() == src.finalize()
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- draw edges
def test_draw_edges(pool, lib):
    legs_a, legs_b = _legs(pool, [2], seed=420, start=2), _legs(pool, [3], seed=421, start=9)
    a, b = _state_of(_own(pool, legs_a)), _state_of(_own(pool, legs_b))
    sa, sb = mr.pack_state(*a), mr.pack_state(*b)
    values = list(dict.fromkeys([1, R_MOD - 1] + batch_reference.glv_edge_scalars() + batch_reference.programmed_values()))
    assert len(values) > 100 and all(0 < v < R_MOD for v in values)
    dst = _fed(pool, legs_b, journal=3)
    for at in range(0, len(values), 2):                             # two draws per call, the journal emptied in between
        cs = (values[at:at + 2] + [1])[:2]
        dst.merge_states([sa, sb], cs)
        assert dst.read() == _merged(lib, b, [a, b], cs), [hex(c) for c in cs]
        dst.drop_legs([1, 2])
        assert dst.read() == b
    dst.close()
    # identity sources, onto an empty and onto a fed destination
    ident = mr.pack_state(ZERO, ZERO, 4, 0)
    dst = _fed(pool, [])
    dst.merge_states([ident, ident], [5, R_MOD - 1])
    assert dst.read() == (ZERO, ZERO, 8, 0) and dst.finalize() == (True, ZERO, ZERO)
    dst.merge_states([sa, ident], [7, 9])
    assert dst.read() == _merged(lib, (ZERO, ZERO, 8, 0), [a, (ZERO, ZERO, 4, 0)], [7, 9])
    dst.close()
    # a source equal to -dst: the merge is the identity, read gives all-zero bytes
    src, dst = _fed(pool, legs_a), _fed(pool, legs_a)
    dst.merge([src], [R_MOD - 1])
    assert dst.read() == (ZERO, ZERO, 2 * a[2], 0) and dst.finalize() == (True, ZERO, ZERO)
    # two equal sources with c and r - c cancel each other
    other, dst2 = _fed(pool, legs_a), _fed(pool, legs_b)
    c = _draws(1, 422)[0]
    dst2.merge([src, other], [c, R_MOD - c])
    assert dst2.read() == (b[0], b[1], b[2] + 2 * a[2], 0) and dst2.finalize()[0] is True
    for x in (src, dst, other, dst2):
        x.close()


def test_a_status_failed_proof_in_a_source(pool, lib):
    s, P, I, _ = pool
    good, spoiled = _legs(pool, [2], seed=430), _legs(pool, [3], seed=431, start=5)
    p = spoiled[0].items[1][1]
    spoiled[0].items[1] = (s, p[:-96] + b"\xff" * 32 + p[-64:], spoiled[0].items[1][2])     # a non-canonical scalar: status -5
    own = _own(pool, spoiled)
    assert own[1] == [0, -5, 0] and circuits.oracle_pairing_check(s, own[2], own[3]) is True
    src, dst = _fed(pool, spoiled), _fed(pool, good, journal=3)
    dst.merge([src], [11])
    want = _merged(lib, _state_of(_own(pool, good)), [_state_of(own)], [11])
    assert want[2:] == (5, 1) and circuits.oracle_pairing_check(s, want[0], want[1]) is True
    assert _check(pool, dst, want) is False                          # not ok, while the pairing bit is 1
    assert dst.check_legs() == [(2, 0, True), (3, 1, True)]
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------------------------- journal
def test_journal_names_and_drops_a_bad_source(pool, lib):
    s, P, I, ctx = pool
    src_legs = [_legs(pool, [2, 1], seed=440 + k, start=4 * k) for k in range(4)]
    bp, bi = _make_bad(P, I, 9, 0)
    assert circuits.oracle_verify_single(s, bp, bi) == -2
    src_legs[2][1] = Leg([(s, bp, bi)], src_legs[2][1].draws)
    owns = [_own(pool, legs) for legs in src_legs]
    assert [circuits.oracle_pairing_check(s, o[2], o[3]) for o in owns] == [True, True, False, True]
    srcs = [_fed(pool, legs) for legs in src_legs]
    base = _legs(pool, [2], seed=449, start=20)
    dst = _fed(pool, base, journal=8)
    draws = _draws(4, 450)
    dst.merge(srcs, draws)
    tuples = [_state_of(o) for o in owns]
    b = _state_of(_own(pool, base))
    assert _check(pool, dst, _merged(lib, b, tuples, draws)) is False
    assert dst.check_legs() == [(2, 0, True), (3, 0, True), (3, 0, True), (3, 0, False), (3, 0, True)]
    dst.drop_legs([3])
    kept = [0, 1, 3]
    assert _check(pool, dst, _merged(lib, b, [tuples[k] for k in kept], [draws[k] for k in kept])) is True
    assert dst.check_legs() == [(2, 0, True)] + [(3, 0, True)] * 3
    # process after a merge, then a second merge: (L, R) <- M (everything so far) + the leg, then + c (source)
    more = _legs(pool, [2], seed=451, start=25)
    _process(dst, [(s, ctx)], more[0])
    M = more[0].draws[0] * more[0].draws[1] % R_MOD
    so_far = _merged(lib, b, [tuples[k] for k in kept], [draws[k] for k in kept])
    leg_own = _state_of(_own(pool, more))
    after_leg = _merged(lib, (ZERO, ZERO, 0, 0), [so_far, leg_own], [M, 1])
    assert dst.read() == after_leg
    dst.merge([srcs[1]], [13])
    assert _check(pool, dst, _merged(lib, after_leg, [tuples[1]], [13])) is True
    assert dst.check_legs() == [(2, 0, True)] + [(3, 0, True)] * 3 + [(2, 0, True), (3, 0, True)]
    dst.drop_legs([4])                                               # the leg out again: W of the entries before it returns to 1
    assert _check(pool, dst, _merged(lib, so_far, [tuples[1]], [13])) is True
    # fewer free entries than sources: refused as a whole, nothing changes
    state = (dst.read(), dst.check_legs(), dst.finalize())
    assert len(state[1]) == 5                                        # 3 free of 8
    import halo2_verifier_amd as h2v
    with pytest.raises(h2v.H2VError) as e:
        dst.merge(srcs, draws)
    assert e.value.code == UNSUPPORTED and (dst.read(), dst.check_legs(), dst.finalize()) == state
    assert _raw("h2v_accumulator_merge_states", dst._h, b"".join(mr.pack_state(*t) for t in tuples), 4, _scalars(draws), None) == UNSUPPORTED
    assert (dst.read(), dst.check_legs(), dst.finalize()) == state
    dst.merge(srcs[:3], draws[:3])                                   # exactly the free entries
    assert len(dst.check_legs()) == 8
    for a in srcs + [dst]:
        a.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_everything_unchanged(pool, lib):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    legs = _legs(pool, [2, 1], seed=460)
    dst, src, src2 = _fed(pool, legs, journal=6), _fed(pool, legs[:1]), _fed(pool, legs[1:])
    state = lambda: (dst.read(), dst.check_legs())
    before = state()
    one = _scalars([1])
    good = mr.pack_state(*_state_of(_own(pool, legs[:1])))
    left, right = good[24:88], good[88:152]

    def merge(srcs, n, draws, d=dst):
        return _raw("h2v_accumulator_merge", d._h if d else None, _handles(srcs) if srcs is not None else None, n, draws, None)

    def merge_states(states, n, draws):
        return _raw("h2v_accumulator_merge_states", dst._h, states, n, draws, None)

    off_curve = left[:32] + (int.from_bytes(left[32:], "little") ^ 1).to_bytes(32, "little")
    x_not_canonical = (int.from_bytes(left[:32], "little") + mr.ref.P).to_bytes(32, "little") + left[32:]    # x + p < 2^256: the same residue
    cases = [
        ("null sources", lambda: merge(None, 1, one)),
        ("null destination", lambda: merge([src], 1, one, d=None)),
        ("too many sources", lambda: _raw("h2v_accumulator_merge", dst._h, (ctypes.c_void_p * 513)(*[src._h.value] * 513), 513, _scalars([1] * 513), None)),
        ("a source equal to dst", lambda: merge([src, dst], 2, _scalars([1, 2]))),
        ("a source given twice", lambda: merge([src, src2, src], 3, _scalars([1, 2, 3]))),
        ("a draw not canonical", lambda: merge([src, src2], 2, _scalars([1, R_MOD]))),
        ("a zero draw", lambda: merge([src, src2], 2, _scalars([3, 0]))),
        ("null states", lambda: merge_states(None, 1, one)),
        ("a zero draw for a state", lambda: merge_states(good, 1, _scalars([0]))),
        ("a draw not canonical for a state", lambda: merge_states(good, 1, _scalars([R_MOD + 1]))),
        ("a wrong magic", lambda: merge_states(mr.pack_state(left, right, 1, 0, magic=mr.STATE_MAGIC + 1), 1, one)),
        ("a wrong version", lambda: merge_states(mr.pack_state(left, right, 1, 0, version=2), 1, one)),
        ("n_failed > n_proofs", lambda: merge_states(mr.pack_state(left, right, 1, 2), 1, one)),
        ("a point off the curve", lambda: merge_states(good + mr.pack_state(off_curve, right, 1, 0), 2, _scalars([1, 1]))),
        ("a right point off the curve", lambda: merge_states(mr.pack_state(left, off_curve, 1, 0), 1, one)),
        ("a coordinate not canonical", lambda: merge_states(mr.pack_state(x_not_canonical, right, 1, 0), 1, one)),
    ]
    for name, call in cases:
        assert call() == BAD_ARGUMENT, name
        assert state() == before, name
    assert dst.finalize()[0] is True
    # n == 0 changes nothing and needs no pointers
    assert merge(None, 0, None) == 0 and merge_states(None, 0, None) == 0 and state() == before
    # the mirror's own checks
    with pytest.raises(ValueError):
        dst.merge([src, src])
    with pytest.raises(ValueError):
        dst.merge([dst])
    with pytest.raises(ValueError):
        dst.merge([src], [1, 2])
    with pytest.raises(TypeError):
        dst.merge([object()])
    with pytest.raises(ValueError):
        dst.merge_states([good[:-1]])
    assert state() == before
    for a in (dst, src, src2):
        a.close()


def test_a_source_over_other_params_is_refused(pool):
    """same_srs compares g[0], g2 and s_g2: an accumulator over a context of another SRS (another secret) is refused as a source"""
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    other = circuits.setup_vector_mul(8, 8, s_seed=43)
    assert other.params != s.params
    other_ctx = h2v.Context(h2v.ParamsKZG(other.params, h2v.SerdeFormat.RawBytes))
    dst = _fed(pool, _legs(pool, [1], seed=470), journal=3)
    src = h2v.Accumulator(other_ctx)
    before = (dst.read(), dst.check_legs())
    assert _raw("h2v_accumulator_merge", dst._h, _handles([src]), 1, _scalars([1]), None) == BAD_ARGUMENT
    assert (dst.read(), dst.check_legs()) == before
    src.close(); dst.close(); other_ctx.close()
    other.free()


# ---------------------------------------------------------------------------------------------------------------- Keccak
def test_gwc_keccak_beside_shplonk_blake2b(lib):
    """accumulators fed through contexts of different multiopen schemes and transcripts over the same params merge under one pairing"""
    import halo2_verifier_amd as h2v
    sa = circuits.setup_vector_mul(8, 6)
    sb = circuits.setup_vector_mul(8, 6).set_options(circuits.GWC, circuits.KECCAK256)
    assert sa.params == sb.params
    Pa, Ia = circuits.prove_vector_mul_batch(sa, 3, seed=81, threads=4)
    Pb, Ib = circuits.prove_vector_mul_batch(sb, 3, seed=82, threads=4)
    ca, cb = _ctx(sa), _ctx(sb)
    la, lb = Leg([(sa, p, i) for p, i in zip(Pa, Ia)], _draws(3, 83)), Leg([(sb, p, i) for p, i in zip(Pb, Ib)], _draws(3, 84))
    a, b = h2v.Accumulator(ca), h2v.Accumulator(cb)
    assert _process(a, [(sa, ca)], la) == [0, 0, 0] and _process(b, [(sb, cb)], lb) == [0, 0, 0]
    oa, ob = _oracle([la], sa), _oracle([lb], sb)
    assert oa[0] is True and ob[0] is True
    dst = h2v.Accumulator(ca, journal=3)
    cs = _draws(2, 85)
    dst.merge([a, b], cs)
    want = _merged(lib, (ZERO, ZERO, 0, 0), [(oa[2], oa[3], 3, 0), (ob[2], ob[3], 3, 0)], cs)
    assert dst.read() == want and dst.finalize() == (True, want[0], want[1])
    assert circuits.oracle_pairing_check(sa, want[0], want[1]) is True
    assert dst.check_legs() == [(0, 0, True), (3, 0, True), (3, 0, True)]
    for x in (a, b, dst):
        x.close()
    ca.close(); cb.close()
    sa.free(); sb.free()
