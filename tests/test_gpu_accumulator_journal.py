"""The leg journal of the resident accumulator (h2v_accumulator_journal_begin / check_legs / drop_legs): find the legs whose own
pairing fails and take them out again.

With the journal on, every successful process / add_msm call leaves an entry — its own sum (l, r), the product M of its draws, its
counters — and entry 0, the base, is the accumulator as it stood at journal_begin.  At every return

    (L, R) = sum_e W_e sum_e,     W_e = prod_{f > e} M_f

check_legs runs the pairing of every entry's sum; drop_legs rebuilds (L, R) from the kept entries, so that the accumulator, the
counters and the journal are those of an accumulator that was never given the dropped calls.  Every comparison is bit for bit, and
every expected value comes from the CPU oracle: batch_reference.expected (circuits.oracle_accumulate restated over cached Guards) for
the points, verdicts and statuses of any set of kept legs, circuits.oracle_pairing_check on the oracle's accumulation of a leg alone
for that leg's bit."""
import ctypes
import random

import pytest

import batch_reference
import circuits
import oracle_lib
from circuits import R_MOD
from test_gpu_identify import _make_bad

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
JOURNAL_MAX = 4096
ZERO = bytes(64)


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


class Leg:
    """one process call: items = [(setup, proof, instances)], one draw per item"""

    def __init__(self, items, draws):
        self.items, self.draws = list(items), list(draws)
        assert len(self.items) == len(self.draws)


def _process(acc, keyed, leg):
    """keyed: [(setup, context)], every leg given every context"""
    keys = [next(k for k, (s, _) in enumerate(keyed) if s is it[0]) for it in leg.items]
    return acc.process([c for _, c in keyed], keys, [p for _, p, _ in leg.items], [i for _, _, i in leg.items], leg.draws)


def _oracle(legs, setup):
    """-> (ok, statuses, left, right) of ONE accumulation over the legs' items with their draws concatenated"""
    return batch_reference.expected([it for l in legs for it in l.items], [d for l in legs for d in l.draws], setup=setup)


def _oracle_bit(leg, setup):
    """the pairing of the oracle's accumulation of that leg alone, and the leg's failure count"""
    _, st, left, right = _oracle([leg], setup)
    return len(leg.items), sum(1 for v in st if v), circuits.oracle_pairing_check(setup, left, right)


def _same_as(acc, legs, setup):
    """the accumulator equals the oracle's accumulation over `legs`: verdict, points and counters"""
    ok, st, left, right = _oracle(legs, setup)
    assert acc.read() == (left, right, len(st), sum(1 for v in st if v))
    assert acc.finalize() == (ok, left, right)
    return ok


def _raw(acc, name, *args):
    from halo2_verifier_amd import _lib
    return getattr(_lib.load_library(), name)(acc._h, *args)


def _raw_drop(acc, indices):
    return _raw(acc, "h2v_accumulator_drop_legs", (ctypes.c_size_t * max(len(indices), 1))(*indices), len(indices))


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


def _pool_legs(pool, sizes, seed, start=0):
    """legs of the given sizes over the pool's proofs, cycled from `start`, with distinct draws"""
    s, P, I, _ = pool
    draws = _draws(sum(sizes), seed)
    legs, at = [], 0
    for m in sizes:
        legs.append(Leg([(s, P[(start + at + j) % len(P)], I[(start + at + j) % len(P)]) for j in range(m)], draws[at:at + m]))
        at += m
    return legs


@pytest.fixture(scope="module")
def six_legs(pool):
    """Six legs of 4 proofs over the pool.  Pairing-only bad proofs (status 0, the pairing fails) of kinds 0 - 3 in legs 1 and 4; a
    non-canonical scalar (status -5) in leg 2.  -> (legs, bad positions)"""
    s, P, I, _ = pool
    P2, I2 = list(P), list(I)
    bad = {4: 0, 6: 1, 17: 2, 19: 3}
    for i, kind in bad.items():
        P2[i], I2[i] = _make_bad(P, I, i, kind)
        assert circuits.oracle_verify_single(s, P2[i], I2[i]) == -2, (i, kind)
    P2[9] = P2[9][:-96] + b"\xff" * 32 + P2[9][-64:]
    draws = _draws(24, 21)
    legs = [Leg([(s, P2[i], I2[i]) for i in range(4 * j, 4 * j + 4)], draws[4 * j:4 * j + 4]) for j in range(6)]
    return legs, sorted(bad)


@pytest.mark.parametrize("J", [1, 2, 9, 40])
def test_rebuild_reproduces_the_accumulator(pool, J):
    """drop_legs([]) rebuilds (L, R) = sum_e W_e sum_e from J entries: a scalar taken from another block, a prefix instead of a suffix
    product or a wrong slot map all change the bytes.  9 is the first count past the fold team's eight lanes; 40 puts several records
    on every lane."""
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    legs = _pool_legs(pool, [1 + (j * 7) % 4 for j in range(J)], seed=100 + J, start=J)
    acc = h2v.Accumulator(ctx, journal=J + 1)
    for leg in legs:
        assert _process(acc, [(s, ctx)], leg) == [0] * len(leg.items)
    assert _same_as(acc, legs, s) is True
    before = acc.read()
    assert acc.check_legs() == [(0, 0, True)] + [(len(l.items), 0, True) for l in legs]
    acc.drop_legs([])
    assert acc.read() == before
    assert _same_as(acc, legs, s) is True
    assert acc.check_legs() == [(0, 0, True)] + [(len(l.items), 0, True) for l in legs]
    acc.close()


def test_failing_legs_are_named_dropped_and_the_rest_stands(pool, six_legs):
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    legs, _ = six_legs
    acc = h2v.Accumulator(ctx, journal=8)
    st = []
    for leg in legs:
        st += _process(acc, [(s, ctx)], leg)
    whole = _oracle(legs, s)
    assert st == whole[1] and [i for i, v in enumerate(st) if v] == [9] and st[9] == -5
    got = acc.check_legs()
    assert got == [(0, 0, True)] + [_oracle_bit(l, s) for l in legs]
    assert [int(ok) for _, _, ok in got] == [1, 1, 0, 1, 1, 0, 1] and got[3][1] == 1
    assert _same_as(acc, legs, s) is False and whole[0] is False
    acc.drop_legs([2, 5])
    kept = [legs[0], legs[2], legs[3], legs[5]]
    assert _same_as(acc, kept, s) is False                      # by the failed status of leg 2, now entry 2
    assert acc.check_legs() == [(0, 0, True)] + [_oracle_bit(l, s) for l in kept]
    assert all(ok for _, _, ok in acc.check_legs()) and acc.check_legs()[2][1] == 1
    acc.drop_legs([2])
    kept = [legs[0], legs[3], legs[5]]
    assert _same_as(acc, kept, s) is True
    assert acc.check_legs() == [(0, 0, True)] + [(4, 0, True)] * 3
    acc.close()


def test_drop_continue_drop_again(pool):
    """Slots come back through the free list: drop the first non-base leg, go on, drop the last leg, go on, drop every non-base leg
    (W x an identity base: the zero bytes, counters 0 / 0, finalize true) — and the emptied accumulator goes on working."""
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    A, B, C, D, E, F, G, H = _pool_legs(pool, [2, 3, 1, 4, 2, 3, 1, 2], seed=31)
    keyed = [(s, ctx)]
    acc = h2v.Accumulator(ctx, journal=6)
    for leg in (A, B, C, D):
        _process(acc, keyed, leg)
    assert _same_as(acc, [A, B, C, D], s)
    acc.drop_legs([1])
    assert _same_as(acc, [B, C, D], s)
    _process(acc, keyed, E)                                     # takes the slot A left
    assert _same_as(acc, [B, C, D, E], s)
    acc.drop_legs([4])
    assert _same_as(acc, [B, C, D], s)
    _process(acc, keyed, F)
    _process(acc, keyed, G)                                     # the journal is full: base + 5
    assert _same_as(acc, [B, C, D, F, G], s)
    assert acc.check_legs() == [(0, 0, True)] + [(len(l.items), 0, True) for l in (B, C, D, F, G)]
    acc.drop_legs([3, 1, 5])                                    # in any order
    assert _same_as(acc, [C, F], s)
    acc.drop_legs([1, 2])
    assert acc.read() == (ZERO, ZERO, 0, 0) and acc.finalize() == (True, ZERO, ZERO) and acc.check_legs() == [(0, 0, True)]
    _process(acc, keyed, H)
    assert _same_as(acc, [H], s)
    acc.close()


def test_base_entry(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    keyed = [(s, ctx)]
    first, good, bad = _pool_legs(pool, [5, 3, 2], seed=41)
    bp, bi = _make_bad(P, I, 11, 0)
    assert circuits.oracle_verify_single(s, bp, bi) == -2
    bad = Leg([bad.items[0], (s, bp, bi)], bad.draws)
    acc = h2v.Accumulator(ctx)
    _process(acc, keyed, first)
    acc.journal_begin(4)
    assert _same_as(acc, [first], s)                            # the points and counters do not change
    _process(acc, keyed, bad)
    _process(acc, keyed, good)
    assert acc.check_legs() == [(5, 0, True), (2, 0, False), (3, 0, True)]
    assert _oracle_bit(bad, s) == (2, 0, False) and _oracle_bit(first, s) == (5, 0, True)
    before = acc.read()
    assert _raw_drop(acc, [0]) == BAD_ARGUMENT and _raw_drop(acc, [1, 0]) == BAD_ARGUMENT
    assert acc.read() == before and len(acc.check_legs()) == 3
    assert _same_as(acc, [first, bad, good], s) is False
    acc.drop_legs([1])
    assert _same_as(acc, [first, good], s) is True
    acc.journal_begin(2)                                        # a checkpoint: everything so far is one base
    assert acc.check_legs() == [(8, 0, True)]
    assert _same_as(acc, [first, good], s) is True
    acc.close()
    # the bad proof among the five: the base's own bit is 0
    spoiled = Leg(first.items[:2] + [(s, bp, bi)] + first.items[3:], first.draws)
    acc = h2v.Accumulator(ctx)
    _process(acc, keyed, spoiled)
    acc.journal_begin(4)
    _process(acc, keyed, good)
    assert acc.check_legs() == [(5, 0, False), (3, 0, True)] and _oracle_bit(spoiled, s) == (5, 0, False)
    assert _same_as(acc, [spoiled, good], s) is False
    acc.journal_begin(3)
    assert acc.check_legs() == [(8, 0, False)]
    acc.close()


def test_scale_edges_through_w(pool):
    """The rebuild multiplies entry A's sum by W_A, the product of the later kept entries' M: a leg of ONE proof with draw v behind A
    makes W_A = v.  Every GLV edge scalar, every programmed value, 0, 1 and r - 1, each rebuilt by dropping a throw-away leg, on one
    accumulator whose journal is begun once."""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    keyed = [(s, ctx)]
    values = list(dict.fromkeys(batch_reference.glv_edge_scalars() + batch_reference.programmed_values() + [0, 1, R_MOD - 1]))
    assert len(values) > 100 and all(0 <= v < R_MOD for v in values)
    A, T = _pool_legs(pool, [3, 2], seed=51)
    acc = h2v.Accumulator(ctx, journal=4)
    for t, v in enumerate(values):
        one = Leg([(s, P[5 + t % 4], I[5 + t % 4])], [v])
        for leg in (A, one, T):
            _process(acc, keyed, leg)
        acc.drop_legs([3])
        ok, st, left, right = _oracle([A, one], s)
        assert acc.read() == (left, right, 4, 0), (t, hex(v))
        acc.drop_legs([1, 2])
        assert acc.read() == (ZERO, ZERO, 0, 0), (t, hex(v))
    # r - 1 against the same proof: the scaled sum meets its negative, both points the identity
    d = _draws(1, 52)
    A1, neg = Leg([(s, P[0], I[0])], d), Leg([(s, P[0], I[0])], [R_MOD - 1])
    for leg in (A1, neg, T):
        _process(acc, keyed, leg)
    acc.drop_legs([3])
    assert _oracle([A1, neg], s) == (True, [0, 0], ZERO, ZERO)
    assert acc.read() == (ZERO, ZERO, 2, 0) and acc.finalize() == (True, ZERO, ZERO)
    acc.close()


def test_add_msm_entries(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    L_ = oracle_lib.load()
    keyed = [(s, ctx)]
    other, leg = _pool_legs(pool, [6, 3], seed=61, start=9)
    ok, _, seed_l, seed_r = _oracle([other], s)                 # another accepted batch's (L, R), as in test_seeds
    assert ok is True
    rnd = random.Random(62)
    a = rnd.randrange(1, R_MOD)
    twice_r = oracle_lib.g1_msm(L_, [2], [seed_r])              # (seed_l, 2 seed_r): sums that fail the pairing
    assert circuits.oracle_pairing_check(s, seed_l, seed_r) is True and circuits.oracle_pairing_check(s, seed_l, twice_r) is False
    acc = h2v.Accumulator(ctx, journal=5)
    acc.add_msm(([a, (1 - a) % R_MOD, 0, 5], [seed_l, seed_l, seed_r, bytes(64)]), ([1], [seed_r]))
    assert _process(acc, keyed, leg) == [0, 0, 0]
    acc.add_msm(([1], [seed_l]), ([2], [seed_r]))
    assert acc.check_legs() == [(0, 0, True), (0, 0, True), (3, 0, True), (0, 0, False)]
    seeded = batch_reference.expected(leg.items, leg.draws, seed=(seed_l, seed_r))
    assert seeded[0] is True
    both = (oracle_lib.g1_msm(L_, [1, 1], [seeded[2], seed_l]), oracle_lib.g1_msm(L_, [1, 1], [seeded[3], twice_r]))
    assert acc.read() == (*both, 3, 0) and acc.finalize() == (False, *both)
    acc.drop_legs([3])
    assert acc.read() == (seeded[2], seeded[3], 3, 0) and acc.finalize() == (True, seeded[2], seeded[3])
    acc.drop_legs([1])                                          # the accumulation without the seed
    assert _same_as(acc, [leg], s) is True and acc.check_legs() == [(0, 0, True), (3, 0, True)]
    acc.close()


def _mixed_lens(s, lens, seed):
    rnd = random.Random(seed)
    P, I = [], []
    for j, m in enumerate(lens):
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=seed * 100 + j)
        P.append(p); I.append(inst)
    return P, I


def test_several_keys_and_shapes_in_one_leg(two_keys):
    """A leg folds the records of several (key, shape) groups into ONE entry: the 64-item interleaving of two keys with per-proof
    shapes inside the first, cut into three legs, the middle one with a wrong public input."""
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    Pm, Im = _mixed_lens(s8, [8, 5, 8, 3, 5, 0, 8, 3], 9)
    first = [(s8, p, i) for p, i in zip(Pm, Im)] + [(s8, p, i) for p, i in A[8:]]
    items = []
    for x, y in zip(first, [(s4, p, i) for p, i in B]):
        items += [x, y]
    assert len(items) == 64
    sb, pb, ib = items[12]
    assert sb is s8
    items[12] = (s8, pb, [[circuits.le32((int.from_bytes(ib[0][0], "little") + 1) % R_MOD)] + ib[0][1:]])
    assert circuits.oracle_verify_single(s8, items[12][1], items[12][2]) == -2
    rand = _draws(64, 2)
    legs = [Leg(items[a:b], rand[a:b]) for a, b in ((0, 10), (10, 21), (21, 64))]
    keyed = [(s8, c8), (s4, c4)]
    acc = h2v.Accumulator(c8, journal=4)
    for leg in legs:
        assert _process(acc, keyed, leg) == [0] * len(leg.items)
    assert acc.check_legs() == [(0, 0, True)] + [_oracle_bit(l, s8) for l in legs] == [(0, 0, True), (10, 0, True), (11, 0, False), (43, 0, True)]
    assert _same_as(acc, legs, s8) is False
    before = acc.read()
    acc.drop_legs([])
    assert acc.read() == before
    acc.drop_legs([2])
    assert _same_as(acc, [legs[0], legs[2]], s8) is True
    acc.close()


def test_gwc_keccak_legs():
    """GWC + Keccak: the left channel of every Guard is a real MSM"""
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 6).set_options(circuits.GWC, circuits.KECCAK256)
    P, I = circuits.prove_vector_mul_batch(s, 9, seed=77, threads=4)
    P[4], I[4] = _make_bad(P, I, 4, 0)
    assert circuits.oracle_verify_single(s, P[4], I[4]) == -2
    ctx = _ctx(s)
    rand = _draws(9, 71)
    legs = [Leg([(s, P[i], I[i]) for i in range(a, a + 3)], rand[a:a + 3]) for a in (0, 3, 6)]
    acc = h2v.Accumulator(ctx, journal=4)
    for leg in legs:
        assert _process(acc, [(s, ctx)], leg) == [0, 0, 0]
    assert acc.check_legs() == [(0, 0, True)] + [_oracle_bit(l, s) for l in legs] == [(0, 0, True), (3, 0, True), (3, 0, False), (3, 0, True)]
    assert _same_as(acc, legs, s) is False
    acc.drop_legs([2])
    assert _same_as(acc, [legs[0], legs[2]], s) is True
    acc.close()
    ctx.close()
    s.free()


def test_refusals_and_atomicity(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    keyed = [(s, ctx)]
    A, B, C = _pool_legs(pool, [2, 3, 1], seed=81)
    bp, bi = _make_bad(P, I, 3, 1)
    B = Leg(B.items[:2] + [(s, bp, bi)], B.draws)               # a failing leg, so that the state is not all ones
    seed = (([1], [bytes(64)]), ([], []))

    def state(acc):
        return acc.read(), acc.check_legs(), acc.finalize()

    # the journal off
    acc = h2v.Accumulator(ctx)
    n = ctypes.c_size_t(77)
    assert _raw(acc, "h2v_accumulator_check_legs", 0, ctypes.byref(n), None, None, None) == 0 and n.value == 0
    assert acc.check_legs() == []
    assert _raw_drop(acc, []) == BAD_ARGUMENT and _raw_drop(acc, [1]) == BAD_ARGUMENT
    for cap in (1, JOURNAL_MAX + 1):
        assert _raw(acc, "h2v_accumulator_journal_begin", cap) == BAD_ARGUMENT
        with pytest.raises(ValueError):
            acc.journal_begin(cap)
    assert acc.check_legs() == [] and acc.read() == (ZERO, ZERO, 0, 0)
    # the journal on
    acc.journal_begin(3)
    _process(acc, keyed, A)
    assert acc.process(ctx, None, [], [], []) == [] and len(acc.check_legs()) == 2          # n == 0 appends nothing
    before = state(acc)
    with pytest.raises(h2v.H2VError) as e:                                                   # a draw that is not canonical
        acc.process(ctx, None, P[:2], I[:2], [1, R_MOD])
    assert e.value.code == BAD_ARGUMENT and state(acc) == before
    _process(acc, keyed, B)
    before = state(acc)
    assert before[1] == [(0, 0, True), (2, 0, True), (3, 0, False)] and before[2][0] is False
    with pytest.raises(h2v.H2VError) as e:                                                   # the journal is full
        _process(acc, keyed, C)
    assert e.value.code == UNSUPPORTED and state(acc) == before
    with pytest.raises(h2v.H2VError) as e:
        acc.add_msm(*seed)
    assert e.value.code == UNSUPPORTED and state(acc) == before
    for indices in ([3], [1, 1], [0], [2, 1, 2], [1, JOURNAL_MAX]):                          # out of range, twice, the base
        assert _raw_drop(acc, indices) == BAD_ARGUMENT and state(acc) == before, indices
    for bad in ([3], [1, 1], [0]):
        with pytest.raises(ValueError):
            acc.drop_legs(bad)
    assert state(acc) == before
    # arrays shorter than the journal: refused, the entry count still written
    for cap in (0, 2):
        n = ctypes.c_size_t(77)
        ok = (ctypes.c_int * 3)(7, 7, 7)
        assert _raw(acc, "h2v_accumulator_check_legs", cap, ctypes.byref(n), None, None, ok) == BAD_ARGUMENT
        assert n.value == 3 and list(ok) == [7, 7, 7] and state(acc) == before
    assert _same_as(acc, [A, B], s) is False
    acc.drop_legs([2])
    _process(acc, keyed, C)                                                                  # room again
    assert _same_as(acc, [A, C], s) is True
    acc.journal_begin(0)                                                                     # off: the entries forgotten, the points kept
    assert acc.check_legs() == [] and _raw_drop(acc, []) == BAD_ARGUMENT
    _process(acc, keyed, B)
    acc.add_msm(*seed)
    assert _same_as(acc, [A, C, B], s) is False
    acc.close()


def test_identify_names_the_proofs_of_the_failing_legs(pool, six_legs):
    import halo2_verifier_amd as h2v
    s, _, _, ctx = pool
    legs, bad = six_legs
    acc = h2v.Accumulator(ctx, journal=8, keep_inputs=True)
    for j, leg in enumerate(legs):
        if j % 2:
            _process(acc, [(s, ctx)], leg)
        else:                                                   # the one-key form
            acc.process(ctx, None, [p for _, p, _ in leg.items], [i for _, _, i in leg.items], leg.draws)
    got = acc.identify()
    assert sorted(got) == [2, 5]
    for e in (2, 5):
        leg = legs[e - 1]
        single = [circuits.oracle_verify_single(s, p, i) for _, p, i in leg.items]
        assert got[e] == single == ctx.verify_each([p for _, p, _ in leg.items], [i for _, _, i in leg.items])
        assert [4 * (e - 1) + j for j, v in enumerate(single) if v] == [i for i in bad if i // 4 == e - 1]
    acc.drop_legs([2, 5])                                       # retained inputs follow the journal
    assert acc.identify() == {}
    _process(acc, [(s, ctx)], legs[4])
    assert sorted(acc.identify()) == [5] and acc.identify()[5] == got[5]
    acc.journal_begin(4)                                        # ... and are forgotten by journal_begin
    assert acc.identify() == {} and acc.check_legs() == [(20, 1, False)]
    acc.close()
    acc = h2v.Accumulator(ctx, journal=8)
    with pytest.raises(ValueError):
        acc.identify()
    acc.close()
