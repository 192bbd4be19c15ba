"""The exact batch reference (tests/batch_reference.py) against the oracle's own restatement of the reference's AccumulatorStrategy
(circuits.oracle_verify_batch: every Guard scaled by its O(n) product of later draws) — for every draw pattern the GPU tests use, both
multi-open schemes and both transcripts, with a proof that fails early and one that only the pairing rejects, per group of a grouped
launch, with a seed, and for several keys against circuits.oracle_accumulate.  No GPU."""
import random

import pytest

import batch_reference as br
import circuits
import oracle_lib
from circuits import R_MOD

N = 16


def _setup(multiopen, transcript):
    return circuits.setup_vector_mul(8, 8).set_options(multiopen, transcript)


@pytest.fixture(scope="module")
def shplonk():
    s = _setup(circuits.SHPLONK, circuits.BLAKE2B)
    P, I = circuits.prove_vector_mul_batch(s, 64, seed=31, threads=8)
    yield s, P, I
    s.free()


def _patterns(n):
    """(name, proofs index list, draws): every draw pattern of tests/test_gpu_batch_structured.py on n proofs"""
    pairs = [i // 2 for i in range(n)]                      # adjacent duplicated pairs
    return [("random", list(range(n)), br.pattern_draws("random", n, 1)),
            ("ones distinct", list(range(n)), br.pattern_draws("ones", n)),
            ("ones repeated", [3] * n, br.pattern_draws("ones", n)),
            ("alternating pairs", pairs, br.pattern_draws("alternating", n)),
            ("alternating distinct", list(range(n)), br.pattern_draws("alternating", n)),
            ("zero at 1", list(range(n)), br.pattern_draws("zero_at", n, 2, k=1)),
            ("zero at n/2", list(range(n)), br.pattern_draws("zero_at", n, 3, k=n // 2)),
            ("zero at n-1", list(range(n)), br.pattern_draws("zero_at", n, 4, k=n - 1)),
            ("zero at 0", list(range(n)), br.pattern_draws("zero_at", n, 5, k=0)),
            ("programmed", list(range(n)), br.pattern_draws("programmed", n, 6))]


def _spoil(P, I, early=None, pairing=None):
    P, I = list(P), list(I)
    if early is not None:                                   # an undecodable point: a status, the proof leaves the accumulators
        b = bytearray(P[early]); b[32:64] = b"\xff" * 32; P[early] = bytes(b)
    if pairing is not None:                                 # a wrong public input: only the pairing rejects
        I[pairing] = [[circuits.le32(12345)] + list(I[pairing][0][1:])]
    return P, I


def test_multipliers_and_their_inverse():
    rnd = random.Random(3)
    d = [rnd.randrange(1, R_MOD) for _ in range(12)]
    m = br.multipliers(d)
    assert m[-1] == 1 and m[0] == d[1] * d[2] % R_MOD * br.multipliers(d[2:])[0] % R_MOD
    assert br.multipliers(br.draws_for(m)) == m
    mg = br.multipliers(d, groups=3)
    assert mg == br.multipliers(d[:4]) + br.multipliers(d[4:8]) + br.multipliers(d[8:])
    assert br.multipliers(br.draws_for(mg, groups=3), groups=3) == mg
    pm = br.programmed_multipliers(40, groups=2)
    assert br.multipliers(br.draws_for(pm, groups=2), groups=2) == pm and pm[19] == pm[39] == 1
    # a zero draw zeroes every earlier multiplier; the first draw scales nothing
    z = br.multipliers(br.pattern_draws("zero_at", 12, 0, k=5))
    assert z[:5] == [0] * 5 and all(z[5:])
    assert br.multipliers([0] + d[1:]) == br.multipliers(d)
    for k in br.programmed_values():
        k1, k2 = br.glv_split(k)
        assert (k1 + k2 * br.LAMBDA - k) % R_MOD == 0 and abs(k1) < 1 << 128 and abs(k2) < 1 << 128


def test_shplonk_left_channel_is_one_term_with_scalar_one(shplonk):
    """What lets programmed draws set the pooled left MSM's scalars: under SHPLONK a Guard's left channel is [1] x pi"""
    s, P, I = shplonk
    rc, g = circuits.oracle_guard(s, P[0], I[0])
    assert rc == 0 and [int.from_bytes(x, "little") for x in g["left_scalars"]] == [1]
    m = br.programmed_multipliers(8)
    pis = [circuits.oracle_guard(s, P[i], I[i])[1]["left_bases"][0] for i in range(8)]
    got = br.expected([(s, P[i], I[i]) for i in range(8)], br.draws_for(m))
    assert got[2] == oracle_lib.g1_msm(s.L, m, pis)


@pytest.mark.parametrize("multiopen,transcript", [(circuits.SHPLONK, circuits.BLAKE2B), (circuits.SHPLONK, circuits.KECCAK256),
                                                  (circuits.GWC, circuits.BLAKE2B), (circuits.GWC, circuits.KECCAK256)])
def test_every_pattern_equals_the_quadratic_oracle(multiopen, transcript):
    s = _setup(multiopen, transcript)
    P, I = circuits.prove_vector_mul_batch(s, N, seed=40 + 2 * multiopen + transcript, threads=8)
    try:
        for name, idx, draws in _patterns(N):
            Pn, In = [P[i] for i in idx], [I[i] for i in idx]
            for early, pairing in ((None, None), (N - 3, None), (None, N // 2 + 1)):
                Ps, Is = _spoil(Pn, In, early, pairing)
                exp = circuits.oracle_verify_batch(s, Ps, Is, draws)
                got = br.expected([(s, p, i) for p, i in zip(Ps, Is)], draws)
                assert got == exp, (name, early, pairing)
                if early is not None:
                    assert got[0] is False and got[1][early] != 0
                elif pairing is not None:
                    assert got[1] == [0] * N and got[0] is (name == "zero at n-1")   # only there the bad proof drops out
                else:
                    assert got[0] is True
                    assert (got[2] == got[3] == br.ZERO) is (name == "alternating pairs")   # everything cancels
    finally:
        s.free()


def test_64_proofs_and_groups(shplonk):
    s, P, I = shplonk
    n = 64
    rnd = random.Random(8)
    draws = [rnd.randrange(1, R_MOD) for _ in range(n)]
    draws[20] = 0
    items = [(s, P[i], I[i]) for i in range(n)]
    assert br.expected(items, draws) == circuits.oracle_verify_batch(s, P[:n], I[:n], draws)
    Ps, Is = _spoil(P[:n], I[:n], early=5, pairing=50)
    items = [(s, p, i) for p, i in zip(Ps, Is)]
    for G in (1, 2, 4):
        oks, st, lefts, rights = br.expected_groups(items, draws, G)
        gs = n // G
        for g in range(G):
            sl = slice(g * gs, (g + 1) * gs)
            assert (oks[g], st[sl], lefts[g], rights[g]) == circuits.oracle_verify_batch(s, Ps[sl], Is[sl], draws[sl]), (G, g)
    # a range: the launch's multipliers over [first, first + count)
    first, count = 36, 10
    m = br.multipliers(draws)
    ok, left, right = br.expected_range(items, draws, first, count)
    exp = circuits.oracle_verify_batch(s, Ps[first:first + count], Is[first:first + count], draws[first:first + count])
    scale = m[first + count - 1]                       # the range's own multipliers times the launch's multiplier of its last proof
    assert left == oracle_lib.g1_msm(s.L, [scale], [exp[2]]) and right == oracle_lib.g1_msm(s.L, [scale], [exp[3]]) and ok


def test_seeded(shplonk):
    """A seed is scaled by the product of ALL draws: seeding with the negation of a batch's own accumulators and draws whose product
    is 1 gives the identity; a zero first draw zeroes the seed."""
    s, P, I = shplonk
    n = 12
    items = [(s, P[i], I[i]) for i in range(n)]
    m = br.programmed_multipliers(n)
    draws = br.draws_for(m, first=pow(m[0], -1, R_MOD))        # d_0 m_0 = 1: the product of all draws
    ok, st, left, right = br.expected(items, draws)
    assert ok
    neg = lambda pt: oracle_lib.g1_msm(s.L, [R_MOD - 1], [pt])
    assert br.expected(items, draws, seed=(neg(left), neg(right))) == (True, [0] * n, br.ZERO, br.ZERO)
    other = br.expected([(s, P[i], I[i]) for i in range(20, 26)], br.pattern_draws("random", 6, 2))
    z = [0] + draws[1:]
    assert br.expected(items, z, seed=(other[2], other[3])) == (ok, st, left, right)


def test_several_keys_equal_the_oracle_accumulator(shplonk):
    s, P, I = shplonk
    t2 = circuits.setup_vector_mul(8, 4)
    try:
        Q, J = circuits.prove_vector_mul_batch(t2, 8, seed=5, threads=8)
        items = []
        for i in range(8):
            items += [(s, P[i], I[i]), (t2, Q[i], J[i])]
        items[6] = items[4]                                   # a duplicated pair of one key: with draws r - 1 it cancels
        for draws in (br.pattern_draws("random", 16, 9), br.pattern_draws("alternating", 16), br.pattern_draws("zero_at", 16, 3, k=7),
                      br.pattern_draws("programmed", 16, 1)):
            assert br.expected(items, draws) == circuits.oracle_accumulate(items, draws)
    finally:
        t2.free()
