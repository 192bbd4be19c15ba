"""The definition of a batch's Guards (tests/guards_out_reference.py) is the right one: per group, the MSM over the expected left and
right terms is the accumulator the oracle's AccumulatorStrategy reports for that group (circuits.oracle_verify_batch), for SHPLONK and
GWC on the toy VK and for a wide VK with lookups and a shuffle, with failing proofs (zero rows) and a zero draw; with unit draws the
SHPLONK rows are the oracle's own Guard lists, element for element; and the GWC merge keeps every base's sum.  No GPU."""
import random

import pytest

import circuits
import guards_out_reference as gr
import oracle_lib
from circuits import R_MOD

ZERO = gr.ZERO


def _msm(s, scalars, bases):
    terms = [(sc, b) for sc, b in zip(scalars, bases) if sc % R_MOD and b != ZERO]
    if not terms:
        return ZERO
    return oracle_lib.g1_msm(s.L, [sc for sc, _ in terms], [b for _, b in terms])


def _check_groups(s, P, I, rand, sizes):
    exp = gr.expected(s, P, I, rand, sizes)
    assert len(exp) == len(P)
    lo = 0
    for sz in sizes:
        rows = exp[lo:lo + sz]
        left = _msm(s, [x for r in rows for x in r["left_scalars"]], [b for r in rows for b in r["left_bases"]])
        right = _msm(s, [x for r in rows for x in r["right_scalars"]], [b for r in rows for b in r["right_bases"]])
        ok, st, eleft, eright = circuits.oracle_verify_batch(s, P[lo:lo + sz], I[lo:lo + sz], rand[lo:lo + sz])
        assert [r["status"] for r in rows] == st
        assert (left, right) == (eleft, eright), (sizes, lo)
        lo += sz
    return exp


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _spoil(P, at):
    P = list(P)
    b = bytearray(P[at]); b[32:64] = b"\xff" * 32; P[at] = bytes(b)   # an undecodable point: a status, no Guard
    return P


@pytest.mark.parametrize("multiopen", [circuits.SHPLONK, circuits.GWC])
def test_group_sums_are_the_oracles_accumulators(multiopen):
    s = circuits.setup_vector_mul(8, 8).set_options(multiopen, circuits.BLAKE2B)
    try:
        P, I = circuits.prove_vector_mul_batch(s, 8, seed=61 + multiopen, threads=8)
        rand = _draws(8, 5)
        _check_groups(s, P, I, rand, [8])
        _check_groups(s, P, I, rand, [4, 4])
        zero = list(rand); zero[3] = 0                      # a zero draw in the middle group: the proofs before it have zero scalars
        exp = _check_groups(s, P, I, zero, [1, 5, 2])
        assert [r["mult"] for r in exp[1:3]] == [0, 0] and all(x == 0 for r in exp[1:3] for x in r["right_scalars"]) and exp[3]["mult"] != 0
        assert exp[1]["right_bases"] != [ZERO] * len(exp[1]["right_bases"])      # under their own bases
        bad = _spoil(P, 2)
        exp = _check_groups(s, bad, I, rand, [4, 4])
        assert exp[2]["status"] != 0 and set(exp[2]["right_bases"]) == {ZERO} and set(exp[2]["left_bases"]) == {ZERO}
        assert not any(exp[2]["right_scalars"]) and not any(exp[2]["left_scalars"])
        assert len(exp[2]["right_scalars"]) == len(exp[0]["right_scalars"]) and len(exp[2]["left_scalars"]) == len(exp[0]["left_scalars"])
    finally:
        s.free()


def test_wide_vk_with_lookups_and_shuffle():
    s = circuits.setup_wide(8)
    try:
        proofs = [circuits.prove_wide(s, witness_seed=3 + i, rng_seed=13 + i) for i in range(3)]
        P, I = [p for p, _ in proofs], [i for _, i in proofs]
        _check_groups(s, P, I, _draws(3, 9), [3])
        _check_groups(s, P, I, _draws(3, 10), [1, 2])
    finally:
        s.free()


def test_unit_draws_give_the_raw_shplonk_guard():
    s = circuits.setup_vector_mul(8, 8)
    try:
        P, I = circuits.prove_vector_mul_batch(s, 3, seed=64, threads=4)
        exp = gr.expected(s, P, I, [1, 1, 1], [3])
        for row, p, i in zip(exp, P, I):
            rc, g = circuits.oracle_guard(s, p, i)
            assert rc == 0 and row["mult"] == 1 and row["status"] == 0
            for side in ("left", "right"):
                assert [x.to_bytes(32, "little") for x in row[side + "_scalars"]] == g[side + "_scalars"]
                assert row[side + "_bases"] == g[side + "_bases"]
    finally:
        s.free()


def test_gwc_merge_is_sum_equal_and_first_appearance():
    s = circuits.setup_vector_mul(8, 8).set_options(circuits.GWC, circuits.BLAKE2B)
    try:
        P, I = circuits.prove_vector_mul_batch(s, 1, seed=65, threads=1)
        rc, g = circuits.oracle_guard(s, P[0], I[0])
        assert rc == 0
        sc = [int.from_bytes(x, "little") for x in g["right_scalars"]]
        ms, mb = gr.merge_first_appearance(sc, g["right_bases"])
        assert len(mb) == len(set(mb)) < len(g["right_bases"])           # something was opened at several points
        firsts = []
        for b in g["right_bases"]:
            if b not in firsts:
                firsts.append(b)
        assert mb == firsts
        assert gr.by_base(ms, mb) == gr.by_base(sc, g["right_bases"])
        row = gr.expected(s, P, I, [1], [1])[0]
        assert (row["right_scalars"], row["right_bases"]) == (ms, mb)
    finally:
        s.free()
    assert gr.merge_first_appearance([1, 2, R_MOD - 1, 5], [b"a", b"b", b"a", b"b"]) == ([0, 7], [b"a", b"b"])


def test_the_gather_model():
    """the pure model on a hand-made layout: slot and VK-wide terms, a range with first > 0, a dead proof"""
    n, np_ = 3, 2
    order = [(0, 1), (1, 0), (0, 0)]
    slot = [10, 11, 20, 21, 30, 31]
    shared = [[100, 200, 300]]
    pts = [bytes([i + 1]) * 64 for i in range(n * np_ + 1)]
    status = [0, -30, 0]
    sc, bs = gr.gather(order, slot, shared, pts, status, n, np_, 1, 2)
    assert sc == [0, 0, 0, 31, 300, 30]
    assert bs == [ZERO] * 3 + [pts[5], pts[6], pts[4]]
    assert gr.proofs_model([7, 8, 9], status, 1, 2) == ([8, 9], [-5, 0])
    assert [gr.decode_status(v) for v in (0, -40, -30, -20, -10, -2)] == [0, -1, -5, -7, -4, -2]
    assert gr.group_multipliers([2, 3, 5, 7, 11], [3, 2]) == [15, 5, 1, 11, 1]
