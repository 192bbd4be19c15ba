"""tests/ingest_reference.py against direct definitions (no GPU): zero_below[g] counts the proofs of group g whose multiplier — the
product of the group's draws behind the proof — is zero, and those proofs are the group's first ones; the packed rows are the rows."""
import random

import ingest_reference as ir

R = ir.R


def _direct(draws, n, groups=1, sizes=None):
    if sizes is not None:
        off = ir.offsets(sizes)
        spans = [(off[g], sizes[g], sizes[g]) for g in range(len(sizes))]
    else:
        gs, nt = n // groups, len(draws) // groups
        spans = [(g * nt, gs, nt) for g in range(groups)]
    out = []
    for first, gs, nt in spans:
        zero = []
        for p in range(gs):
            m = 1
            for d in draws[first + p + 1:first + nt]:
                m = m * d % R
            zero.append(m == 0)
        k = sum(zero)
        assert zero == [True] * k + [False] * (gs - k)   # a prefix
        out.append(k)
    return out


def test_zero_below_is_the_count_of_zero_multipliers():
    rnd = random.Random(5)
    draw = lambda: rnd.choice([0, 0, 1, R - 1, rnd.randrange(R)])
    for _ in range(300):
        groups = rnd.choice([1, 2, 4, 5])
        gs = rnd.randrange(1, 7)
        nt = gs * rnd.choice([1, 1, 2, 3])
        draws = [draw() for _ in range(groups * nt)]
        assert ir.zero_below(draws, groups * gs, groups) == _direct(draws, groups * gs, groups)
        sizes = [rnd.randrange(1, 6) for _ in range(groups)]
        draws = [draw() for _ in range(sum(sizes))]
        assert ir.zero_below(draws, sum(sizes), sizes=sizes) == _direct(draws, sum(sizes), sizes=sizes)


def test_zero_below_by_hand():
    assert ir.zero_below([0, 5, 5, 5], 4) == [0]                    # a zero at a group's first index zeroes nobody
    assert ir.zero_below([5, 5, 5, 0], 4) == [3]
    assert ir.zero_below([5, 0, 5, 5, 5, 5, 0, 5], 8, 2) == [1, 2]
    assert ir.zero_below([5, 5, 5, 0], 2) == [2]                    # a shard: the zero lies behind both proofs
    assert ir.zero_below([5, 5, 0, 5, 5, 5, 5, 5], 4, 2) == [2, 0]  # two groups of two proofs and four draws
    assert ir.zero_below([5, 0, 0, 5, 5], 5, sizes=[2, 1, 2]) == [1, 0, 0]
    assert ir.zero_below([], 0, 3) == [0, 0, 0]


def test_stored_draws_and_the_fault_word():
    draws = [0, 1, R - 1, R, R + 1, (1 << 256) - 1, 7]
    stored, fault, zb = ir.ingest_draws(draws, 7)
    assert stored == [0, 1, R - 1, 1, 1, 1, 7] and fault == 3 and zb == [0]
    assert ir.ingest_draws([3, 0, R - 1], 3)[1:] == (ir.NO_FAULT, [1])


def test_pack_rows():
    src = bytes(range(48)) + b"\xee" * 16 + bytes(range(100, 148)) + b"\xee" * 16
    assert ir.pack_rows(src, 2, 48, 64) == bytes(range(48)) + bytes(range(100, 148))
    assert ir.pack_rows(src[:112], 2, 48, 64) == bytes(range(48)) + bytes(range(100, 148))   # (the last row needs no padding)
    assert ir.pack_rows(b"", 0, 32, 32) == b""
