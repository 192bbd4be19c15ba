"""The definition of h2v_accumulator_process_batch in Python integers (tests/legs_reference.py), checked against what it must equal:
`process` once per group, and ONE accumulation over all proofs with all draws concatenated — on random scalars in place of points, and
once on G1 points.  No GPU."""
import random

import legs_reference as lr
import msm_reference as ref
from msm_reference import R

CASES = [[6] * 4, [1, 7, 2, 14], [24], [1] * 24, [1] * 65, [3, 1, 1, 9, 2], [1] * 512]


def _case(sizes, seed, zero_at=()):
    rnd = random.Random(seed)
    n = sum(sizes)
    draws = [rnd.randrange(1, R) for _ in range(n)]
    for i in zero_at:
        draws[i] = 0
    guards = [rnd.randrange(R) for _ in range(n)]
    return draws, guards, rnd.randrange(R)


def _check(sizes, draws, guards, acc):
    got, entries = lr.process_batch(acc, draws, guards, sizes)
    # one accumulation over the concatenation
    assert got == lr.process(acc, draws, guards)
    # process once per group, and the entries such calls leave
    off = lr.offsets(sizes)
    step = acc
    for g in range(len(sizes)):
        sl = slice(off[g], off[g + 1])
        step = lr.process(step, draws[sl], guards[sl])
        M = 1
        for r in draws[sl]:
            M = M * r % R
        assert entries[g] == (lr.process(0, draws[sl], guards[sl]), M)
    assert got == step
    # the journal's invariant, with the accumulator as the base entry
    assert lr.from_entries([(acc, 1)] + entries) == got


def test_legs_equal_one_accumulation():
    for k, sizes in enumerate(CASES):
        draws, guards, acc = _case(sizes, 100 + k)
        _check(sizes, draws, guards, acc)
        _check(sizes, draws, guards, 0)          # an empty accumulator


def test_zero_and_unit_draws():
    sizes = [3, 3, 3]
    for at in range(9):                          # a zero as first, middle and last draw of the first, the middle and the last group
        draws, guards, acc = _case(sizes, 200 + at, zero_at=(at,))
        _check(sizes, draws, guards, acc)
        got, entries = lr.process_batch(acc, draws, guards, sizes)
        assert entries[at // 3][1] == 0
        # everything before the proof with the zero draw drops out, the accumulator included
        assert got == lr.process(0, draws[at:], guards[at:]) == lr.process(12345, draws[at:], guards[at:])
    draws, guards, acc = _case([1, 1], 300)
    draws, guards = [draws[0], R - 1], [guards[0]] * 2     # 1 and r - 1 against the same Guard on an empty accumulator: the sums cancel
    assert lr.process_batch(0, draws, guards, [1, 1])[0] == 0
    _check([1, 1], draws, guards, acc)
    _check([2, 1, 2], [1, 1, 1, 1, 1], [5, 6, 7, 8, 9], 11)


def test_weights():
    assert lr.leg_weights([]) == (1, [])
    assert lr.leg_weights([7]) == (7, [1])
    assert lr.leg_weights([2, 3, 5]) == (30, [15, 5, 1])
    assert lr.leg_weights([2, 0, 5]) == (0, [0, 5, 1])
    assert lr.group_multipliers([2, 3, 5, 7, 11], [2, 3]) == [3, 1, 77, 11, 1]
    assert lr.leg_products([2, 5], [3, 77]) == [6, 385]


def test_on_g1_points():
    rnd = random.Random(5)
    grp = (ref.add, ref.mul, None)
    sizes = [2, 1, 3]
    draws = [rnd.randrange(1, R) for _ in range(6)]
    guards = [ref.mul(rnd.randrange(1, R), ref.G) for _ in range(6)]
    acc = ref.mul(rnd.randrange(1, R), ref.G)
    got, entries = lr.process_batch(acc, draws, guards, sizes, grp)
    assert got == lr.process(acc, draws, guards, grp) and ref.on_curve(got)
    assert lr.from_entries([(acc, 1)] + entries, grp) == got
    # the fold: the sum of the scaled records replaces the accumulator; the slots take the unscaled pairs
    total, W = lr.leg_weights([m for _, m in entries])
    records = [(ref.mul(total, acc), None)] + [(ref.mul(w, s), None) for w, (s, _) in zip(W, entries)]
    pairs = [(s, None) for s, _ in entries]
    out, written = lr.legs_fold(records, pairs, [4, 0, 2])
    assert out == (got, None) and written == {4: pairs[0], 0: pairs[1], 2: pairs[2]}
