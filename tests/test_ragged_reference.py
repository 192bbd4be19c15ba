"""tests/ragged_reference.py against itself and against the definition tests/test_gpu_multipliers.py uses for equal groups.  No GPU."""
import random

import pytest

import ragged_reference as rr
from ragged_reference import R


def _equal_groups_definition(draws, n):
    """test_gpu_multipliers._expected, word for word: one group's tail -> the multipliers of its first n proofs"""
    out, run = [0] * len(draws), 1
    for j in range(len(draws) - 1, -1, -1):
        out[j] = run
        run = run * draws[j] % R
    return out[:n]


@pytest.mark.parametrize("G,n", [(1, 1), (1, 65), (4, 63), (32, 64), (3, 1024)])
def test_equal_sizes_are_the_equal_groups_definition(G, n):
    rnd = random.Random(G * 10007 + n)
    draws = [rnd.randrange(R) for _ in range(G * n)]
    want = [v for g in range(G) for v in _equal_groups_definition(draws[g * n:(g + 1) * n], n)]
    assert rr.multipliers([n] * G, draws) == want
    assert rr.multipliers_scan([n] * G, draws) == want


SIZE_LISTS = [[1], [1, 1, 1], [255, 1], [256, 256], [257, 1, 254], [1] * 300, [3, 700, 1, 1, 2049, 5], rr.tile_edge_sizes()]


@pytest.mark.parametrize("sizes", SIZE_LISTS, ids=lambda s: f"{len(s)}x{max(s)}")
def test_the_scan_is_the_definition(sizes):
    rnd = random.Random(sum(sizes) * 31 + len(sizes))
    draws = [rnd.randrange(1, R) for _ in range(sum(sizes))]
    assert rr.multipliers_scan(sizes, draws) == rr.multipliers(sizes, draws)


def test_the_scan_in_small_tiles_and_chunks():
    """every path of the scheme at a size Python walks quickly: groups over several tiles and several chunks of the scan over tiles"""
    rnd = random.Random(5)
    for sizes in ([1, 40, 2, 2, 100, 1], [150], [7] * 20 + [1] * 9, [1] * 16 + [64, 3]):
        draws = [rnd.randrange(1, R) for _ in range(sum(sizes))]
        assert rr.multipliers_scan(sizes, draws, tile=4, chunk=8) == rr.multipliers(sizes, draws)


def test_a_zero_draw_stays_inside_its_group():
    sizes = [3, 700, 5]
    rnd = random.Random(6)
    draws = [rnd.randrange(1, R) for _ in range(sum(sizes))]
    draws[3 + 300] = 0
    m = rr.multipliers_scan(sizes, draws)
    assert m == rr.multipliers(sizes, draws)
    assert all(v == 0 for v in m[3:303]) and all(v != 0 for v in m[:3] + m[303:])


def test_tile_edge_sizes_cover_every_edge():
    sizes = rr.tile_edge_sizes()
    ends = set(rr.offsets(sizes)[1:])
    assert sum(sizes) == 1024 and all(s >= 1 for s in sizes)
    assert all({e - 1, e, e + 1} <= ends for e in (256, 512, 768))


def test_last_flags():
    assert rr.last_flags([2, 1, 3]) == [0, 1, 1, 0, 0, 1]
