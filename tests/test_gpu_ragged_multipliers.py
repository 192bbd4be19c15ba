"""The multipliers of groups of unequal size (csrc/verify_kernels.hip: the segmented suffix scan k_seg_mult_tiles / k_seg_mult_scan_tiles /
k_seg_mult_apply behind multipliers_enqueue) against Python big integers (tests/ragged_reference.py), exactly, as canonical
residues.  build/verify_units ragged (tests/cpp/verify_units.hip, built by csrc/Makefile with the library's flags) runs the library's own enqueue
function on raw draws chosen here; it presets the outputs and checks the guard bands around them and around the per-tile scratch."""
import random
import struct

import pytest

import ragged_reference as rr
import units_harness as uh
from ragged_reference import R

pytestmark = pytest.mark.gpu


# the scan over tile products walks chunks of 1024 tiles (262 144 draws), last chunk first: the second group lies in all three chunks of this list
CHUNKED = [3, 270000, 1, 262144 + 517, 2]
SIZE_LISTS = [[1], [1, 1, 1], [255, 1], [256, 256], [257, 1, 254], [1] * 300, [3, 700, 1, 1, 2049, 5], rr.tile_edge_sizes()]


def _run(jobs, tmp_path):
    """jobs: [(sizes, draws)] -> per job the multipliers"""
    blob = [struct.pack("<I", len(jobs))]
    for sizes, draws in jobs:
        assert len(draws) == sum(sizes)
        blob.append(struct.pack(f"<I{len(sizes)}I", len(sizes), *sizes))
        blob.append(b"".join(d.to_bytes(32, "little") for d in draws))
    raw = uh.run("verify_units", ["ragged"], b"".join(blob), tmp_path, timeout=120)
    out, at = [], 0
    for sizes, _ in jobs:
        n = sum(sizes)
        out.append([int.from_bytes(raw[at + 32 * p:at + 32 * p + 32], "little") for p in range(n)])
        at += 32 * n
    assert at == len(raw)
    return out


def _check(jobs, got):
    for (sizes, draws), m in zip(jobs, got):
        want = rr.multipliers(sizes, draws)
        bad = [p for p in range(len(want)) if m[p] != want[p]]
        assert not bad, f"{len(sizes)} groups, {len(draws)} draws: {len(bad)} multipliers differ, first at proof {bad[0]}: {m[bad[0]]:#x} != {want[bad[0]]:#x}"


def test_ragged_multipliers_match_big_integers(tmp_path):
    rnd = random.Random(700)
    jobs = [(sizes, [rnd.randrange(1, R) for _ in range(sum(sizes))]) for sizes in SIZE_LISTS]
    _check(jobs, _run(jobs, tmp_path))


def test_a_group_over_several_chunks_of_the_tile_scan(tmp_path):
    rnd = random.Random(701)
    jobs = [(CHUNKED, [rnd.randrange(1, R) for _ in range(sum(CHUNKED))])]
    _check(jobs, _run(jobs, tmp_path))


def test_zero_draw_zeroes_the_earlier_multipliers_of_its_group_only(tmp_path):
    rnd = random.Random(702)
    jobs, where = [], []
    for sizes, g0, k in [([3, 700, 1, 1, 2049, 5], 4, 1000), ([3, 700, 1, 1, 2049, 5], 1, 699), ([257, 1, 254], 0, 256), ([1] * 300, 17, 0), ([256, 256], 1, 1)]:
        draws = [rnd.randrange(1, R) for _ in range(sum(sizes))]
        first = rr.offsets(sizes)[g0]
        draws[first + k] = 0
        jobs.append((sizes, draws)); where.append((first, k, sizes[g0]))
    got = _run(jobs, tmp_path)
    _check(jobs, got)
    for (first, k, size), m in zip(where, got):
        assert all(v == 0 for v in m[first:first + k]) and all(v != 0 for v in m[:first] + m[first + k:])
