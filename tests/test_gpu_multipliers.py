"""The batch multipliers of equal groups (csrc/verify_kernels.hip: the segmented suffix scan k_seg_mult_tiles / k_seg_mult_scan_tiles /
k_seg_mult_apply behind multipliers_enqueue) against Python big integers: mult[g][p] = the product of the draws of the LATER proofs of
p's own group, mod r (kzg/strategy.rs:129, msm.rs:173-176).  build/verify_units multipliers (tests/cpp/verify_units.hip, built by
csrc/Makefile with the library's flags) runs the library's own kernels on raw draws chosen here: n = 1, 2, 63, 64, 65, 1024 and 8192
proofs per group in 1, 4 and 32 groups, with a zero draw inside a group (it zeroes the multipliers of the group's earlier proofs and
of no other group: the proofs h2v_batch_recheck refuses ranges over), and a shard's form (more draws than proofs: the tail of the
whole batch).  The values are compared exactly, as canonical residues."""
import random
import struct

import pytest

import units_harness as uh

pytestmark = pytest.mark.gpu

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
SIZES = [1, 2, 63, 64, 65, 1024, 8192]
GROUPS = [1, 4, 32]


def _expected(draws, n):
    """draws: one group's tail -> the multipliers of its first n proofs"""
    out, run = [0] * len(draws), 1
    for j in range(len(draws) - 1, -1, -1):
        out[j] = run
        run = run * draws[j] % R
    return out[:n]


def _run(jobs, tmp_path):
    """jobs: [(groups, n_tail, n, draws[groups][n_tail])] -> per job the multipliers [groups][n]"""
    blob = [struct.pack("<I", len(jobs))]
    for G, nt, n, draws in jobs:
        blob.append(struct.pack("<III", G, nt, n))
        blob.append(b"".join(d.to_bytes(32, "little") for grp in draws for d in grp))
    raw = uh.run("verify_units", ["multipliers"], b"".join(blob), tmp_path, timeout=600)
    out, at = [], 0
    for G, nt, n, _ in jobs:
        out.append([[int.from_bytes(raw[at + 32 * (g * n + p):at + 32 * (g * n + p) + 32], "little") for p in range(n)] for g in range(G)])
        at += 32 * G * n
    assert at == len(raw)
    return out


def _check(jobs, got):
    for (G, nt, n, draws), m in zip(jobs, got):
        for g in range(G):
            want = _expected(draws[g], n)
            bad = [p for p in range(n) if m[g][p] != want[p]]
            assert not bad, f"G={G} n_tail={nt} n={n} group {g}: {len(bad)} multipliers differ, first at proof {bad[0]}: {m[g][bad[0]]:#x} != {want[bad[0]]:#x}"


@pytest.mark.parametrize("G", GROUPS)
def test_multipliers_match_big_integers(G, tmp_path):
    rnd = random.Random(100 + G)
    jobs = [(G, n, n, [[rnd.randrange(1, R) for _ in range(n)] for _ in range(G)]) for n in SIZES]
    _check(jobs, _run(jobs, tmp_path))


@pytest.mark.parametrize("G", GROUPS)
def test_zero_draw_zeroes_the_earlier_multipliers_of_its_group_only(G, tmp_path):
    rnd = random.Random(200 + G)
    jobs = []
    for n in SIZES:
        draws = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(G)]
        g0 = G // 2
        z = n // 2 if n < 1024 else 3 * 256 + 17      # (inside a tile that is neither the first nor the last)
        draws[g0][z] = 0
        jobs.append((G, n, n, draws))
    got = _run(jobs, tmp_path)
    _check(jobs, got)
    for (G_, nt, n, draws), m in zip(jobs, got):
        g0 = G_ // 2
        z = draws[g0].index(0)
        assert all(v == 0 for v in m[g0][:z]) and all(v != 0 for v in m[g0][z:])
        assert all(v != 0 for g in range(G_) if g != g0 for v in m[g])


def test_a_shard_uploads_the_tail_of_the_whole_batch(tmp_path):
    """more draws than proofs (distributed.tail_for_shard): the later shards' draws count, and their proofs get no multiplier here"""
    rnd = random.Random(300)
    jobs = []
    for G, n, nt in [(1, 1, 9), (1, 64, 65), (4, 63, 1024), (4, 256, 257), (2, 1024, 8192), (32, 65, 130)]:
        jobs.append((G, nt, n, [[rnd.randrange(R) for _ in range(nt)] for _ in range(G)]))
    _check(jobs, _run(jobs, tmp_path))


def test_groups_against_the_tile_boundaries(tmp_path):
    """equal groups are segments of one scan over the whole draw array, in tiles of 256 draws: a group whose draws past its proofs
    straddle a tile's end (gs = 255, nt = 257, G = 3), and groups that end exactly on a tile's end (gs = nt = 256, G = 2)"""
    rnd = random.Random(350)
    jobs = [(G, nt, n, [[rnd.randrange(1, R) for _ in range(nt)] for _ in range(G)]) for G, n, nt in [(3, 255, 257), (2, 256, 256)]]
    _check(jobs, _run(jobs, tmp_path))


def test_gather_multipliers(tmp_path):
    """k_gather_multipliers behind gather_multipliers_enqueue: out[i] = src[idx[i]], the nine limbs as they lie in memory, with repeated,
    reversed and out-of-order indices at n = 1, 255, 256, 257 and 512 (one and two workgroups, a partial last one); n = 0 launches
    nothing.  The harness checks every index against the source length before the launch and the guard bands around the output after."""
    import numpy as np
    rnd = random.Random(400)
    jobs = []
    for n_src, n, kind in [(1, 1, "repeat"), (300, 255, "reverse"), (300, 256, "shuffle"), (300, 257, "repeat"), (257, 257, "reverse"), (7, 512, "shuffle"),
                           (256, 256, "identity"), (5, 0, "identity")]:
        src = np.array([[rnd.randrange(1 << 29) for _ in range(9)] for _ in range(n_src)], dtype="<u4").reshape(n_src, 9)
        if kind == "repeat": idx = [(i // 3) % n_src for i in range(n)]
        elif kind == "reverse": idx = [n_src - 1 - i % n_src for i in range(n)]
        elif kind == "shuffle": idx = [rnd.randrange(n_src) for _ in range(n)]
        else: idx = list(range(n))
        assert all(0 <= i < n_src for i in idx)
        jobs.append((src, idx))
    blob = struct.pack("<I", len(jobs)) + b"".join(struct.pack("<II", len(src), len(idx)) + src.tobytes() + np.asarray(idx, dtype="<u4").tobytes() for src, idx in jobs)
    out = uh.as_words(uh.run("verify_units", ["gather"], blob, tmp_path, timeout=120))
    at = 0
    for src, idx in jobs:
        got = out[at:at + 9 * len(idx)].reshape(len(idx), 9); at += got.size
        assert (got == src[idx]).all() if idx else got.size == 0, (len(src), len(idx))
    assert at == len(out)
