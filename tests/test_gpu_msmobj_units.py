"""The two kernels of the resident MSM object alone (halo2_verifier_amd/csrc/util.hip: k_msm_scale, k_affine_to_bytes), through
tests/cpp/msmobj_units.hip and their launchers, against Python integers.

  - scale: words <- words * f mod r, in place, exactly; n = 1, 255, 256, 257 (one below, at and one above the 256-thread workgroup) and
    1000 (several workgroups with a ragged last one); scalars 0, 1, 2, r - 1, r - 2, 2^253 and random ones; factors 0, 1, 2, r - 1 and
    random ones; the terms past n come back unchanged, and the guard bands around the buffer untouched (the harness ends with status 5).
  - to_bytes: affine Montgomery points -> canonical x | y, the identity as 64 zero bytes: the identity, the generator, SRS points, points
    with x or y just below p (the kernel does not ask for the curve); what lies past n keeps its preset.

The command line of the program (no GPU needed): the two checks tests/test_units_usage.py makes for the other harnesses."""
import random

import pytest

import units_harness as uh
from srs_util import P, R_MOD, g1_xy

PROG = "msmobj_units"
MODES = ["scale", "to_bytes"]
SIZES = [1, 255, 256, 257, 1000]
SLACK = 3
EDGE_SCALARS = [0, 1, 2, R_MOD - 1, R_MOD - 2, 1 << 253]


def le32(v):
    return v.to_bytes(32, "little")


def test_usage_names_every_mode():
    r = uh.start(PROG, [])
    assert r.returncode == 2, (r.returncode, r.stderr)
    usage = [l for l in r.stderr.splitlines() if l.startswith("usage: " + PROG)]
    assert len(usage) == 1, r.stderr
    assert set(MODES) <= set(usage[0].replace("|", " ").split()), usage[0]
    r = uh.start(PROG, ["no_such_mode", "a", "b"])
    assert r.returncode == 2 and "usage: " + PROG in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("mode", MODES)
def test_empty_input_is_too_short(mode, tmp_path):
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    out = tmp_path / "out.bin"
    r = uh.start(PROG, [mode, empty, out])
    assert r.returncode == 2 and "input too short" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()


@pytest.mark.gpu
def test_scale_is_exact(tmp_path):
    rnd = random.Random(2401)
    factors = [0, 1, 2, R_MOD - 1] + [rnd.randrange(R_MOD) for _ in range(2)]
    jobs = []
    for n in SIZES:
        for f in factors:
            scalars = [rnd.randrange(R_MOD) for _ in range(n + SLACK)]
            for i, e in enumerate(EDGE_SCALARS):   # at the front, and again at the ragged end of the last workgroup
                if i < n:
                    scalars[i] = e
                if n - 1 - i >= len(EDGE_SCALARS):
                    scalars[n - 1 - i] = e
            jobs.append((n, f, scalars))
    blob = uh.words([len(jobs)])
    for n, f, scalars in jobs:
        blob += uh.words([n, SLACK]) + le32(f) + b"".join(le32(s) for s in scalars)
    out = uh.Cursor(uh.run(PROG, ["scale"], blob, tmp_path))
    for n, f, scalars in jobs:
        got = [out.num() for _ in range(n + SLACK)]
        assert got[:n] == [s * f % R_MOD for s in scalars[:n]], (n, f)
        assert got[n:] == scalars[n:], (n, f, "terms past n were touched")
    out.done()


@pytest.mark.gpu
def test_to_bytes_is_exact(tmp_path, srs):
    rnd = random.Random(2402)
    special = [bytes(64), g1_xy((1, 2)), le32(P - 1) + le32(P - 2), le32(5) + le32(P - 1), le32(P - 1) + le32(7), le32(0) + le32(1), le32(1) + le32(0)]
    pts = [g1_xy(p) for p in srs.g]
    jobs = []
    for n in SIZES:
        points = [pts[rnd.randrange(len(pts))] for _ in range(n)]
        for i, sp in enumerate(special):
            if i < n:
                points[i] = sp
            if n - 1 - i >= len(special):
                points[n - 1 - i] = sp
        jobs.append((n, points))
    blob = uh.words([len(jobs)])
    for n, points in jobs:
        blob += uh.words([n, SLACK]) + b"".join(points)
    out = uh.Cursor(uh.run(PROG, ["to_bytes"], blob, tmp_path))
    for n, points in jobs:
        got = [out.take(64) for _ in range(n + SLACK)]
        assert got[:n] == points, n
        assert got[n:] == [b"\xff" * 64] * SLACK, (n, "bytes past n were written")
    out.done()
