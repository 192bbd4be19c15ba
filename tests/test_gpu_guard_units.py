"""k_guard_terms alone (halo2_verifier_amd/csrc/util.hip), through its launcher, in tests/cpp/guard_units.hip: the conversion of a
call's Guard terms — scalar bytes to the MSM's words, times the guard's multiplier; base bytes to affine points; one validity word —
against Python big integers.  Term counts 1, 255, 256, 257 and 1000 (the workgroup is 256 lanes); every output lies between guard
bands preset apart from the outputs."""
import random
import struct

import pytest

import msm_reference as ref
import record_reference as rr
import units_harness as uh

R, P = ref.R, ref.P
NONE = 0xffffffff
SIZES = (1, 255, 256, 257, 1000)


def _run(blob, tmp_path):
    return uh.as_words(uh.run("guard_units", ["terms"], blob, tmp_path))


def _job(scalars, bases, gidx=None, mult=None):
    """scalars: integers below 2^256; bases: 64-byte strings; gidx / mult: the guard of every term and the guards' multipliers"""
    n = len(scalars)
    b = struct.pack("<III", n, 1 if mult is not None else 0, len(mult) if mult is not None else 0)
    b += b"".join(int(s).to_bytes(32, "little") for s in scalars) + b"".join(bases)
    if mult is not None:
        b += uh.words(gidx) + b"".join(int(m).to_bytes(32, "little") for m in mult)
    return b


def _split(out, jobs):
    res, at = [], 0
    for n in jobs:
        sc = out[at:at + 8 * n].reshape(n, 8); at += 8 * n
        pts = out[at:at + 18 * n].reshape(n, 18); at += 18 * n
        res.append((sc, pts, int(out[at]))); at += 1
    assert at == len(out)
    return res


def _xy(pt):
    return rr.point_to_bytes(pt)[0]


def _words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


@pytest.mark.gpu
def test_products_exact(tmp_path):
    """s * mult[guard] at 0, 1, r - 1 on either side and both, and random values; the guards' boundaries never line up with 256"""
    rnd = random.Random(11)
    edge = [0, 1, R - 1]
    jobs = []
    for n in SIZES:
        n_guards = max(1, n // 3)
        mult = [edge[g % 3] if g < 6 else rnd.randrange(R) for g in range(n_guards)]
        gidx = sorted(rnd.randrange(n_guards) for _ in range(n))
        gidx[:9] = [0, 0, 0, 1 % n_guards, 1 % n_guards, 1 % n_guards, 2 % n_guards, 2 % n_guards, 2 % n_guards][:n]
        scalars = [edge[i % 3] if i < 9 else rnd.randrange(R) for i in range(n)]
        jobs.append((scalars, [_xy(ref.G)] * n, gidx[:n], mult))
    res = _split(_run(struct.pack("<I", len(jobs)) + b"".join(_job(*j) for j in jobs), tmp_path), [len(j[0]) for j in jobs])
    for (scalars, _, gidx, mult), (sc, pts, word) in zip(jobs, res):
        assert word == NONE
        for i, s in enumerate(scalars):
            assert sc[i].tolist() == _words(s * mult[gidx[i]] % R), i
        assert all((ref.fq_value(w[:9]), ref.fq_value(w[9:])) == ref.G and rr.in_range(w, 2) for w in pts.tolist())
    if len(jobs[-1][0]) >= 9:
        assert {(jobs[-1][0][i], jobs[-1][3][jobs[-1][2][i]]) for i in range(9)} == {(a, b) for a in edge for b in edge}


@pytest.mark.gpu
def test_null_multipliers_pass_the_scalar_through(tmp_path):
    rnd = random.Random(12)
    jobs = [([0, 1, R - 1][:n] + [rnd.randrange(R) for _ in range(max(0, n - 3))], [_xy(ref.mul(i + 1, ref.G)) for i in range(n)]) for n in SIZES[:4]]
    res = _split(_run(struct.pack("<I", len(jobs)) + b"".join(_job(*j) for j in jobs), tmp_path), [len(j[0]) for j in jobs])
    for (scalars, _), (sc, pts, word) in zip(jobs, res):
        assert word == NONE
        assert [w.tolist() for w in sc] == [_words(s) for s in scalars]
        for i, w in enumerate(pts.tolist()):
            assert (ref.fq_value(w[:9]), ref.fq_value(w[9:])) == ref.mul(i + 1, ref.G) and rr.in_range(w, 2)


def _bad_bases():
    x, y = ref.mul(5, ref.G)
    le = lambda v: int(v).to_bytes(32, "little")
    return [le(P) + le(y), le(x) + le(P), le(x + P) + le(y), le(x) + le(y + 1), le(x) + le(0), le(0) + le(y), le(1) + le(3)]


@pytest.mark.gpu
def test_bases_and_the_validity_word(tmp_path):
    """the identity, canonical points, x = p, points off the curve, scalars from r on: a bad term is a zero scalar under the identity,
    and the word is the lowest bad index, also when several terms are bad in different workgroups"""
    rnd = random.Random(13)
    good = [_xy(ref.mul(k, ref.G)) for k in (1, 2, 7)] + [_xy(ref.neg(ref.G)), bytes(64)]
    bad = _bad_bases()
    n = 1000
    plans = [{}, {999: ("b", 0)}, {0: ("s", R)}, {700: ("b", 3), 300: ("s", R + 1), 999: ("b", 1)}, {513: ("b", 6), 514: ("s", (1 << 256) - 1)},
             {256 + i: ("b", i) for i in range(len(bad))}]
    jobs = []
    for plan in plans:
        scalars = [rnd.randrange(1, R) for _ in range(n)]
        bases = [good[i % len(good)] for i in range(n)]
        for i, (kind, v) in plan.items():
            if kind == "s":
                scalars[i] = v
            else:
                bases[i] = bad[v]
        n_guards = 77
        jobs.append((scalars, bases, [i * n_guards // n for i in range(n)], [rnd.randrange(1, R) for _ in range(n_guards)], plan))
    jobs.append(([R], [good[0]], None, None, {0: ("s", R)}))          # n = 1, bad, no multipliers
    jobs.append(([5], [bad[3]], [0], [1], {0: ("b", 3)}))
    res = _split(_run(struct.pack("<I", len(jobs)) + b"".join(_job(*j[:4]) for j in jobs), tmp_path), [len(j[0]) for j in jobs])
    for (scalars, bases, gidx, mult, plan), (sc, pts, word) in zip(jobs, res):
        assert word == (min(plan) if plan else NONE), sorted(plan)
        for i, s in enumerate(scalars):
            pt, flag = rr.point_from_bytes(bases[i])
            if i in plan:
                assert flag == 1 or s >= R
                assert sc[i].tolist() == [0] * 8 and pts[i].tolist() == [0] * 18, i
                continue
            assert flag == 0
            assert sc[i].tolist() == _words(s * (mult[gidx[i]] if mult else 1) % R), i
            w = pts[i].tolist()
            if pt is None:
                assert w == [0] * 18
            else:
                assert (ref.fq_value(w[:9]), ref.fq_value(w[9:])) == pt and rr.in_range(w, 2), i


# ---- the command line (no GPU: both end before any HIP call)
def test_usage_and_empty_input(tmp_path):
    r = uh.start("guard_units", [])
    assert r.returncode == 2 and "usage: guard_units terms IN OUT" in r.stderr, (r.returncode, r.stderr)
    r = uh.start("guard_units", ["no_such_mode", "a", "b"])
    assert r.returncode == 2 and "usage: guard_units" in r.stderr
    empty, out = tmp_path / "empty.bin", tmp_path / "out.bin"
    empty.write_bytes(b"")
    r = uh.start("guard_units", ["terms", empty, out])
    assert r.returncode == 2 and "input too short" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()
