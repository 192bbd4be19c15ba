"""k_results_tiles, k_results_close and k_results_scatter alone (halo2_verifier_amd/csrc/util.hip), the launches of a finish into
device memory, through their launcher in tests/cpp/results_units.hip, exact against tests/results_reference.py.  Every output lies
between guard bands (a write outside an output ends the program with status 5) and is preset to 0xff: an output that was not asked
for, and the index words behind the last failing proof, must come back as they were."""
import random
import struct

import pytest

import results_reference as rr
import units_harness as uh

CODES = [-40, -30, -20, -10, -123456]     # the four rank codes, and a negative word that passes through
ALL = 127
UNTOUCHED = 0xffffffff
RAGGED_5 = [1, 7, 24, 3, 1]


def _sizes_300(seed=5):
    rnd = random.Random(seed)
    return [1 + (rnd.random() < 0.5) for _ in range(300)]


def _words(n, failing, rnd):
    w = [0] * n
    for k, i in enumerate(sorted(failing)):
        w[i] = CODES[k % len(CODES)] if rnd is None else rnd.choice(CODES)
    return w


class Job:
    def __init__(self, words, groups=1, sizes=None, flags=rr.FLAG_PAIRING, fold=None, ok=None, fault=rr.NO_FAULT, cap=None, want=ALL, repeat=1, seed=0):
        self.words, self.sizes, self.flags, self.fault, self.want, self.repeat = words, sizes, flags, fault, want, repeat
        self.G = len(sizes) if sizes is not None else groups
        self.fold = fold if fold is not None else [0] * self.G
        self.ok = ok if ok is not None else [1] * self.G
        self.cap = cap if cap is not None else max(len(words), 1)
        self.bytes = random.Random(1000 + seed).randbytes(128 * self.G)

    def blob(self):
        n = len(self.words)
        b = struct.pack("<8I", n, self.G, 1 if self.sizes is not None else 0, self.flags, self.fault, self.cap, self.want, self.repeat)
        if self.sizes is not None:
            b += uh.words(rr.offsets(n, sizes=self.sizes))
        b += struct.pack("<%di" % n, *self.words) + uh.words(self.fold) + uh.words(self.ok) + self.bytes
        return b

    def check(self, out, case):
        n, G = len(self.words), self.G
        exp = rr.finish(self.words, self.fold, self.ok, self.bytes, self.flags, G, self.sizes, self.fault, self.cap)
        got = {"status": [out.sword() for _ in range(n)], "group_ok": [out.word() for _ in range(G)], "left_xy": out.take(64 * G), "right_xy": out.take(64 * G),
               "group_failed": [out.word() for _ in range(G)], "failed_index": [out.word() for _ in range(self.cap)], "summary": [out.word() for _ in range(8)]}
        scratch = [out.word() for _ in range(G)]
        assert scratch == [0] * G, (case, "the scratch's group words are not zero again")
        exp["failed_index"] = exp["failed_index"] + [UNTOUCHED] * (self.cap - len(exp["failed_index"]))   # (nothing behind the last index)
        for bit, name in enumerate(("status", "group_ok", "left_xy", "right_xy", "group_failed", "failed_index", "summary")):
            if self.want >> bit & 1:
                assert got[name] == exp[name], (case, name)
            elif name in ("left_xy", "right_xy"):
                assert got[name] == b"\xff" * (64 * G), (case, name, "written though not asked for")
            elif name == "status":
                assert got[name] == [-1] * n, (case, name, "written though not asked for")
            else:
                assert got[name] == [UNTOUCHED] * len(got[name]), (case, name, "written though not asked for")


def _run(jobs, tmp_path):
    blob = struct.pack("<I", len(jobs)) + b"".join(j.blob() for j in jobs)
    out = uh.Cursor(uh.run("results_units", ["finish"], blob, tmp_path))
    for k, j in enumerate(jobs):
        j.check(out, (k, len(j.words), j.G, j.flags, j.cap, j.want))
    out.done()


def _patterns(n, off):
    """the failing sets: none; every proof; exactly every group's first and last proof; both sides of every tile boundary; two waves of
    one tile"""
    firsts_lasts = sorted({o for o in off[:-1]} | {o - 1 for o in off[1:]})
    boundary = [i for i in (255, 256, 511, 512) if i < n]
    waves = [i for i in (3, 70, 130, 200, 255) if i < n]
    return [[], list(range(n)), firsts_lasts, boundary, waves]


@pytest.mark.gpu
def test_sizes_groups_and_failure_patterns(tmp_path):
    """n in {1, 255, 256, 257, 1000} as one group; 4 equal groups; sizes [1, 7, 24, 3, 1]; 300 sizes of 1 or 2 — each with every
    failure pattern, the status words being the four rank codes and a word that passes through"""
    rnd = random.Random(31)
    jobs = []
    shapes = [(n, 1, None) for n in (1, 255, 256, 257, 1000)] + [(n, 4, None) for n in (4, 256, 260, 1000)]
    shapes += [(sum(RAGGED_5), 1, RAGGED_5), (sum(_sizes_300()), 1, _sizes_300())]
    for n, groups, sizes in shapes:
        off = rr.offsets(n, groups, sizes)
        for k, failing in enumerate(_patterns(n, off)):
            jobs.append(Job(_words(n, failing, rnd if k % 2 else None), groups, sizes, seed=len(jobs), repeat=1 + k % 2))
    _run(jobs, tmp_path)


@pytest.mark.gpu
def test_more_tiles_than_one_pass_of_the_scan(tmp_path):
    """n = 65 536 + 300: 258 tiles, two passes of the scan with the total carried between them; failing proofs in the first tile, at
    the last tile of the first pass, the first of the second, and the last proof; status words only"""
    n = 65536 + 300
    failing = [0, 1, 255 * 256 + 17, 255 * 256 + 255, 256 * 256, 256 * 256 + 64, 257 * 256 + 1, n - 1]
    jobs = [Job(_words(n, failing, None), 4, None, want=1 | 16 | 32 | 64, cap=16),
            Job(_words(n, range(0, n, 97), random.Random(2)), 1, None, want=1 | 16 | 32 | 64, cap=n)]
    _run(jobs, tmp_path)


@pytest.mark.gpu
def test_each_reason_alone_rejects_a_group(tmp_path):
    """four groups: one failing proof; one fold_failed word; one pairing word of 0; one clean — each for equal groups and for sizes; and
    with the pairing flag off the pairing words are garbage that is not looked at"""
    jobs = []
    for groups, sizes, n in ((4, None, 40), (1, [1, 7, 24, 3], 35)):
        off = rr.offsets(n, groups, sizes)
        words = _words(n, [off[0]], None)
        jobs.append(Job(words, groups, sizes, fold=[0, 3, 0, 0], ok=[1, 1, 0, 1], flags=rr.FLAG_PAIRING))
        jobs.append(Job(words, groups, sizes, fold=[0, 0xffffffff, 0, 0], ok=[1, 1, 0, 1], flags=rr.FLAG_PAIRING | rr.FLAG_FOLDED))
        jobs.append(Job(words, groups, sizes, fold=[0, 3, 0, 0], ok=[0xdeadbeef, 0, 0, 0x80000000], flags=0))
        jobs.append(Job([0] * n, groups, sizes, fold=[0, 0, 0, 0], ok=[0, 0, 0, 0], flags=0))
        jobs.append(Job([0] * n, groups, sizes, fold=[0, 0, 0, 0], ok=[0, 0, 0, 0], flags=rr.FLAG_PAIRING))
    _run(jobs, tmp_path)
    # (the reference's own answers for the first job, by hand)
    assert rr.finish(jobs[0].words, jobs[0].fold, jobs[0].ok, jobs[0].bytes, jobs[0].flags, 4)["group_ok"] == [0, 0, 0, 1]
    assert rr.finish(jobs[2].words, jobs[2].fold, jobs[2].ok, jobs[2].bytes, 0, 4)["group_ok"] == [0, 0, 1, 1]


@pytest.mark.gpu
def test_cap_below_at_and_above_the_count(tmp_path):
    """7 failing proofs in three tiles and several waves: caps 1, 6, 7, 8 and 600; the summary holds the true count"""
    n = 600
    failing = [5, 63, 64, 255, 256, 300, 599]
    jobs = [Job(_words(n, failing, None), 4, None, cap=cap, seed=cap) for cap in (1, 6, 7, 8, 600)]
    jobs += [Job(_words(n, range(n), None), 1, None, cap=cap, seed=cap) for cap in (1, 255, 257, 599, 600)]
    _run(jobs, tmp_path)
    assert all(rr.finish(j.words, j.fold, j.ok, j.bytes, j.flags, j.G, cap=j.cap)["summary"][1] == (7 if j.G == 4 else n) for j in jobs)


@pytest.mark.gpu
def test_every_combination_of_outputs(tmp_path):
    """each of the 128 sets of outputs, on 4 groups with failures in two of them: what is asked for is right and the rest is untouched"""
    n = 300
    words = _words(n, [0, 74, 75, 256, 299], None)
    _run([Job(words, 4, None, fold=[0, 0, 1, 0], want=want, cap=3, seed=want, repeat=1 + want % 2) for want in range(128)], tmp_path)


@pytest.mark.gpu
def test_the_fault_word_rejects_every_group(tmp_path):
    n = 36
    jobs = [Job([0] * n, 1, RAGGED_5, fault=17), Job(_words(n, [8], None), 4, None, fault=0), Job([0] * n, 4, None, fault=rr.NO_FAULT - 1, flags=0)]
    _run(jobs, tmp_path)
    assert rr.finish(jobs[0].words, jobs[0].fold, jobs[0].ok, jobs[0].bytes, jobs[0].flags, sizes=RAGGED_5, fault=17)["summary"][:3] == [17, 0, 0]


@pytest.mark.gpu
def test_no_proofs_still_give_the_groups_and_the_summary(tmp_path):
    _run([Job([], 1, None), Job([], 4, None, fold=[0, 1, 0, 0], ok=[1, 1, 0, 1], repeat=2)], tmp_path)


# ---- the command line (no GPU: both end before any HIP call)
def test_usage_and_empty_input(tmp_path):
    r = uh.start("results_units", [])
    assert r.returncode == 2 and "usage: results_units finish IN OUT" in r.stderr, (r.returncode, r.stderr)
    empty, out = tmp_path / "empty.bin", tmp_path / "out.bin"
    empty.write_bytes(b"")
    r = uh.start("results_units", ["finish", empty, out])
    assert r.returncode == 2 and "input too short" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()
