"""The record, byte-conversion and small group kernels (csrc/util.hip) one by one against Python big integers
(tests/record_reference.py).  build/util_units (tests/cpp/util_units.hip, built by csrc/Makefile with the library's flags) runs
each kernel through the library's own launcher on raw limbs, bytes and words chosen here, with every output preset to 0xff between
guard bands that the harness checks.

  fold         k_fold_records: the eight-lane teams at n_recs = 1 .. 25 (record tails, teams that are not live, several workgroups),
               records of the fold's cut, of other cuts and whole ones mixed across the lanes of a team, degenerate sums, the failure
               counts — and what a malformed record, a cut beyond the bound and a count that would wrap do
  export       k_export_records: the failed count at the stride's edges, pieces and whole points, the seeded call without statuses
  to_bytes     k_point_to_bytes: the identity with garbage coordinates, every representative, the safegcd inversion at its specials
  bases        k_bases_from_bytes: canonicity, the identity, points off the curve
  scalars      k_scalars_from_bytes: the comparison with r at every word
  to_jacobian, copy
Points are compared as group elements (the identity: Z = 0) unless the kernel promises a form; bytes, flags, words and counts exactly.
One child process per mode (two where a mode's input is another's output), each under a time limit."""
import random
import struct

import numpy as np
import pytest

import msm_reference as ref
import pairing_reference as pr
import record_reference as rr
from msm_reference import P, R
from units_harness import words as _words
import units_harness as uh

pytestmark = pytest.mark.gpu

REPS3 = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
FF = 0xffffffff


def _run(mode, blob, tmp_path, timeout=120):
    """the harness on one input file -> its output words"""
    return uh.as_words(uh.run("util_units", [mode], blob, tmp_path, timeout))


_POOL = None


def _pool():
    """48 points with no small relation between them, and their negatives behind them"""
    global _POOL
    if _POOL is None:
        rnd = random.Random(9090)
        pt, step = ref.mul(rnd.randrange(1, R), ref.G), ref.mul(rnd.randrange(1, R), ref.G)
        pts = []
        for _ in range(48):
            pts.append(pt)
            pt = ref.add(pt, step)
        _POOL = pts + [ref.neg(p) for p in pts]
    return _POOL


def _point_words(pt, rnd, plain=False):
    """27 words of a stored Jacobian form of pt: a random Z (or 1) and random representatives; the identity as (0, 1, 0), or as garbage
    X and Y over Z = 0, Z stored as 0 or as the limb string p"""
    reps = rnd.choice(REPS3)
    if pt is None:
        if plain or rnd.random() < 0.3:
            return ref.jac_words(None, reps=reps)
        return ref.fq_words(rnd.randrange(1, P), reps[0]) + ref.fq_words(rnd.randrange(1, P), reps[1]) + ref.fq_words(0, reps[2])
    return ref.jac_words(pt, 1 if plain or rnd.random() < 0.2 else rnd.randrange(2, P), reps)


def _record(rnd, failed, parts, shift, left, right, reserved=0, fill=True):
    """-> (rr.Record, 328 words).  Pieces j >= parts of the words hold points that no fold may read (fill) — or zeros"""
    pool = _pool()
    words = [failed, parts, shift, reserved]
    for side in (left, right):
        for j in range(rr.PIECES):
            if j < len(side):
                words += _point_words(side[j], rnd)
            else:
                words += _point_words(rnd.choice(pool), rnd) if fill else [0] * 27
    assert len(words) == rr.RECORD_WORDS
    return rr.Record(failed, parts, shift, left, right, reserved), words


def _target_shift(parts):
    """the shift a launch that leaves `parts` pieces has (the first of msm_split_pairs)"""
    return next(s for s, k in pr.msm_split_pairs() if k == parts and s > 0) if parts > 1 else 0


def _cut(kind, parts, shift, salt):
    """the (parts, shift) of a record of one kind, for a fold into (parts, shift)"""
    small = (1, 2, 5, 43)[salt % 4]
    if kind == "same":
        return parts, shift
    if kind == "other_shift":
        return parts, small if parts > 1 else 9            # (a whole point's shift word is not looked at)
    if kind == "fewer":
        return (max(2, parts - 1 - salt % 2), small) if parts > 2 else (1, 0)
    if kind == "more":
        return (min(6, parts + 1 + salt % 2), small) if parts < 6 else (5, small)
    return 1, 0                                            # whole


KINDS = ["same", "other_shift", "fewer", "more", "whole"]


# ====================================================================== fold
class FoldJob:
    def __init__(self, name, n_recs, groups, parts, shift, with_pieces, recs):
        self.name, self.n_recs, self.groups, self.parts, self.shift, self.with_pieces, self.recs = name, n_recs, groups, parts, shift, with_pieces, recs
        self.eff = parts if parts > 1 and with_pieces else 1

    def blob(self):
        out = [struct.pack("<5I", self.n_recs, self.groups, self.parts, self.shift, self.with_pieces)]
        for row in self.recs:
            assert len(row) == self.groups
            for _, words in row:
                out.append(_words(words))
        assert len(self.recs) == self.n_recs
        return b"".join(out)

    def expected(self):
        return rr.fold([[rec for rec, _ in row] for row in self.recs], self.groups, self.eff, self.shift if self.eff > 1 else 0)


def _mixed_job(name, rnd, n_recs, groups, parts, kinds=KINDS, with_pieces=1):
    pool, shift = _pool(), _target_shift(parts)
    recs = []
    for i in range(n_recs):
        row = []
        for g in range(groups):
            k, sh = _cut(kinds[(i + 2 * g) % len(kinds)], parts, shift, i + g)
            sides = [[rnd.choice(pool + [None] * 8) for _ in range(k)] for _ in (0, 1)]
            row.append(_record(rnd, (7 * i + 3 * g) % 5 * (g + 1), k, sh, sides[0], sides[1]))
        recs.append(row)
    return FoldJob(name, n_recs, groups, parts, shift, with_pieces, recs)


SHAPES = [(1, 1, 1), (2, 1, 1), (7, 1, 1), (8, 1, 1), (9, 2, 1), (17, 3, 3), (25, 5, 6), (3, 2, 2)]


def _fold_jobs():
    rnd = random.Random(606)
    pool = _pool()
    jobs = [_mixed_job(f"shape{s}", rnd, *s) for s in SHAPES]
    # every kind of cut inside one fold and across the lanes of one team, for every target
    jobs += [_mixed_job(f"mixed{parts}", rnd, 10, 2, parts) for parts in (1, 2, 3, 6)]
    # parts > 1 asked for without piece arrays: the launcher folds whole points
    jobs.append(_mixed_job("no_piece_arrays", rnd, 5, 2, 3, with_pieces=0))
    for parts in (1, 3):
        shift = _target_shift(parts)

        def same(pts_l, pts_r, failed=0):
            return _record(rnd, failed, parts, shift, pts_l, pts_r)

        a, b, c = ([pool[3 * parts * t + j] for j in range(parts)] for t in range(3))
        neg = lambda ps: [ref.neg(p) for p in ps]
        ident = [None] * parts
        # all records equal, word for word: every butterfly step is a doubling
        one = same(a, b)
        jobs.append(FoldJob(f"equal{parts}", 8, 1, parts, shift, 1, [[one]] * 8))
        # records r and r + 4 cancel: the butterfly adds identities from its first step on
        rows = [[same(pool[t:t + parts], pool[t + 9:t + 9 + parts])] for t in range(4)]
        rows += [[same(neg(pool[t:t + parts]), neg(pool[t + 9:t + 9 + parts]))] for t in range(4)]
        jobs.append(FoldJob(f"cancel{parts}", 8, 1, parts, shift, 1, rows))
        # identity partial sums in the middle of the butterfly, and as the result: lanes 0 and 3 cancel at d = 4, lanes 2 and 1 carry c and -c
        rows = [same(a, a), same(ident, ident), same(c, c), same(b, b), same(neg(a), neg(a)), same(neg(c), neg(c)), same(ident, ident), same(neg(b), neg(b))]
        jobs.append(FoldJob(f"middle{parts}", 8, 1, parts, shift, 1, [[r] for r in rows]))
        # a record all of whose pieces are the identity; one side the identity and the other not (in two groups, either side)
        rows = [[same(ident, ident, 2), same(a, ident, 1)], [same(ident, b), same(ident, ident)], [same(ident, ident), same(c, ident, 4)]]
        jobs.append(FoldJob(f"sides{parts}", 3, 2, parts, shift, 1, rows))
    return jobs


def _parse_fold(out, jobs):
    res, at = [], 0
    for jb in jobs:
        eff = int(out[at]); at += 1
        assert eff == jb.eff
        acc = out[at:at + 27 * 2 * jb.groups].reshape(2 * jb.groups, 27); at += acc.size
        cnt = 2 * jb.groups * eff if eff > 1 else 0
        pieces = out[at:at + 32 * cnt].reshape(cnt, 32); at += pieces.size
        ready = out[at:at + 32 * cnt].reshape(cnt, 32); at += ready.size
        failed = out[at:at + jb.groups].tolist(); at += jb.groups
        res.append(dict(acc=acc, pieces=pieces, ready=ready, failed=failed))
    assert at == len(out)
    return res


def _check_fold(jb, got, check_failed=True):
    """every output of one fold against the reference"""
    want, failed = jb.expected()
    for g in range(jb.groups):
        for side in (0, 1):
            if jb.eff == 1:
                w = got["acc"][2 * g + side].tolist()
                assert rr.in_range(w), (jb.name, g, side)
                assert ref.jac_point(w) == want[g][side][0], (jb.name, g, side)
                continue
            assert (got["acc"] == FF).all(), jb.name + ": acc written by a fold into pieces"
            for j in range(jb.eff):
                k = (2 * g + side) * jb.eff + j
                w, rd = got["pieces"][k].tolist(), got["ready"][k].tolist()
                assert rr.in_range(w[:27]) and rr.in_range(rd[:27]), (jb.name, g, side, j)
                assert w[27:] == [0] * 5 and rd[27:] == [0] * 5, (jb.name, g, side, j, "the slot's padding")
                assert ref.jac_point(w[:27]) == want[g][side][j], (jb.name, g, side, j)
                assert rr.values_of(rd[:27]) == rr.ready_of(w[:27]), (jb.name, g, side, j, "ready is not (X Z, Y, Z^3)")
    if check_failed:
        assert got["failed"] == failed, (jb.name, got["failed"], failed)


@pytest.fixture(scope="module")
def export_run(tmp_path_factory):
    jobs = _export_jobs()
    out = _run("export", struct.pack("<I", len(jobs)) + b"".join(j["blob"] for j in jobs), tmp_path_factory.mktemp("export"))
    at = 0
    for j in jobs:
        j["out"] = out[at:at + rr.RECORD_WORDS * j["groups"]].reshape(j["groups"], rr.RECORD_WORDS); at += j["out"].size
    assert at == len(out)
    return jobs


@pytest.fixture(scope="module")
def fold_run(tmp_path_factory, export_run):
    """one child process: the shapes, the mixtures, the degenerate sums, the fixes' cases, and a fold over records the export mode wrote"""
    jobs = _fold_jobs() + _fix_jobs()
    # exported records, fed straight back: the two exports of three groups at (3, 44)
    ex = [j for j in export_run if j["name"].startswith("refold")]
    assert len(ex) == 2
    recs = [[(None, e["out"][g].tolist()) for g in range(3)] for e in ex]
    jobs.append(FoldJob("refold", 2, 3, 3, 44, 1, recs))
    out = _run("fold", struct.pack("<I", len(jobs)) + b"".join(j.blob() for j in jobs), tmp_path_factory.mktemp("fold"))
    return {j.name: (j, g) for j, g in zip(jobs, _parse_fold(out, jobs))}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fold_shapes(fold_run, shape):
    """(n_recs, groups, parts): one record, a team's tail (n_recs % 8 != 0), 18 teams of which two are live in the last workgroup
    (17, 3, 3), five groups of six pieces — each with records of every cut dealt over the lanes"""
    _check_fold(*fold_run[f"shape{shape}"])


@pytest.mark.parametrize("parts", [1, 2, 3, 6])
def test_fold_mixed_cuts(fold_run, parts):
    """the same cut, the same parts with another shift, fewer pieces, more pieces and whole points inside one fold: a record of another cut
    joins piece 0 with its pieces put together, sum_j 2^(shift j) piece_j"""
    jb, got = fold_run[f"mixed{parts}"]
    kinds = {rr.record_kind(rec, jb.eff, jb.shift) for row in jb.recs for rec, _ in row}
    assert kinds == {"same", "foreign"}
    cuts = {(rec.parts, rec.shift) for row in jb.recs for rec, _ in row}
    assert len(cuts) >= (3 if parts == 1 else 5), cuts
    _check_fold(jb, got)


def test_fold_without_piece_arrays_gives_whole_points(fold_run):
    jb, got = fold_run["no_piece_arrays"]
    assert jb.eff == 1 and jb.parts == 3
    _check_fold(jb, got)


@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("name", ["equal", "cancel", "middle", "sides"])
def test_fold_degenerate_sums(fold_run, name, parts):
    """all records equal (every butterfly step a doubling), pairs that cancel (identity partial sums in the middle of the butterfly and as
    the result), identity pieces with Z = 0 over non-zero X and Y, a record of identities, one side the identity"""
    jb, got = fold_run[name + str(parts)]
    want, _ = jb.expected()
    if name in ("cancel", "middle"):
        assert all(p is None for g in want for s in g for p in s)
    _check_fold(jb, got)


def test_fold_failed_is_written_once_per_group(fold_run):
    """per-group sums over all records with different counts per group, with parts = 1 and with parts > 1"""
    for name in ("shape(9, 2, 1)", "shape(17, 3, 3)", "shape(25, 5, 6)", "mixed6"):
        jb, got = fold_run[name]
        _, failed = jb.expected()
        assert got["failed"] == failed and len(set(failed)) == len(failed) > 1 and all(failed), (name, failed)


def test_fold_of_exported_records_gives_back_the_points(fold_run, export_run):
    jb, got = fold_run["refold"]
    ex = [j for j in export_run if j["name"].startswith("refold")]
    for g in range(3):
        for side in (0, 1):
            want = None
            for e in ex:
                want = ref.add(want, rr.weighted_sum(e["points"][(2 * g + side) * 3:(2 * g + side) * 3 + 3], 44))
            pcs = [ref.jac_point(got["pieces"][(2 * g + side) * 3 + j][:27].tolist()) for j in range(3)]
            assert rr.weighted_sum(pcs, 44) == want
    assert got["failed"] == [sum(e["counts"][g] for e in ex) for g in range(3)]


# ---------------------------------------------------------------------- the fixes the tests pin
def _fix_jobs():
    rnd = random.Random(707)
    pool = _pool()
    jobs = []
    good = lambda i, failed=0: _record(rnd, failed, 1, 0, [pool[i]], [pool[i + 1]])
    zero = (rr.Record(0, 0, 0, [], []), [0] * rr.RECORD_WORDS)                      # a record never written
    seven = _record(rnd, 0, 7, 0, [pool[20 + j] for j in range(6)], [pool[30 + j] for j in range(6)])
    huge = _record(rnd, 2, 0x80000001, 3, [pool[5]], [pool[6]])
    # group 0 holds the malformed record, group 1 does not
    for name, bad in (("zeroed", zero), ("seven", seven), ("huge_parts", huge)):
        jobs.append(FoldJob("bad_" + name, 3, 2, 1, 0, 1, [[good(0), good(2)], [bad, good(4)], [good(6), good(8)]]))
    # into pieces as well: a zeroed record among records of the fold's cut
    s3 = _target_shift(3)
    cut3 = lambda i: _record(rnd, 0, 3, s3, pool[i:i + 3], pool[i + 3:i + 6])
    jobs.append(FoldJob("bad_zeroed_pieces", 2, 1, 3, s3, 1, [[cut3(0)], [zero]]))
    # the bound on shift (parts - 1): at the bound (256) a record is put together, one past it (257) it is malformed
    at_bound = _record(rnd, 0, 2, rr.MAX_SPAN, [pool[10], pool[11]], [pool[12], pool[13]])
    past = _record(rnd, 0, 2, rr.MAX_SPAN + 1, [pool[10], pool[11]], [pool[12], pool[13]])
    past5 = _record(rnd, 0, 5, 65, pool[10:15], pool[15:20])                           # 65 * 4 = 260
    jobs.append(FoldJob("span_at_bound", 2, 1, 1, 0, 1, [[good(0)], [at_bound]]))
    jobs.append(FoldJob("span_past_bound", 2, 1, 1, 0, 1, [[good(0)], [past]]))
    jobs.append(FoldJob("span_past_bound5", 2, 1, 3, s3, 1, [[cut3(0)], [past5]]))
    # a record of the fold's own cut is not put together: its shift is not bounded
    jobs.append(FoldJob("span_same_cut", 2, 1, 2, 1000, 1, [[_record(rnd, 1, 2, 1000, pool[0:2], pool[2:4])], [_record(rnd, 2, 2, 1000, pool[4:6], pool[6:8])]]))
    # counts that wrap 32 bits: in one lane's loop (records 0 and 8), across the butterfly (records 0 and 1), three of them
    half = 0x80000000
    jobs.append(FoldJob("wrap_butterfly", 2, 1, 1, 0, 1, [[good(0, half)], [good(2, half)]]))
    jobs.append(FoldJob("wrap_lane", 9, 1, 1, 0, 1, [[good(0, half)]] + [[good(2 * i)] for i in range(1, 8)] + [[good(16, half)]]))
    jobs.append(FoldJob("wrap_three", 3, 2, 1, 0, 1, [[good(0, half), good(2, 1)], [good(4, half), good(6, 2)], [good(8, half), good(10, 3)]]))
    jobs.append(FoldJob("wrap_one_more", 2, 1, 1, 0, 1, [[good(0, FF)], [good(2, 1)]]))
    return jobs


@pytest.mark.parametrize("name", ["zeroed", "seven", "huge_parts", "zeroed_pieces"])
def test_a_malformed_record_fails_the_fold(fold_run, name):
    """parts = 0 (a record never written), 7 or 2^31 + 1: the record contributes the identity, and fold_failed of ITS group is non-zero —
    the fold cannot report ok without the shard's proofs.  (Before the fix fold_failed was the sum of the failed words: 0 for the zeroed
    record and for parts = 7.)"""
    jb, got = fold_run["bad_" + name]
    _check_fold(jb, got, check_failed=False)
    _, failed = jb.expected()
    print(name, "fold_failed", got["failed"], "reference", failed)
    assert got["failed"][0] != 0
    assert got["failed"] == failed


def test_a_cut_beyond_the_span_bound_is_malformed(fold_run):
    """shift (parts - 1) = 256: put together; 257 (the smallest value past the bound) and 260: the identity and a failure; a record of the
    fold's own cut at shift 1000: added piece by piece as ever"""
    for name in ("span_at_bound", "span_same_cut"):
        jb, got = fold_run[name]
        assert {rr.record_kind(rec, jb.eff, jb.shift) for row in jb.recs for rec, _ in row} <= {"same", "foreign"}
        _check_fold(jb, got)
    for name in ("span_past_bound", "span_past_bound5"):
        jb, got = fold_run[name]
        assert rr.record_kind(jb.recs[1][0][0], jb.eff, jb.shift) == "malformed"
        print(name, "fold_failed", got["failed"])
        assert got["failed"] == [1]
        _check_fold(jb, got)


@pytest.mark.parametrize("name", ["wrap_butterfly", "wrap_lane", "wrap_three", "wrap_one_more"])
def test_the_failure_count_saturates(fold_run, name):
    """two counts of 2^31 — in one lane's loop, or met in the butterfly — are 2^32 - 1, not 0"""
    jb, got = fold_run[name]
    print(name, "fold_failed", got["failed"])
    assert got["failed"][0] == FF
    _check_fold(jb, got)


# ====================================================================== export
GS = [1, 255, 256, 257, 600]
EDGES = [0, 255, 256, -1]          # the stride's edges: the only proofs with a non-zero status


def _statuses(gs, g):
    """group g's statuses: non-zero, positive and negative, at a subset of the stride's edges that differs from group to group"""
    st = [0] * gs
    mask = (0b0110, 0b1011, 0b1111)[g % 3]
    for b, e in enumerate(EDGES):
        i = e if e >= 0 else gs - 1
        if i < gs and mask >> b & 1:
            st[i] = (-3 - b) if (b + g) % 2 else (1 << (8 * b)) + g
    return st


def _export_job(name, rnd, groups, gs, parts, shift, from_pieces, with_status):
    pool = _pool()
    n_pts = 2 * groups * (parts if from_pieces else 1)
    points = [rnd.choice(pool + [None] * 6) for _ in range(n_pts)]
    words = [_point_words(p, rnd) for p in points]
    st = [_statuses(gs, g) for g in range(groups)] if with_status else [[] for _ in range(groups)]
    blob = struct.pack("<6I", groups, gs if with_status else 0, parts, shift, from_pieces, with_status) + b"".join(_words(w) for w in words)
    if with_status:
        blob += np.asarray([s for row in st for s in row], dtype="<i4").tobytes()
    return dict(name=name, groups=groups, gs=gs, parts=parts if from_pieces else 1, shift=shift if from_pieces else 0, from_pieces=from_pieces, points=points,
                words=words, statuses=st, counts=[sum(1 for s in row if s) for row in st], blob=blob)


def _export_jobs():
    rnd = random.Random(808)
    jobs = []
    for i, gs in enumerate(GS):
        parts = i + 1
        jobs.append(_export_job(f"pieces_gs{gs}", rnd, 3, gs, parts, _target_shift(parts), 1, 1))
        jobs.append(_export_job(f"whole_gs{gs}", rnd, 3, gs, 1, 0, 0, 1))
    jobs.append(_export_job("pieces_gs600_6", rnd, 3, 600, 6, _target_shift(6), 1, 1))
    jobs.append(_export_job("seeded_whole", rnd, 1, 0, 1, 0, 0, 0))          # status = nullptr, n = 0: the seeded and add_msm call
    jobs.append(_export_job("seeded_pieces", rnd, 2, 0, 4, _target_shift(4), 1, 0))
    jobs.append(_export_job("refold_a", rnd, 3, 257, 3, 44, 1, 1))
    jobs.append(_export_job("refold_b", rnd, 3, 600, 3, 44, 1, 1))
    return jobs


def test_export_records(export_run):
    """header: the non-zero statuses of the group (over gs proofs with a stride of 256: the edges 0, 255, 256, gs - 1), the cut, reserved = 0;
    pieces j < parts: the limbs as they were; pieces j >= parts: the identity with Z = 0"""
    seen_parts, seen_counts = set(), set()
    for j in export_run:
        parts = j["parts"]
        for g in range(j["groups"]):
            rec = j["out"][g].tolist()
            assert rec[:4] == rr.export_header(j["statuses"][g], parts, j["shift"]), (j["name"], g, rec[:4])
            seen_counts.add(rec[0])
            for side in (0, 1):
                for k in range(rr.PIECES):
                    w = rec[4 + 27 * (rr.PIECES * side + k):4 + 27 * (rr.PIECES * side + k + 1)]
                    if k < parts:
                        assert w == j["words"][(2 * g + side) * parts + k], (j["name"], g, side, k)
                    else:
                        assert rr.in_range(w) and ref.fq_value(w[18:27]) == 0 and ref.from_limbs(w[18:27]) in (0, P), (j["name"], g, side, k, w)
        seen_parts.add((j["from_pieces"], parts))
    assert seen_parts >= {(1, k) for k in range(1, 7)} | {(0, 1)}
    assert seen_counts >= {0, 1, 2, 3, 4}, seen_counts


def test_export_statuses_sit_at_the_stride_edges_only(export_run):
    for j in export_run:
        for row in j["statuses"]:
            nz = {i for i, s in enumerate(row) if s}
            assert nz <= {0, 255, 256, len(row) - 1}
    rows = [row for j in export_run for row in j["statuses"] if len(row) == 600]
    assert any(r[0] and r[255] and r[256] and r[599] for r in rows) and any(s < 0 for r in rows for s in r) and any(s > 0 for r in rows for s in r)


# ====================================================================== to_bytes -> bases -> to_jacobian -> to_bytes
def _inverse_specials():
    """the integers the device's safegcd inversion is handed (the canonical Montgomery representative of Z): the specials of
    tests/test_field_host.py without 0"""
    return [1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 1 << 253, (1 << 253) - 1, 1 << 128, (1 << 128) - 1, (1 << 30) - 1, 1 << 30, (1 << 60) + 1,
            P - (1 << 200), 0x5555555555555555555555555555555555555555555555555555555555555555 % P]


def _to_bytes_cases():
    """(point, 27 words)"""
    rnd = random.Random(909)
    pool = _pool()
    cases = []
    for i, a in enumerate(_inverse_specials()):
        for high in (False, True):
            pt, z = pool[(2 * i + high) % len(pool)], pr.mont_value(a)
            reps = REPS3[(i + 3 * high) % 8]
            w = ref.fq_words(pt[0] * z * z, reps[0]) + ref.fq_words(pt[1] * z * z * z, reps[1]) + pr.limbs(a + (P if high else 0))
            assert ref.jac_point(w) == pt
            cases.append((pt, w))
    for i in range(8):                                       # Z = 0 (stored as 0 and as p) under garbage X and Y
        w = ref.fq_words(rnd.randrange(1, P), i & 1) + ref.fq_words(rnd.randrange(1, P), i & 2) + ref.fq_words(0, i & 4)
        cases.append((None, w))
    cases.append((None, ref.jac_words(None)))
    for i, reps in enumerate(REPS3):                         # Z = 1 and a random Z in every representative
        cases.append((pool[i], ref.jac_words(pool[i], 1, reps)))
        cases.append((pool[8 + i], ref.jac_words(pool[8 + i], rnd.randrange(2, P), reps)))
    while len(cases) < 130:
        pt = rnd.choice(pool)
        cases.append((pt, ref.jac_words(pt, rnd.randrange(2, P), rnd.choice(REPS3))))
    return cases


TO_BYTES_N = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def to_bytes_run(tmp_path_factory):
    cases = _to_bytes_cases()
    jobs = []
    for n in TO_BYTES_N:
        for reserve in (0, 1):
            off = 0 if n == 130 else (7 * n + 31 * reserve) % 60
            jobs.append((n, reserve, [cases[(off + i) % len(cases)] for i in range(n)]))
    blob = struct.pack("<I", len(jobs)) + b"".join(struct.pack("<II", n, rs) + b"".join(_words(w) for _, w in cs) for n, rs, cs in jobs)
    out = _run("to_bytes", blob, tmp_path_factory.mktemp("to_bytes"))
    res, at = [], 0
    for n, rs, cs in jobs:
        by = out[at:at + 16 * n].tobytes(); at += 16 * n
        fl = out[at:at + n].tolist(); at += n
        res.append((n, rs, cs, by, fl))
    assert at == len(out)
    return res


@pytest.mark.parametrize("reserve", [0, 1])
@pytest.mark.parametrize("n", TO_BYTES_N)
def test_point_to_bytes(to_bytes_run, n, reserve):
    """exact bytes and flags: Z = 0 under garbage X and Y is 64 zero bytes with flag 1; Z = 1, random Z, X, Y, Z as m and as m + p; Z whose
    stored integer — what the device's safegcd inversion is handed — is 1, 2, 3, p - 1, p - 2, (p +- 1) / 2, 2^253, 2^128, 2^30, ...;
    launched with and without the LDS request of the auxiliary stream"""
    _, _, cs, by, fl = next(r for r in to_bytes_run if r[0] == n and r[1] == reserve)
    for i, (pt, _) in enumerate(cs):
        want, flag = rr.point_to_bytes(pt)
        assert by[64 * i:64 * i + 64] == want and fl[i] == flag, (n, reserve, i, pt)
    if n == 130:
        assert sum(fl) == 9


BASES_N = [1, 255, 256, 257]


def _bases_cases():
    """(64 bytes, point or None, flag)"""
    pool = _pool()
    enc = lambda x, y: int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little")
    cases = []
    for i in range(6):
        x, y = pool[i]
        other = next(q[1] for q in pool if (q[1] * q[1] - 3) % P)      # (0, y) is off the curve for this y
        assert x + P < 1 << 256 and y + P < 1 << 256
        cases += [(enc(x, y), (x, y), 0), (enc(x, P - y), (x, P - y), 0), (bytes(64), None, 0),
                  (enc(P, y), None, 1), (enc(x + P, y), None, 1), (enc(x, P), None, 1), (enc(x, y + P), None, 1),
                  (enc(x | 1 << 255, y), None, 1), (enc(x, y | 1 << 255), None, 1), (enc(x | 1 << 254, y), None, 1), (enc((1 << 256) - 1, (1 << 256) - 1), None, 1),
                  (enc(x, (y + 1) % P), None, 1), (enc(x, 0), None, 1), (enc(0, other), None, 1), (enc(P, 0), None, 1), (enc(0, P), None, 1), (enc(P, P), None, 1)]
    for b, pt, flag in cases:
        assert rr.point_from_bytes(b) == (pt, flag)
    return cases


@pytest.fixture(scope="module")
def bases_run(tmp_path_factory, to_bytes_run):
    cases = _bases_cases()
    jobs = [[cases[(11 * n + i) % len(cases)] for i in range(n)] for n in BASES_N]
    # the bytes k_point_to_bytes wrote for its 130 points
    _, _, cs, by, fl = next(r for r in to_bytes_run if r[0] == 130 and r[1] == 0)
    jobs.append([(by[64 * i:64 * i + 64], pt, 0) for i, (pt, _) in enumerate(cs)])
    blob = struct.pack("<I", len(jobs)) + b"".join(struct.pack("<I", len(j)) + b"".join(b for b, _, _ in j) for j in jobs)
    out = _run("bases", blob, tmp_path_factory.mktemp("bases"))
    res, at = [], 0
    for j in jobs:
        pts = out[at:at + 18 * len(j)].reshape(len(j), 18); at += pts.size
        fl = out[at:at + len(j)].tolist(); at += len(j)
        res.append((j, pts, fl))
    assert at == len(out)
    return res


@pytest.mark.parametrize("k", range(len(BASES_N) + 1), ids=[f"n{n}" for n in BASES_N] + ["round_trip"])
def test_bases_from_bytes(bases_run, k):
    """a point and its negative; the all-zero identity (flag 0); x or y = p, + p, with the top bits set; (x, y + 1), (x, 0), (0, y) off the
    curve: each bad encoding gives flag 1 and the exact identity (all-zero limbs).  The last job reads the bytes k_point_to_bytes wrote"""
    cases, pts, fl = bases_run[k]
    for i, (b, pt, flag) in enumerate(cases):
        w = pts[i].tolist()
        assert fl[i] == flag, (i, b.hex())
        if pt is None:
            assert w == [0] * 18, (i, b.hex())
        else:
            assert rr.in_range(w, 2) and (ref.fq_value(w[:9]), ref.fq_value(w[9:])) == pt, (i, b.hex())


@pytest.fixture(scope="module")
def chain_run(tmp_path_factory, bases_run):
    """what k_bases_from_bytes left (n = 257, and the round trip's 130), through k_affine_to_jacobian, then through k_point_to_bytes"""
    tmp = tmp_path_factory.mktemp("chain")
    aff = [(pt, pts[i].tolist()) for cases, pts, _ in bases_run[3:] for i, (_, pt, _) in enumerate(cases)]
    sizes = [0, 1, 63, 64, 65, len(aff)]
    blob = struct.pack("<I", len(sizes)) + b"".join(struct.pack("<I", n) + b"".join(_words(w) for _, w in aff[:n]) for n in sizes)
    out = _run("to_jacobian", blob, tmp)
    assert len(out) == 27 * sum(sizes)
    jac = out[27 * (sum(sizes) - len(aff)):].reshape(len(aff), 27)
    heads = out[:27 * (sum(sizes) - len(aff))]
    out2 = _run("to_bytes", struct.pack("<III", 1, len(aff), 0) + jac.tobytes(), tmp)
    return aff, sizes, heads, jac, out2[:16 * len(aff)].tobytes(), out2[16 * len(aff):].tolist()


def test_affine_to_jacobian(chain_run):
    """the identity goes to the identity with Z = 0, any other point keeps its limbs and gets Z = one; n = 0 launches nothing"""
    aff, sizes, heads, jac, _, _ = chain_run
    one = ref.fq_words(1)
    n_ident = 0
    for (pt, w), j in zip(aff, jac.tolist()):
        if pt is None:
            assert ref.from_limbs(j[18:27]) in (0, P) and rr.in_range(j)
            n_ident += 1
        else:
            assert j[:18] == w and j[18:] == one
    assert n_ident > 50 and len(aff) - n_ident > 50
    at = 0
    for n in sizes[:-1]:                # the smaller launches wrote the same limbs
        assert (heads[at:at + 27 * n].reshape(n, 27) == jac[:n]).all()
        at += 27 * n


def test_bases_are_accepted_by_to_jacobian_and_to_bytes(chain_run):
    aff, _, _, _, by, fl = chain_run
    for i, (pt, _) in enumerate(aff):
        want, flag = rr.point_to_bytes(pt)
        assert by[64 * i:64 * i + 64] == want and fl[i] == flag, i


# ====================================================================== scalars
def _scalar_cases():
    vals = [0, 1, R - 1, R, R + 1, 1 << 254, (1 << 256) - 1]
    for k in range(8):              # each word position decides the comparison once in each direction
        vals += [R + (1 << (32 * k)), R - (1 << (32 * k))]
    rnd = random.Random(1010)
    return vals + [rnd.randrange(1 << 256) for _ in range(9)]


@pytest.fixture(scope="module")
def scalars_run(tmp_path_factory):
    vals = _scalar_cases()
    jobs = [[vals[(5 * n + i) % len(vals)] for i in range(n)] for n in (1, 255, 256, 257)]
    blob = struct.pack("<I", len(jobs)) + b"".join(struct.pack("<I", len(j)) + b"".join(v.to_bytes(32, "little") for v in j) for j in jobs)
    out = _run("scalars", blob, tmp_path_factory.mktemp("scalars"))
    res, at = [], 0
    for j in jobs:
        w = out[at:at + 8 * len(j)].reshape(len(j), 8); at += w.size
        fl = out[at:at + len(j)].tolist(); at += len(j)
        res.append((j, w, fl))
    assert at == len(out)
    return res


@pytest.mark.parametrize("k", range(4), ids=["n1", "n255", "n256", "n257"])
def test_scalars_from_bytes(scalars_run, k):
    """0, 1, r - 1, r, r + 1, 2^254, 2^256 - 1, r +- 2^(32 k): refused exactly from r on, and then the words are zero"""
    vals, w, fl = scalars_run[k]
    for i, v in enumerate(vals):
        words, flag = rr.scalar_from_bytes(v.to_bytes(32, "little"))
        assert fl[i] == flag and w[i].tolist() == words, (i, hex(v))
    if k:
        assert {v for v in vals} >= set(_scalar_cases()[:23])


# ====================================================================== copy
def test_copy_words(tmp_path):
    """word counts 0, 1, 255, 256 and 257 between guard bands, with and without the LDS request"""
    rnd = np.random.RandomState(3)
    jobs = [(n, rs, rnd.randint(0, 1 << 32, size=n, dtype=np.uint64).astype("<u4")) for n in (0, 1, 255, 256, 257) for rs in (0, 1)]
    out = _run("copy", struct.pack("<I", len(jobs)) + b"".join(struct.pack("<II", n, rs) + w.tobytes() for n, rs, w in jobs), tmp_path)
    at = 0
    for n, rs, w in jobs:
        assert (out[at:at + n] == w).all(), (n, rs)
        at += n
    assert at == len(out)
