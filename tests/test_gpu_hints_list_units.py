"""The hinted decompression stage with its miss list (k_decompress_hinted + k_decompress_misses,
halo2_verifier_amd/csrc/verify_kernels.hip; include/h2v_hints.h), through tests/cpp/hints_list_units.hip and the launchers
decompress_begin_enqueue / decompress_range_enqueue / decompress_finish_enqueue, on programmed points and hints.  Every job with hints
runs with the list given: there is no hinted stage without one.

A wave of the first kernel whose live lanes all miss takes its roots in place; a wave with a hit and a miss stores a
placeholder for its misses and lists their point indices, and the second kernel takes those roots densely.  Whatever the hints: pts,
phi (as field elements), ycanon bytes and status words equal the unhinted stage's on the same points, which itself agrees with
hints_reference.decode; the miss word is hints_reference.count_misses; the list holds exactly the points of mixed waves that missed,
each once, inside the segment of the piece that listed them; every buffer lies between guard bands (the harness ends with status 5
on a write past one).

Shapes (Np = 3, one lane per point): n = 1 (3 lanes), 21 (63), 22 (66), 43 (129: three waves, so that a whole-miss wave can lie
between two mixed ones), n = 22 cut [0, 7, 22] and n = 43 cut [0, 7, 30, 43] (a piece's waves start at the piece: lane 0 of a piece
is its first point).  Hint sets: hints_reference.HINT_SETS; one wrong hint at lane 0, at lane 63 and at the last live lane of every
wave of the whole run; every second PROOF without a row (zeros); wave 0 all wrong with wave 1 alternating (both paths in one launch).
Each from a buffer of its own and from the ycanon buffer itself.  Point sets: valid points; the same with undecodable ones at main and
opening slots; and, at n = 43, every kind of undecodable point (a non-residue x, x >= p, the identity flag) at a main slot and at the
opening slot, paired with a right-looking, a zero and a wrong hint, once in a mixed wave (wave 0) and once in a whole-miss wave (wave 1)."""
import functools
import random

import pytest

import hints_reference as hr
import units_harness as uh

pytestmark = pytest.mark.gpu

PROG = "hints_list_units"
NP, N_MAIN, PROOF_LEN, OFFSETS = 3, 2, 128, (0, 64, 96)
ST_TRANSCRIPT, ST_OPENING = -30, -10
SHAPES = [(1, [0, 1]), (21, [0, 21]), (22, [0, 22]), (43, [0, 43]), (22, [0, 7, 22]), (43, [0, 7, 30, 43])]
OWN_SETS = ("lane0", "lane63", "last_live", "alt_proofs", "wave0_wrong_wave1_alt")
PAIRINGS = ("pair_looks_right", "pair_zero", "pair_wrong")
NEVER = 0xffffffff

decode = functools.lru_cache(maxsize=None)(hr.decode)


def is_hit(pt, hint):
    y = decode(pt)
    return y is not None and bytes(hint) == hr.le32(y)


def _bad_points(rnd):
    return (hr.encode(hr.non_residue_x(rnd.randrange(hr.P // 2)), 1), hr.encode(hr.P + rnd.randrange(1 << 200), 0), hr.encode(rnd.randrange(1, hr.P), 1, identity=1))


def _points(n, mixed, seed):
    """n x NP compressed points; mixed: undecodable ones of every kind at main slots (0, 1) and at the opening slot (2)"""
    rnd = random.Random(seed)
    pts = [[hr.random_point(rnd) for _ in range(NP)] for _ in range(n)]
    if mixed:
        nonres, big, ident = _bad_points(rnd)
        if n == 1:
            pts[0][0], pts[0][2] = nonres, ident
        else:
            for proof, slot, bad in [(1, 0, nonres), (2, 2, nonres), (3, 1, big), (4, 2, big), (5, 0, ident), (6, 2, ident), (n - 1, 2, nonres), (8, 0, big), (8, 2, ident)]:
                pts[proof][slot] = bad
    return pts


# n = 43: wave 0 is points 0 .. 63 (proofs 0 .. 20 and one point of 21), wave 1 points 64 .. 127 (proofs 22 .. 41 whole)
BAD_AT = [(first + k, slot) for first in (1, 23) for k, slot in enumerate((0, 2, 1, 2, 0, 2))]


def _bad_everywhere(seed):
    """43 proofs with the three kinds of undecodable point at a main and at the opening slot, in wave 0 and again in wave 1"""
    rnd = random.Random(seed)
    pts = [[hr.random_point(rnd) for _ in range(NP)] for _ in range(43)]
    nonres, big, ident = _bad_points(rnd)
    for (proof, slot), bad in zip(BAD_AT, (nonres, nonres, big, big, ident, ident) * 2):
        pts[proof][slot] = bad
    return pts


def _looks_right(pt):
    """what a sender who ignored the refusal might send for an undecodable point: the root candidate of x^3 + 3 with x taken mod p and
    the flags' parity — a canonical value of the right parity that only the decoding rules turn down"""
    b = bytearray(pt)
    sign = 1 if b[31] & hr.FLAG_SIGN else 0
    b[31] &= 0x3f
    x = int.from_bytes(b, "little") % hr.P
    y = pow((x ** 3 + 3) % hr.P, (hr.P + 1) // 4, hr.P)
    return hr.le32(y if (y & 1) == sign else hr.P - y)


def _pairing_hints(pairing, flat, seed):
    """wave 0 right, wave 1 all wrong, the rest right — and every undecodable point's hint by `pairing`"""
    rnd = random.Random(seed)
    out = []
    for t, pt in enumerate(flat):
        y = decode(pt)
        if y is None:
            out.append({"pair_looks_right": _looks_right(pt), "pair_zero": bytes(32), "pair_wrong": bytes(rnd.randrange(256) for _ in range(32))}[pairing])
        else:
            out.append(hr.le32(y ^ 2) if 64 <= t < 128 else hr.le32(y))
    return b"".join(out)


def _own_set(kind, flat):
    total = len(flat)
    out = []
    for t, pt in enumerate(flat):
        y = decode(pt) or 0
        right, wrong = hr.le32(y), hr.le32(y ^ 2)     # (a flipped bit that keeps the parity: only the curve check can tell)
        if kind == "lane0":
            h = wrong if t % 64 == 0 else right
        elif kind == "lane63":
            h = wrong if t % 64 == 63 else right
        elif kind == "last_live":
            h = wrong if t == min(t // 64 * 64 + 63, total - 1) else right
        elif kind == "alt_proofs":
            h = bytes(32) if (t // NP) % 2 else right
        else:
            h = wrong if t < 64 else (right if t >= 128 or t % 2 == 0 else bytes(32))
        out.append(h)
    return b"".join(out)


def _proofs(pts):
    out = []
    for row in pts:
        proof = bytearray(b"\x5a" * PROOF_LEN)
        for off, pt in zip(OFFSETS, row):
            proof[off:off + 32] = pt
        out.append(bytes(proof))
    return out


def _job(proofs, cut, hints, in_place=False):
    n = len(proofs)
    head = [n, NP, N_MAIN, PROOF_LEN, 0 if hints is None else (3 if in_place else 1), len(cut) - 1] + list(cut) + list(OFFSETS)
    return uh.words(head) + b"".join(proofs) + (hints or b"")


def _read(cur, n):
    pts = [(cur.num(), cur.num(), cur.num(), cur.num(), cur.word(), cur.take(32)) for _ in range(n * NP)]
    status = [cur.sword() for _ in range(n)]
    return pts, status, cur.word(), cur.word(), [cur.word() for _ in range(n * NP)]


def _expected_list(flat, hints, cut):
    """-> per piece (first point, end point, the points its mixed waves list)"""
    out = []
    for a, b in zip(cut, cut[1:]):
        listed = set()
        for w0 in range(a * NP, b * NP, 64):
            lanes = range(w0, min(w0 + 64, b * NP))
            missing = [t for t in lanes if not is_hit(flat[t], hints[32 * t:32 * t + 32])]
            if 0 < len(missing) < len(lanes):
                listed.update(missing)
        out.append((a * NP, b * NP, listed))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every job in one run of the program -> [(n, cut, point set, flat points, kind, in_place, hints, output)]"""
    jobs, blobs = [], []

    def add(n, cut, pset, rows, sets):
        proofs, flat = _proofs(rows), [pt for row in rows for pt in row]
        for kind, make in [(None, None)] + sets:
            for in_place in ((False,) if kind is None else (False, True)):
                hints = None if kind is None else make(flat)
                jobs.append((n, cut, pset, flat, kind, in_place, hints))
                blobs.append(_job(proofs, cut, hints, in_place))

    for n, cut in SHAPES:
        for mixed in (False, True):
            sets = [(kind, functools.partial(lambda flat, kind: hr.hint_set(kind, flat, seed=n), kind=kind)) for kind in hr.HINT_SETS]
            sets += [(kind, functools.partial(lambda flat, kind: _own_set(kind, flat), kind=kind)) for kind in OWN_SETS]
            add(n, cut, "mixed" if mixed else "valid", _points(n, mixed, seed=1000 * n + len(cut) + mixed), sets)
    for cut in ([0, 43], [0, 7, 30, 43]):
        add(43, cut, "bad", _bad_everywhere(seed=77), [(p, functools.partial(lambda flat, p: _pairing_hints(p, flat, seed=5), p=p)) for p in PAIRINGS])
    raw = uh.run(PROG, ["decompress"], uh.words([len(jobs)]) + b"".join(blobs), tmp_path_factory.mktemp("hints_list_units"))
    cur = uh.Cursor(raw)
    out = [job + (_read(cur, job[0]),) for job in jobs]
    cur.done()
    return out


def test_the_unhinted_stage_is_the_reference(results):
    seen = 0
    for n, cut, pset, flat, kind, in_place, hints, (pts, status, miss, count, lst) in results:
        if kind is not None:
            continue
        seen += 1
        assert miss == NEVER and count == NEVER and set(lst) == {NEVER}          # nobody wrote them
        want_status = [0] * n
        for t, pt in enumerate(flat):
            y = decode(pt)
            x, yy, _, phiy, ident, ycanon = pts[t]
            if y is None:
                assert (x, yy, ident, ycanon) == (0, 0, 1, bytes(32)), (n, t)
                want_status[t // NP] = min(want_status[t // NP], ST_TRANSCRIPT if t % NP < N_MAIN else ST_OPENING)
            else:
                b = bytearray(pt); b[31] &= 0x3f
                assert (x, yy, phiy, ident, ycanon) == (int.from_bytes(b, "little"), y, y, 0, hr.le32(y)), (n, t)
        assert status == want_status, (n, cut, pset)
    assert seen == 2 * len(SHAPES) + 2


def test_hints_and_the_list_change_nothing_but_the_miss_word(results):
    plain = {(n, tuple(cut), pset): out for n, cut, pset, flat, kind, in_place, hints, out in results if kind is None}
    seen = set()
    for n, cut, pset, flat, kind, in_place, hints, (pts, status, miss, count, lst) in results:
        if kind is None:
            continue
        where = (n, cut, pset, kind, in_place)
        ref_pts, ref_status = plain[(n, tuple(cut), pset)][:2]
        assert pts == ref_pts, where           # x, y of pts and phi as canonical integers, the identity word, the ycanon bytes
        assert status == ref_status, where
        assert miss == sum(0 if is_hit(pt, hints[32 * t:32 * t + 32]) else 1 for t, pt in enumerate(flat)) == hr.count_misses(flat, hints), where
        seen.add(kind)
    assert seen == set(hr.HINT_SETS) | set(OWN_SETS) | set(PAIRINGS)


def test_the_list_holds_the_misses_of_mixed_waves_each_once(results):
    mixed_jobs = whole_miss_beside_mixed = 0
    for n, cut, pset, flat, kind, in_place, hints, (pts, status, miss, count, lst) in results:
        if kind is None:
            continue
        where = (n, cut, pset, kind, in_place)
        pieces = _expected_list(flat, hints, cut)
        for a, b, want in pieces:
            seg = [t for t in lst[a:b] if t != NEVER]
            assert len(seg) == len(set(seg)), where                # each once
            assert set(seg) == want, where                          # the piece's own misses of mixed waves, in its own segment
            assert lst[a:a + len(seg)] == seg, where                # appended from the segment's start, nothing behind them
        assert count == len(pieces[-1][2]), where                   # the counter as the last piece left it
        listed = set().union(*(p[2] for p in pieces))
        mixed_jobs += bool(listed)
        whole_miss_beside_mixed += bool(listed) and miss > len(listed)
    assert mixed_jobs and whole_miss_beside_mixed                   # both paths were taken, and both in one job


def test_the_sets_are_what_they_are_named_for(results):
    """the reference's own counts, so that the comparisons above cannot pass on a reference that calls everything a miss (or a hit)"""
    for n, cut, pset, flat, kind, in_place, hints, (pts, status, miss, count, lst) in results:
        total, bad = n * NP, sum(1 for pt in flat if decode(pt) is None)
        listed = sum(1 for t in lst if t != NEVER)
        if kind == "right":
            assert miss == bad and listed <= bad          # (an undecodable point alone in a piece's last wave is a whole-miss wave: not listed)
            if pset == "valid":
                assert listed == 0
        elif kind in ("zero", "other_root", "plus_p", "random"):
            assert miss == total and listed == 0                    # whole-miss waves only: roots in place
        elif kind == "lane0_wrong":
            waves = (total + 63) // 64      # of the whole run: lane t of it owns point t, whatever the pieces
            assert bad <= miss <= bad + waves and miss >= (1 if pset == "valid" else 0)
        elif kind == "even_lanes":
            assert miss == sum(1 for t, pt in enumerate(flat) if t % 2 or decode(pt) is None)
        elif kind in ("lane0", "lane63", "last_live") and pset == "valid":
            assert miss == sum(1 for t in range(total) if {"lane0": t % 64 == 0, "lane63": t % 64 == 63, "last_live": t == min(t // 64 * 64 + 63, total - 1)}[kind])
        elif kind == "alt_proofs" and pset == "valid":
            assert miss == NP * (n // 2)
        elif kind in PAIRINGS:
            assert bad == 12 and miss == 64 + 6                     # wave 1 whole, and wave 0's six undecodable points
            if len(cut) == 2:
                assert listed == 6                                  # wave 0 is mixed, wave 1 misses whole, wave 2 hits
