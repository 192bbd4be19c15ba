"""k_decompress_hinted alone (halo2_verifier_amd/csrc/verify_kernels.hip; include/h2v_hints.h), through tests/cpp/hints_units.hip and the
launchers decompress_begin_enqueue / decompress_range_enqueue / decompress_finish_enqueue, on programmed points and hints.

For every shape, point set and hint set: the hinted stage's pts, phi (as field elements), ycanon bytes and status words equal the
unhinted stage's on the same points, the miss word is the count tests/hints_reference.is_hit gives, and the unhinted stage itself
agrees with hints_reference.decode.  Every output lies between guard bands (the harness ends with status 5 on a write past one).

Shapes (Np = 3, one lane per point): n = 1 (three live lanes of one wave), n = 21 (63 lanes), n = 22 (66 lanes: two workgroups, a
ragged end), and n = 22 cut into the pieces [0, 7) [7, 22), whose second piece starts in the middle of a wave of the whole run (the p0
offset of the hints).  Hint sets: hints_reference.HINT_SETS, from a buffer of their own, and the right and the one-miss-per-wave set
also from the ycanon buffer itself, as the batch keeps them.  Point sets: valid points; and the same with a non-residue x, an x >= p
and an identity flag, each at a main-point slot and at an opening slot (n = 1: one of each kind that fits)."""
import random

import pytest

import hints_reference as hr
import units_harness as uh

pytestmark = pytest.mark.gpu

PROG = "hints_units"
NP, N_MAIN, PROOF_LEN, OFFSETS = 3, 2, 128, (0, 64, 96)
ST_TRANSCRIPT, ST_OPENING = -30, -10
SHAPES = [(1, [0, 1]), (21, [0, 21]), (22, [0, 22]), (22, [0, 7, 22])]


def _points(n, mixed, seed):
    """n x NP compressed points; mixed: undecodable ones of every kind at main slots (0, 1) and at the opening slot (2)"""
    rnd = random.Random(seed)
    pts = [[hr.random_point(rnd) for _ in range(NP)] for _ in range(n)]
    if mixed:
        nonres = hr.encode(hr.non_residue_x(rnd.randrange(hr.P // 2)), 1)
        big = hr.encode(hr.P + rnd.randrange(1 << 200), 0)
        ident = hr.encode(0, 0, identity=1)
        if n == 1:
            pts[0][0], pts[0][2] = nonres, ident
        else:
            for k, (proof, slot, bad) in enumerate([(1, 0, nonres), (2, 2, nonres), (3, 1, big), (4, 2, big), (5, 0, ident), (6, 2, ident), (n - 1, 2, nonres), (8, 0, big),
                                                    (8, 2, ident)]):
                pts[proof][slot] = bad
    return pts


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
    return pts, status, cur.word()


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """every job in one run of the program -> [(n, cut, mixed, flat points, kind, in_place, hints, output)]"""
    jobs, blobs = [], []
    for n, cut in SHAPES:
        for mixed in (False, True):
            rows = _points(n, mixed, seed=1000 * n + len(cut) + mixed)
            proofs, flat = _proofs(rows), [pt for row in rows for pt in row]
            sets = [(None, False, None)] + [(kind, False, hr.hint_set(kind, flat, seed=n)) for kind in hr.HINT_SETS]
            sets += [(kind, True, hr.hint_set(kind, flat, seed=n)) for kind in ("right", "lane0_wrong")]
            for kind, in_place, hints in sets:
                jobs.append((n, cut, mixed, flat, kind, in_place, hints))
                blobs.append(_job(proofs, cut, hints, in_place))
    raw = uh.run(PROG, ["decompress"], uh.words([len(jobs)]) + b"".join(blobs), tmp_path_factory.mktemp("hints_units"))
    cur = uh.Cursor(raw)
    out = [job + (_read(cur, job[0]),) for job in jobs]
    cur.done()
    return out


def test_the_unhinted_stage_is_the_reference(results):
    seen = 0
    for n, cut, mixed, flat, kind, in_place, hints, (pts, status, miss) in results:
        if kind is not None:
            continue
        seen += 1
        assert miss == 0xffffffff          # nobody wrote the word
        want_status = [0] * n
        for t, pt in enumerate(flat):
            y = hr.decode(pt)
            x, yy, _, phiy, ident, ycanon = pts[t]
            if y is None:
                assert (x, yy, ident, ycanon) == (0, 0, 1, bytes(32)), (n, t)
                want_status[t // NP] = min(want_status[t // NP], ST_TRANSCRIPT if t % NP < N_MAIN else ST_OPENING)
            else:
                b = bytearray(pt); b[31] &= 0x3f
                assert (x, yy, phiy, ident, ycanon) == (int.from_bytes(b, "little"), y, y, 0, hr.le32(y)), (n, t)
        assert status == want_status, (n, cut, mixed)
    assert seen == 2 * len(SHAPES)


def test_hints_change_nothing_but_the_miss_word(results):
    plain = {(n, tuple(cut), mixed): out for n, cut, mixed, flat, kind, in_place, hints, out in results if kind is None}
    seen = set()
    for n, cut, mixed, flat, kind, in_place, hints, (pts, status, miss) in results:
        if kind is None:
            continue
        where = (n, cut, mixed, kind, in_place)
        ref_pts, ref_status, _ = plain[(n, tuple(cut), mixed)]
        assert pts == ref_pts, where           # x, y of pts and phi as canonical integers, the identity word, the ycanon bytes
        assert status == ref_status, where
        assert miss == hr.count_misses(flat, hints), where
        seen.add(kind)
    assert seen == set(hr.HINT_SETS)


def test_the_miss_counts_are_the_ones_the_sets_are_named_for(results):
    """the reference's own counts, so that the comparison above cannot pass on a reference that calls everything a miss"""
    for n, cut, mixed, flat, kind, in_place, hints, (pts, status, miss) in results:
        bad = sum(1 for pt in flat if hr.decode(pt) is None)
        total = n * NP
        if kind == "right":
            assert miss == bad
        elif kind in ("zero", "other_root", "plus_p", "random"):
            assert miss == total
        elif kind == "lane0_wrong":
            waves = (total + 63) // 64      # of the whole run: lane t of it owns point t, whatever the pieces
            assert bad <= miss <= bad + waves and miss >= (1 if not mixed else 0)
        elif kind == "even_lanes":
            assert miss == sum(1 for t, pt in enumerate(flat) if t % 2 or hr.decode(pt) is None)
