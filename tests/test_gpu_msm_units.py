"""The MSM kernels (csrc/msm.hip) and the device group law (csrc/curve.hip.h) stage by stage, against Python big integers
(tests/msm_reference.py).  build/msm_units (tests/cpp/msm_units.hip, built by csrc/Makefile with the library's flags) runs the
library's own code on scalars, points and bucket layouts chosen here; every comparison is exact.

  digits   msm_glv_prep's digit table and the global sort's counts / offsets / list, for c in 2 .. 12, checked BY DEFINITION: the signed
           digits of the two halves must spell k = k1 + k2 lambda (mod r); scalars whose second half is negative, carries through
           every window, raw == 2^(c-1), windows across 32-bit words
  law      g1_dbl_inl / g1_dbl_quad / g1_madd_fast / g1_add_fast / g1_add_inl / g1_add_affine_inl / g1_phi / msm_entry_apply /
           msm_horner_quad with coordinates stored as m and as m + p, and a chain of 2000 operations
  msm      launches through msm_enqueue_multi: programmed bucket layouts with the control words (heavy, E, straddling, team, redo)
           predicted from the bucket sizes, and every window width a launch of the suite's sizes can select
  scale    k_accumulator_scale behind a slot map
One child process per mode, each under a time limit."""
import functools
import itertools
import random
import struct

import numpy as np
import pytest

import msm_reference as ref
import oracle_lib
from msm_reference import LAMBDA, P, R
from units_harness import words as _words
import units_harness as uh

pytestmark = pytest.mark.gpu

WIDTHS = [2, 3, 4, 5, 6, 7, 10, 11, 12]
ENTRY_HALF, ENTRY_NEG, ENTRY_TERM = 0x40000000, 0x80000000, 0x3fffffff
FIXUP_TEAM, FIXUP_SERIAL, SHORT_LIST = 3, 64, 98304       # msm.hip: MSM_FIXUP_TEAM, MSM_FIXUP_SERIAL, MSM_SHORT_LIST
IDENTITY_WORDS = ref.fq_words(0) + ref.fq_words(1) + ref.fq_words(0)


def _run(mode, blob, tmp_path, timeout=300):
    """the harness on one input file -> its output words"""
    return uh.as_words(uh.run("msm_units", [mode], blob, tmp_path, timeout))


def _scalars(ks):
    return b"".join(int(k).to_bytes(32, "little") for k in ks)


@functools.lru_cache(maxsize=None)
def _pool(count):
    """count points a G, (a + d) G, (a + 2 d) G .. with their logarithms: no small relation between them, so no partial sum of a
    bucket meets another of its points by accident"""
    rnd = random.Random(4242)
    a, d = rnd.randrange(1, R), rnd.randrange(1, R)
    pt, step = ref.mul(a, ref.G), ref.mul(d, ref.G)
    pts, logs = [], []
    for i in range(count):
        pts.append(pt)
        logs.append((a + i * d) % R)
        pt = ref.add(pt, step)
    return pts, logs


# ====================================================================== digits
def _digit_scalars(c):
    """-> scalars, the (index, k1, j) of the negative-half class, the (index, k1, k2) of the width class"""
    ks = list(ref.edge_scalars())
    neg = [(len(ks) + i, k1, j) for i, (_, k1, j) in enumerate(ref.negative_half_scalars())]
    ks += [k for k, _, _ in ref.negative_half_scalars()]
    wid = [(len(ks) + i, k1, k2) for i, (_, k1, k2) in enumerate(ref.width_scalars(c))]
    ks += [k for k, _, _ in ref.width_scalars(c)]
    ks += ref.random_scalars(900 + c)
    return ks, neg, wid


DIGIT_IDENTITY_BASES = (40, 700, 1001)       # terms whose base is the identity (their scalars are not zero)


@pytest.fixture(scope="module")
def digit_runs(tmp_path_factory):
    """one child process: every width's digit table, counts, offsets and list"""
    pts, _ = _pool(64)
    blob, plans = [struct.pack("<I", len(WIDTHS))], {}
    for c in WIDTHS:
        ks, neg, wid = _digit_scalars(c)
        n, windows = len(ks), (130 + c - 1) // c       # msm_plan's window count
        bases = [bytes(64) if t in DIGIT_IDENTITY_BASES else ref.affine_bytes(pts[t % 64]) for t in range(n)]
        assert all(ks[t] for t in DIGIT_IDENTITY_BASES)
        blob += [struct.pack("<III", c, windows, n), _scalars(ks), b"".join(bases)]
        plans[c] = (ks, neg, wid, windows)
    out = _run("digits", b"".join(blob), tmp_path_factory.mktemp("digits"))
    runs, at = {}, 0
    for c in WIDTHS:
        ks, neg, wid, windows = plans[c]
        n = len(ks)
        w_, buckets, nb, E = (int(v) for v in out[at:at + 4])
        assert (w_, buckets, nb) == (windows, 1 << (c - 1), windows << (c - 1))
        at += 4
        dig = out[at:at + windows * n].reshape(windows, n); at += windows * n
        counts = out[at:at + nb + 8]; at += nb + 8
        offsets = out[at:at + nb]; at += nb
        lst = out[at:at + E]; at += E
        runs[c] = dict(ks=ks, neg=neg, wid=wid, windows=windows, buckets=buckets, nb=nb, E=E, dig=dig, counts=counts, offsets=offsets, list=lst)
    assert at == len(out)
    return runs


def _halves_from_table(run, c):
    """per term the two signed halves the digit table spells: sum_w (+/- mag_w) 2^(c w); the largest magnitude; the top window used"""
    dig, n = run["dig"], len(run["ks"])
    halves = [[0, 0] for _ in range(n)]
    max_mag, top = 0, -1
    for w in range(run["windows"]):
        row = dig[w].tolist()
        for t in range(n):
            word = row[t]
            if not word:
                continue
            top = max(top, w)
            for hf in (0, 1):
                d16 = (word >> (16 * hf)) & 0xffff
                mag = d16 & 0x7fff
                if mag:
                    max_mag = max(max_mag, mag)
                    halves[t][hf] += (-mag if d16 & 0x8000 else mag) << (c * w)
    return halves, max_mag, top


@pytest.mark.parametrize("c", WIDTHS)
def test_digit_table_spells_the_scalar(digit_runs, c):
    """sum_w d_w 2^(c w) over half 0 plus lambda times the same over half 1 is k (mod r); every |d_w| <= 2^(c-1); a zero scalar or an
    identity base has all-zero words; the halves are those of exact floors (inside the lattice cell: 0 <= k1 < a1 + a2,
    -a2 < k2 < b2); the width class decomposes to itself, so that its digit patterns — a carry through every window,
    raw == 2^(c-1) exactly — are the ones the recoding really saw"""
    run = digit_runs[c]
    ks = run["ks"]
    halves, max_mag, top = _halves_from_table(run, c)
    assert max_mag <= 1 << (c - 1)
    assert max_mag == 1 << (c - 1), "no digit reached 2^(c-1): the class meant to produce it did not"
    for t, k in enumerate(ks):
        if k == 0 or t in DIGIT_IDENTITY_BASES:
            assert not run["dig"][:, t].any(), t
            continue
        k1, k2 = halves[t]
        assert (k1 + k2 * LAMBDA - k) % R == 0, (c, t, hex(k), k1, k2)
        assert ref.in_cell(k1, k2), (c, t, hex(k), k1, k2)
    assert len(run["wid"]) == 16
    for t, k1, k2 in run["wid"]:
        assert tuple(halves[t]) == (k1, k2), (c, t)
    # the top window any term uses: bit c * top + (c - 1) at the most — what the plan's window count has to cover
    print(f"c={c}: windows={run['windows']} top window used={top} negative second halves={sum(1 for h in halves if h[1] < 0)}")
    assert top < run["windows"]
    assert top >= 126 // c, "no magnitude of 127 bits among the classes"


@pytest.mark.parametrize("c", WIDTHS)
def test_sorted_list_spells_the_same_digits(digit_runs, c):
    """the global sort's list: entry sign, half flag and bucket index + 1 stand for the digit; counts and offsets agree with the list"""
    run = digit_runs[c]
    n, nb, buckets, E = len(run["ks"]), run["nb"], run["buckets"], run["E"]
    counts, offsets, lst = run["counts"].tolist(), run["offsets"].tolist(), run["list"].tolist()
    assert counts[nb + 1] == E == sum(counts[:nb])
    halves = [[0, 0] for _ in range(n)]
    seen = set()
    at = 0
    for b in range(nb):
        assert offsets[b] == at, b
        w, mag = divmod(b, buckets)
        mag += 1
        for e in lst[at:at + counts[b]]:
            t, hf = e & ENTRY_TERM, 1 if e & ENTRY_HALF else 0
            assert t < n and (t, hf, w) not in seen, (b, hex(e))
            seen.add((t, hf, w))
            halves[t][hf] += (-mag if e & ENTRY_NEG else mag) << (c * w)
        at += counts[b]
    want, _, _ = _halves_from_table(run, c)
    assert halves == want


def test_negative_half_class_is_negative(digit_runs):
    """k = (k1 - j lambda) mod r for k1 in {2^126, 2^126 - 1, 2^126 + 2^64, a1 - 1} and j in {1, 2, 3, 2^20, 2^62} is split into exactly
    (k1, -j), at every width: glv_finish's negation and the entry sign `neg_digit != h.neg` have run (the table and the list are
    compared above).  Before glv_decompose corrected its approximate quotients to exact floors only 9 of the 20 came out this way —
    j <= 2, and j = 3 at k1 = a1 - 1 — and the other 11 as (k1 + a2, b2 - j), outside the lattice cell."""
    for c in WIDTHS:
        run = digit_runs[c]
        halves, _, _ = _halves_from_table(run, c)
        print(f"c={c}: negative-half class: {sum(1 for t, _, _ in run['neg'] if halves[t][1] < 0)} of {len(run['neg'])} second halves negative")
        bad = [(hex(k1), j) for t, k1, j in run["neg"] if tuple(halves[t]) != (k1, -j)]
        assert not bad, f"c={c}: not split into (k1, -j): {bad}"


# ====================================================================== group law
OP_DBL, OP_DBL_QUAD, OP_MADD_FAST, OP_ADD_FAST, OP_ADD, OP_ADD_AFFINE, OP_PHI, OP_ENTRY_APPLY, OP_HORNER = range(9)
REPS3 = list(itertools.product((False, True), repeat=3))
ZERO27 = [0] * 27


def _jac_variants(pt, rnd):
    """the stored forms of a point: Z = 1 and a random Z, every coordinate as m or as m + p.  The identity: (0, 1, 0), a random (X, Y)
    over Z = 0, and Z stored as p — Fp::is_zero accepts the limb string p as zero ([0, 2p) representatives), so G1J::is_identity does"""
    if pt is None:
        x, y = rnd.randrange(P), rnd.randrange(P)
        return [ref.jac_words(None, reps=r) for r in REPS3] + [ref.fq_words(x, r[0]) + ref.fq_words(y, r[1]) + ref.fq_words(0, r[2]) for r in REPS3]
    return [ref.jac_words(pt, z, r) for z in (1, rnd.randrange(2, P)) for r in REPS3]


def _aff_variants(pt):
    if pt is None:
        return [ref.fq_words(0, a) + ref.fq_words(0, b) + [0] * 9 for a in (False, True) for b in (False, True)]
    return [ref.fq_words(pt[0], a) + ref.fq_words(pt[1], b) + [0] * 9 for a in (False, True) for b in (False, True)]


def _in_range(words27, coords=3):
    return all(ref.fq_in_range(words27[9 * i:9 * i + 9]) for i in range(coords))


def _law_inputs():
    rnd = random.Random(77)
    logs = [1, 2, 3, 5, rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)]
    pts = {k: ref.mul(k, ref.G) for k in logs}
    pairs = [(1, 2), (2, 1), (3, 5), (logs[4], logs[5]), (logs[6], 1), (5, logs[4])]           # P + Q
    pairs += [(1, 1), (3, 3), (logs[4], logs[4]), (logs[5], logs[5])]                            # P + P
    pairs += [(1, R - 1), (5, R - 5), (logs[6], R - logs[6])]                                    # P + (-P)
    pairs += [(2, 0), (0, 2), (logs[5], 0), (0, logs[5]), (0, 0)]                                # the identity on either side
    for k in list(pts):
        pts[R - k] = ref.neg(pts[k])
    pts[0] = None
    cases, meta = [], []          # meta: (op, P, Q, words of A, extra)

    def case(op, A, B, a0=0, a1=0, a2=0, **m):
        cases.append([op, a0, a1, a2] + A + B)
        meta.append(dict(op=op, A=A, B=B, **m))

    for ka, kb in pairs:
        pa, pb = pts[ka], pts[kb]
        va, vb, vaff = _jac_variants(pa, rnd), _jac_variants(pb, rnd), _aff_variants(pb)
        for i, A in enumerate(va):
            case(OP_ADD_FAST, A, vb[(5 * i + 3) % len(vb)], p=pa, q=pb)
            case(OP_ADD, A, vb[(5 * i + 7) % len(vb)], p=pa, q=pb)
            case(OP_MADD_FAST, A, vaff[i % 4], p=pa, q=pb)
            case(OP_ADD_AFFINE, A, vaff[(i + 1) % 4], p=pa, q=pb)
    for k in logs + [0]:
        for A in _jac_variants(pts[k], rnd):
            case(OP_DBL, A, ZERO27, p=pts[k])
            case(OP_DBL_QUAD, A, ZERO27, p=pts[k])
        for B in _aff_variants(pts[k]):
            case(OP_PHI, ZERO27, B, p=pts[k])
            for e in (0, ENTRY_HALF, ENTRY_NEG, ENTRY_HALF | ENTRY_NEG):
                for have_phi in (0, 1):
                    case(OP_ENTRY_APPLY, ZERO27, B, a0=e | 12345, a1=have_phi, p=pts[k], e=e, have_phi=have_phi)
    # Horner over pool slices: items weigh 2^(dbl i); identities among them, the plan's (windows, c) shapes
    pool_pts = []
    horner = [(1, 7), (3, 7), (19, 7), (65, 2), (44, 3), (11, 12)]
    for items, dblc in horner:
        first = len(pool_pts)
        for i in range(items):
            pool_pts.append(None if i % 5 == 3 else ref.mul(rnd.randrange(R), ref.G))
        case(OP_HORNER, ZERO27, ZERO27, a0=first, a1=items, a2=dblc, items=pool_pts[first:first + items], dbl=dblc)
    return cases, meta, pool_pts, rnd


def _chain(pool_pts, rnd):
    """2000 operations, each on the previous result: blocks that meet the same point and its negative (the fast forms refuse, the complete
    ones double or cancel; every block ends at the identity), then a random mixture.  -> pool words, ops, the expected point and refusals"""
    base = len(pool_pts)
    extra, ops = [], []
    acc, refused = None, 0
    n_blocks = 40
    for b in range(n_blocks):
        pt = ref.mul(rnd.randrange(R), ref.G)
        i = base + len(extra)
        extra += [pt, ref.neg(ref.dbl(pt))]
        # acc = identity: take P; P again: refused; complete: 2P; -2P: refused; complete: identity
        ops += [(OP_MADD_FAST, i), (OP_MADD_FAST if b % 2 else OP_ADD_FAST, i), (OP_ADD_AFFINE if b % 2 else OP_ADD, i),
                (OP_ADD_FAST if b % 2 else OP_MADD_FAST, i + 1), (OP_ADD if b % 2 else OP_ADD_AFFINE, i + 1)]
        refused += 2
    all_pts = pool_pts + extra
    live = [i for i, p in enumerate(all_pts)]
    while len(ops) < 2000:
        op = rnd.choice([OP_DBL, OP_DBL_QUAD, OP_MADD_FAST, OP_ADD_FAST, OP_ADD, OP_ADD_AFFINE])
        ops.append((op, rnd.choice(live)))
    for op, i in ops[5 * n_blocks:]:
        nxt = ref.dbl(acc) if op in (OP_DBL, OP_DBL_QUAD) else ref.add(acc, all_pts[i])
        if op in (OP_MADD_FAST, OP_ADD_FAST) and acc is not None and all_pts[i] is not None and acc[0] == all_pts[i][0]:
            refused += 1        # (no random step gets here; the rule is the same)
            continue
        acc = nxt
    # pool words: affine operands read (X, Y) of the slot, so every slot keeps Z = 1; representatives vary
    words = []
    for i, pt in enumerate(all_pts):
        reps = REPS3[i % 8]
        words.append(ref.jac_words(pt, 1, reps) if pt is not None else ref.fq_words(0, reps[0]) + ref.fq_words(0, reps[1]) + ref.fq_words(0, reps[2]))
    return words, ops, acc, refused


@pytest.fixture(scope="module")
def law_run(tmp_path_factory):
    cases, meta, pool_pts, rnd = _law_inputs()
    pool_words, ops, chain_pt, chain_refused = _chain(pool_pts, rnd)
    blob = [struct.pack("<I", len(pool_words))] + [_words(w) for w in pool_words]
    blob += [struct.pack("<I", len(cases))] + [_words(c) for c in cases]
    blob += [struct.pack("<I", len(ops)), _words(IDENTITY_WORDS), _words([v for o in ops for v in o])]
    out = _run("law", b"".join(blob), tmp_path_factory.mktemp("law")).reshape(len(cases) + 1, 112)
    return meta, out, chain_pt, chain_refused


def _lanes(rec):
    return [rec[4 + 27 * r:31 + 27 * r].tolist() for r in range(4)]


def test_fast_additions_refuse_exactly_when_x_agrees(law_run):
    """g1_madd_fast / g1_add_fast return false exactly when both operands are points with the same x — in whichever representatives
    and whatever Z — and then leave the accumulator's limbs untouched; otherwise the accumulator is the sum, below 2p, limbs below 2^29"""
    meta, out, _, _ = law_run
    seen = {True: 0, False: 0}
    for m, rec in zip(meta, out):
        if m["op"] not in (OP_MADD_FAST, OP_ADD_FAST):
            continue
        lanes = _lanes(rec)
        agree = m["p"] is not None and m["q"] is not None and m["p"][0] == m["q"][0]
        assert int(rec[0]) == (0 if agree else 1), m
        seen[agree] += 1
        assert all(l == lanes[0] for l in lanes)
        if agree:
            assert lanes[0] == m["A"]
        else:
            assert ref.jac_point(lanes[0]) == ref.add(m["p"], m["q"]), m
            assert _in_range(lanes[0])
    assert seen[True] > 100 and seen[False] > 100


def test_complete_additions_give_the_sum(law_run):
    meta, out, _, _ = law_run
    kinds = set()
    for m, rec in zip(meta, out):
        if m["op"] not in (OP_ADD, OP_ADD_AFFINE):
            continue
        lanes = _lanes(rec)
        assert all(l == lanes[0] for l in lanes)
        want = ref.add(m["p"], m["q"])
        assert ref.jac_point(lanes[0]) == want, m
        assert _in_range(lanes[0])
        kinds.add("id" if want is None else ("dbl" if m["p"] == m["q"] else "add"))
    assert kinds == {"id", "dbl", "add"}


def test_doublings_agree_lane_for_lane(law_run):
    """g1_dbl_quad's four lanes agree limb for limb with each other and — for a point — with g1_dbl_inl.  (For an identity operand
    g1_dbl_inl returns its input as it is while the quad computes Z3 = 2 Y Z = 0: both are the identity, not the same limbs.)"""
    meta, out, _, _ = law_run
    inl = {}
    for m, rec in zip(meta, out):
        if m["op"] == OP_DBL:
            lanes = _lanes(rec)
            assert ref.jac_point(lanes[0]) == ref.dbl(m["p"]) and _in_range(lanes[0])
            inl[tuple(m["A"])] = lanes[0]
    n = 0
    for m, rec in zip(meta, out):
        if m["op"] != OP_DBL_QUAD:
            continue
        lanes = _lanes(rec)
        assert all(l == lanes[0] for l in lanes), m
        assert ref.jac_point(lanes[0]) == ref.dbl(m["p"]) and _in_range(lanes[0])
        if m["p"] is not None:
            assert lanes[0] == inl[tuple(m["A"])], m
            n += 1
    assert n >= 7 * 16


def test_phi_entry_apply_and_horner(law_run):
    meta, out, _, _ = law_run
    for m, rec in zip(meta, out):
        lane = _lanes(rec)[0]
        x, y = ref.fq_value(lane[0:9]), ref.fq_value(lane[9:18])
        p = m.get("p")
        if m["op"] == OP_PHI:
            assert (x, y) == ((ref.BETA * p[0] % P, p[1]) if p else (0, 0)) and _in_range(lane, 2)
        elif m["op"] == OP_ENTRY_APPLY:
            want = p if p else (0, 0)
            if m["e"] & ENTRY_HALF and not m["have_phi"]:
                want = (ref.BETA * want[0] % P, want[1])
            if m["e"] & ENTRY_NEG:
                want = (want[0], -want[1] % P)
            assert (x, y) == want, m
            assert _in_range(lane, 2), m                      # 2p - y stays below 2p for y stored as m and as m + p
            if p is None:
                assert all(ref.from_limbs(lane[9 * i:9 * i + 9]) in (0, P) for i in (0, 1))      # the identity is still recognised
        elif m["op"] == OP_HORNER:
            want = None
            for i, pt in enumerate(m["items"]):
                want = ref.add(want, ref.mul(1 << (m["dbl"] * i), pt))
            assert all(ref.jac_point(l) == want for l in _lanes(rec)), (len(m["items"]), m["dbl"])
            assert _in_range(lane)


def test_chain_of_2000_operations(law_run):
    _, out, chain_pt, chain_refused = law_run
    lanes = _lanes(out[-1])
    assert int(out[-1][0]) == chain_refused
    assert all(l == lanes[0] for l in lanes)
    assert ref.jac_point(lanes[0]) == chain_pt
    assert _in_range(lanes[0])


# ====================================================================== launches
def _msm_blob(jobs):
    """jobs: [(tuning dict, [(scalars, base bytes, n1, phi)])]"""
    blob = [struct.pack("<I", len(jobs))]
    for tune, problems in jobs:
        blob.append(struct.pack("<6I", tune.get("msm_global_sort", 0), tune.get("msm_no_term_split", 0), tune.get("msm_window_threads", 0),
                                tune.get("msm_window_wpw", 0), tune.get("msm_window_slots", 0), len(problems)))
        for ks, bases, n1, phi in problems:
            assert len(ks) == len(bases)
            blob += [struct.pack("<III", len(ks), len(ks) if n1 is None else n1, phi), _scalars(ks), b"".join(bases)]
    return b"".join(blob)


def _msm_parse(out, jobs):
    res, at = [], 0
    for _, problems in jobs:
        c, windows, buckets, launched, cut, ch = (int(v) for v in out[at:at + 6])
        control = [int(v) for v in out[at + 6:at + 14]]
        at += 14
        pts = []
        for _ in problems:
            w = out[at:at + 27].tolist()
            assert _in_range(w)
            pts.append(ref.jac_point(w))
            at += 27
        res.append(dict(c=c, windows=windows, buckets=buckets, launched=launched, cut=cut, ch=ch, heavy=control[0], E=control[1],
                        straddling=control[2], team=control[3], redo=control[4], points=pts))
    assert at == len(out)
    return res


def _small_digits(k, c):
    """the (window, bucket, negated) entries of a scalar below 2^c - 1, by definition of the signed recoding: k itself up to 2^(c-1),
    else k - 2^c in window 0 and the carry 1 in window 1.  (Such a scalar is its own first GLV half: k < a2.)"""
    half = 1 << (c - 1)
    assert 1 <= k < (1 << c) - 1
    return [(0, k - 1, False)] if k <= half else [(0, (1 << c) - k - 1, True), (1, 0, False)]


def _control_from_sizes(sizes, ch):
    """msm_chunk_tail's rule on the dense list: a bucket [lo, hi) that begins in chunk lo // ch and runs on past it into `span` further
    chunks is listed as heavy (span >= 64), for a team (span >= 3), else as straddling.  sizes: bucket sizes in bin order"""
    heavy = team = strad = 0
    spans, starts, lo = set(), set(), 0
    for s in sizes:
        if s:
            hi, i0 = lo + s, lo // ch
            span = (hi - 1) // ch - i0
            starts.add(lo % ch == 0)
            if span:
                spans.add(span)
                if span >= FIXUP_SERIAL:
                    heavy += 1
                elif span >= FIXUP_TEAM:
                    team += 1
                else:
                    strad += 1
            lo = hi
    return dict(heavy=heavy, team=team, straddling=strad, E=lo), spans, starts


def _bin_sizes(problems_ks, c, windows):
    """bucket sizes in bin order (problem, window, bucket) for problems of small scalars"""
    buckets = 1 << (c - 1)
    sizes = [0] * (len(problems_ks) * windows * buckets)
    for q, ks in enumerate(problems_ks):
        for k in ks:
            for w, b, _ in _small_digits(k, c):
                sizes[(q * windows + w) * buckets + b] += 1
    return sizes


def _programmed_layout():
    """one problem at c = 7, chunk length 4: bucket b of window 0 holds the terms with scalar b + 1.  Buckets that begin on and off a chunk
    boundary and run into exactly 1, 2, 3, 4, 63, 64 and 65 further chunks; a point that meets itself inside a chunk, a point and its
    negative inside a chunk, the same point in two chunks of one bucket; scalars above 64 (a negative digit and a carry into window 1).
    -> scalars, base indices (negative: the negated point), the chunks to redo"""
    sizes, special, at = [], {}, 0

    def bucket(size, tag=None):
        nonlocal at
        if tag:
            special[tag] = (len(sizes), at)
        sizes.append(size)
        at += size

    def align(mod):
        if at % 4 != mod:
            bucket((mod - at) % 4)

    for span in (1, 2, 3, 4, 63, 64, 65):
        for mod in (0, 3 if span % 2 else 1):
            align(mod)
            bucket(4 * span - mod + 1 + (span % 3 if mod == 0 else 0))      # ends in the first .. third slot of its last chunk
    align(0); bucket(2, "twice")            # P, P inside one chunk
    align(0); bucket(1); bucket(2, "opposite")     # P, -P inside one chunk, off the boundary
    align(3); bucket(2, "split")            # P | P on either side of a chunk boundary
    assert len(sizes) <= 58
    ks, bases, nxt = [], [], 0
    for b, s in enumerate(sizes):
        tag = next((t for t, (bb, _) in special.items() if bb == b), None)
        for i in range(s):
            ks.append(b + 1)
            if tag and i == 1:
                bases.append(-(nxt - 1) - 1 if tag == "opposite" else nxt - 1)     # the previous term's point again, or its negative
            else:
                bases.append(nxt); nxt += 1
    for k in (65, 66, 66, 67, 67, 67, 69):       # negative digits with a carry, in buckets behind the programmed ones (64 is the last positive digit)
        ks.append(k); bases.append(nxt); nxt += 1
    redo = {special["twice"][1] // 4, special["opposite"][1] // 4}
    assert len(redo) == 2 and special["split"][1] % 4 == 3
    return ks, bases, len(redo)


def _layout_problem(ks, base_idx, pts, logs):
    bases = [ref.affine_bytes(pts[i] if i >= 0 else ref.neg(pts[-i - 1])) for i in base_idx]
    lg = [logs[i] if i >= 0 else -logs[-i - 1] for i in base_idx]
    return bases, ref.msm_by_logs(ks, lg)


@pytest.fixture(scope="module")
def layout_runs(tmp_path_factory):
    pts, logs = _pool(4096)
    cases = {}
    # 1. the programmed layout
    ks, idx, redo = _programmed_layout()
    bases, want = _layout_problem(ks, idx, pts, logs)
    cases["programmed"] = dict(ks=[ks], bases=[bases], want=[want], redo=redo, c=7, ch=4)
    # 2. 300 equal scalars: one bucket of 300 entries in window 0 (negated) and one in window 1 (the carry)
    ks = [100] * 300
    bases, want = _layout_problem(ks, list(range(300)), pts, logs)
    cases["equal"] = dict(ks=[ks], bases=[bases], want=[want], redo=0, c=7, ch=4)
    # 3. E just above 98 304: 49 200 terms of two entries each; the problem is cut into four of 12 300 (c = 11), chunks of 16.  Copies of a base
    #    (index i mod 4096) carry different scalars, so they never share a bucket
    n = 49200
    ks = [1025 + (i % 1022) for i in range(n)]
    idx = [i % 4096 for i in range(n)]
    bases, want = _layout_problem(ks, idx, pts, logs)
    cases["long"] = dict(ks=[ks[i:i + 12300] for i in range(0, n, 12300)], bases=[bases], want=[want], redo=0, c=11, ch=16, flat=[ks])
    jobs = []
    for name, cs in cases.items():
        flat = cs.get("flat", cs["ks"])
        for sort in (0, 1):
            jobs.append(({"msm_global_sort": sort}, [(k, b, None, 0) for k, b in zip(flat, cs["bases"])]))
    res = _msm_parse(_run("msm", _msm_blob(jobs), tmp_path_factory.mktemp("layouts")), jobs)
    return cases, {(name, sort): res[2 * i + sort] for i, name in enumerate(cases) for sort in (0, 1)}


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("name", ["programmed", "equal", "long"])
def test_bucket_layouts_and_control_words(layout_runs, name, sort):
    """the result equals the reference, and the control words equal what msm_chunk_tail's rule gives for the bucket sizes — computed here
    from the scalars, not read from the device"""
    cases, res = layout_runs
    cs, got = cases[name], res[(name, sort)]
    print(name, "global sort" if sort else "LDS sort", {k: got[k] for k in ("c", "windows", "launched", "cut", "ch", "heavy", "E", "straddling", "team", "redo")})
    assert got["points"] == cs["want"]
    assert (got["c"], got["ch"]) == (cs["c"], cs["ch"]) and got["launched"] == len(cs["ks"])
    want, spans, starts = _control_from_sizes(_bin_sizes(cs["ks"], got["c"], got["windows"]), got["ch"])
    assert {k: got[k] for k in want} == want
    assert got["redo"] == cs["redo"]
    if name == "programmed":
        assert spans >= {1, 2, 3, 4, 63, 64, 65} and starts == {True, False}
    if name == "long":
        assert got["E"] > SHORT_LIST and got["cut"] == 1


def test_every_fixup_path_was_taken(layout_runs):
    """each of the heavy, team, lane (straddling) and redo counts is non-zero in at least one case, under both sorts"""
    _, res = layout_runs
    for sort in (0, 1):
        for word in ("heavy", "team", "straddling", "redo"):
            assert any(r[word] for (name, s), r in res.items() if s == sort), (word, sort)


# ---------------------------------------------------------------------- window widths
WIDTH_SHAPES = [(2, 180, 26), (3, 60, 98), (4, 20, 297), (5, 5, 1079), (6, 3, 1587), (7, 1, 1000), (10, 3, 1588), (11, 1, 8006), (12, 1, 14569)]


def _width_problems(c, count, n, bases_pool):
    """the edge, negative-half and width-c scalars dealt over the problems, random ones for the rest; every problem has an identity base
    and a zero scalar"""
    rnd = random.Random(5000 + c)
    edge = ref.edge_scalars() + [k for k, _, _ in ref.negative_half_scalars()] + [k for k, _, _ in ref.width_scalars(c)]
    rnd.shuffle(edge)
    per = min(n - 2, (len(edge) + count - 1) // count)
    problems = []
    for q in range(count):
        ks = edge[q * per:(q + 1) * per]
        ks += [rnd.randrange(R) for _ in range(n - len(ks))]
        rnd.shuffle(ks)
        bases = [bases_pool[rnd.randrange(len(bases_pool))] for _ in range(n)]
        ks[rnd.randrange(n)] = 0
        bases[next(i for i in range(n) if ks[i])] = bytes(64)
        problems.append((ks, bases, None, 0))
    return problems


@pytest.fixture(scope="module")
def width_runs(tmp_path_factory, srs, oracle):
    from srs_util import g1_xy
    pool = [g1_xy(p) for p in srs.g]
    jobs, want = [], []
    for c, count, n in WIDTH_SHAPES:
        problems = _width_problems(c, count, n, pool)
        exp = [oracle_lib.g1_msm(oracle, ks, bases) for ks, bases, _, _ in problems]
        for sort in (0, 1):
            jobs.append(({"msm_global_sort": sort}, problems))
            want.append(exp)
    # two segments: n = 12 with n1 = 5; a cut problem of 16 390 terms whose segment boundary (8200) falls inside the second sub-problem
    rnd = random.Random(61)
    for n, n1, phis in ((12, 5, (0,)), (16390, 8200, (0, 1))):
        ks = [rnd.randrange(R) for _ in range(n)]
        edge = [k for k, _, _ in ref.negative_half_scalars()] + ref.edge_scalars()[:10]
        for i, k in enumerate(edge[:n - 2]):
            ks[(i * 7919) % n] = k
        bases = [pool[rnd.randrange(len(pool))] for _ in range(n)]
        ks[3], bases[n1] = 0, bytes(64)
        exp = [oracle_lib.g1_msm(oracle, ks, bases)]
        for phi in phis:
            jobs.append(({}, [(ks, bases, n1, phi)]))
            want.append(exp)
    res = _msm_parse(_run("msm", _msm_blob(jobs), tmp_path_factory.mktemp("widths")), jobs)
    return res, want


def _xy(pt):
    return ref.affine_bytes(pt)


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("i", range(len(WIDTH_SHAPES)))
def test_every_window_width_in_a_launch(width_runs, i, sort):
    res, want = width_runs
    c, count, n = WIDTH_SHAPES[i]
    got = res[2 * i + sort]
    assert got["c"] == c, (got["c"], c, count, n)
    assert [_xy(p) for p in got["points"]] == want[2 * i + sort]


@pytest.mark.parametrize("j", range(3))
def test_two_segment_problems(width_runs, j):
    """n = 12 with n1 = 5; n = 16 390 with n1 = 8200, cut in two, without and with the caller's own phi(P)"""
    res, want = width_runs
    got, exp = res[2 * len(WIDTH_SHAPES) + j], want[2 * len(WIDTH_SHAPES) + j]
    assert got["cut"] == (0 if j == 0 else 1) and got["launched"] == (1 if j == 0 else 2)
    assert [_xy(p) for p in got["points"]] == exp


# ====================================================================== scale
def test_accumulator_scale_behind_a_slot_map(tmp_path):
    """k_accumulator_scale: record i = M_i (L, R) of the pair at slots[i].  J = 5 items behind a slot map that is not the identity map, then
    the whole negative-half class and more edge scalars; pairs with random Z, with the left point the identity, with both"""
    rnd = random.Random(31)
    pts, _ = _pool(64)
    pairs = [(pts[1], pts[2]), (None, pts[3]), (None, None), (pts[4], pts[5]), (pts[6], ref.neg(pts[6]))]
    pair_words = []
    for i, (l, r) in enumerate(pairs):
        for pt in (l, r):
            pair_words += ref.jac_words(pt, rnd.randrange(2, P), REPS3[(3 * i + 1) % 8]) if pt else ref.jac_words(None)
    neg = [k for k, _, _ in ref.negative_half_scalars()]
    edge = [0, 1, 2, R - 1, R - 2, LAMBDA, LAMBDA + 1, LAMBDA - 1, R - LAMBDA, LAMBDA * LAMBDA % R, (1 << 253) % R, R - (1 << 128), (1 << 128) - 1]
    jobs = [([4, 2, 0, 3, 1], [neg[0], R - 1, neg[5], LAMBDA, rnd.randrange(R)])]
    more = neg + edge + [k for k, _, _ in ref.width_scalars(4)] + ref.random_scalars(17, 8)
    jobs.append(([(3 * i + 1) % 5 for i in range(len(more))], more))
    blob = [struct.pack("<I", len(jobs))]
    for slots, ks in jobs:
        blob += [struct.pack("<II", len(ks), len(pairs)), _words(pair_words), _words(slots), _scalars(ks)]
    out = _run("scale", b"".join(blob), tmp_path)
    at = 0
    for slots, ks in jobs:
        words = int(out[at]); at += 1
        assert words == 4 + 2 * 6 * 27
        for slot, k in zip(slots, ks):
            rec = out[at:at + words].tolist(); at += words
            assert rec[0:4] == [0, 1, 0, 0], rec[0:4]                 # failed, parts, shift, reserved
            for side in (0, 1):
                pieces = [rec[4 + 27 * (6 * side + j):4 + 27 * (6 * side + j + 1)] for j in range(6)]
                assert ref.jac_point(pieces[0]) == ref.mul(k, pairs[slot][side]), (slot, side, hex(k))
                assert _in_range(pieces[0])
                assert all(p == IDENTITY_WORDS for p in pieces[1:])
    assert at == len(out)
