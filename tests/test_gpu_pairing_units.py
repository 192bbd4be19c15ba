"""The pairing kernels' device arithmetic (halo2_verifier_amd/csrc/pairing.hip) against big integers, at adversarial representatives.

build/pairing_units (tests/cpp/pairing_units.hip, built by csrc/Makefile with the library's flags) runs the real pair_step6,
pair_coefficients6 / coef_form, pair_in_fq_star6, k_pair_lines and both check entry points on raw 29-bit limbs chosen here:
Montgomery representatives v 2^261 mod p or that plus p (below 2p, the contract every stored form and line coordinate keeps).
  * step: SQR / MUL / MULL / CONJ / CONJ0 / COPY / FROB1..4, aliased operands and in-place coefficient operations, in k_pairing's
    layout and as column B of k_pairing2's.  Every stored form of the destination must be exactly the limbs of m or of m + p, m the
    Montgomery form of what that form holds (c0, c1, -c1, 9 c0 - c1, 9 c1 + c0, -(9 c1 + c0)) of the flat Fq12 result: the residue, the
    six-form identities, limbs below 2^29 and every form below 2p in one comparison.
  * check: pair_in_fq_star6 on crafted registers.
  * lines: k_pair_lines' merged iteration products against the products of the sparse line values.
  * verdict: the split checks (k_pairing2 and one stream) and the whole-point check against pyref.pairing_check of the folded points.
Each mode runs once, in a child process under a time limit."""
import random

import numpy as np
import pytest

import pairing_reference as pr
import units_harness as uh

pytestmark = pytest.mark.gpu

P = pr.P
MASK = (1 << 29) - 1
EDGE = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]
CASES_PER_CLASS = 20000
OP_CLASSES = [pr.P_SQR, pr.P_MUL, pr.P_MULL, pr.P_CONJ, pr.P_CONJ0, pr.P_COPY, pr.P_FROB, pr.P_FROB2, pr.P_FROB3, pr.P_FROB4]
OP_NAME = {pr.P_SQR: "SQR", pr.P_MUL: "MUL", pr.P_MULL: "MULL", pr.P_CONJ: "CONJ", pr.P_CONJ0: "CONJ0", pr.P_COPY: "COPY",
           pr.P_FROB: "FROB1", pr.P_FROB2: "FROB2", pr.P_FROB3: "FROB3", pr.P_FROB4: "FROB4"}
FORM_NAME = ["c0", "c1", "-c1", "9c0-c1", "9c1+c0", "-(9c1+c0)"]


def _run(args, timeout):
    uh.run("pairing_units", args, timeout=timeout)


def limbs_np(vals):
    """integers below 2^261 -> (n, 9) uint32 limbs of 29 bits"""
    wd = np.frombuffer(b"".join(int(v).to_bytes(40, "little") for v in vals), dtype="<u8").reshape(-1, 5)
    out = np.empty((len(vals), 9), np.uint32)
    for l in range(9):
        w, o = (29 * l) // 64, (29 * l) % 64
        x = wd[:, w] >> np.uint64(o)
        if o + 29 > 64:
            x = x | (wd[:, w + 1] << np.uint64(64 - o))
        out[:, l] = (x & np.uint64(MASK)).astype(np.uint32)
    return out


P_LIMBS = np.array(pr.limbs(P), np.int64)


def plus_p(lm):
    """limbs of x -> limbs of x + p (x + p below 2^261)"""
    out = lm.astype(np.int64) + P_LIMBS
    for l in range(8):
        out[..., l + 1] += out[..., l] >> 29
        out[..., l] &= MASK
    return out.astype(np.uint32)


def forms(c0, c1):
    """the six residues a register keeps of c0 + c1 u"""
    f4 = (9 * c1 + c0) % P
    return [c0 % P, c1 % P, (-c1) % P, (9 * c0 - c1) % P, f4, (-f4) % P]


def rep(v, high):
    m = pr.to_mont(v)
    return m + P if high else m


def reg_words(coefs, rnd, high=None):
    """six (c0, c1) residues -> the 324 representatives of a six-form register (high: all m + p; None: each at random)"""
    return [rep(f, rnd.random() < 0.5 if high is None else high) for c0, c1 in coefs for f in forms(c0, c1)]


def fq2_words(coefs, rnd, high=None):
    return [rep(x, rnd.random() < 0.5 if high is None else high) for c in coefs for x in c]


def _pool_coefs(rnd, edge):
    return [tuple(rnd.choice(EDGE) if edge else rnd.randrange(P) for _ in range(2)) for _ in range(6)]


def test_step_matches_flat_arithmetic(tmp_path):
    rnd = random.Random(2024)
    NPOOL, NLINE = 1024, 512
    pool, pool_words = [], []
    for i in range(NPOOL):
        edge = i >= NPOOL // 2
        coefs = _pool_coefs(rnd, edge)
        if i == NPOOL // 2: coefs = [(0, 0)] * 6                 # zero: every form stored as the limb string p
        if i == NPOOL // 2 + 1: coefs = [(1, 0)] + [(0, 0)] * 5
        pool.append(pr.reg_to_flat(coefs))
        pool_words += reg_words(coefs, rnd, high=(True if edge and i % 2 == 0 else None))
    lines, line_words = [], []
    for i in range(NLINE):
        edge = i >= NLINE // 2
        coefs = _pool_coefs(rnd, edge)
        lines.append(pr.reg_to_flat(coefs))
        line_words += fq2_words(coefs, rnd, high=(True if edge and i % 2 == 0 else None))
    cases = []   # (op word, pool a, pool b, line, column)
    for op in OP_CLASSES:
        for n in range(CASES_PER_CLASS):
            half = NPOOL // 2 if n % 2 else 0              # half the cases from the random pool, half from the edge pool
            pa, pb = half + rnd.randrange(NPOOL // 2), half + rnd.randrange(NPOOL // 2)
            a = rnd.randrange(2)
            if op == pr.P_MUL: d, b = 2, rnd.choice([0, 1, a])   # b = a: both factors the same register
            else: d, b = (rnd.choice([a, 2]) if op in (pr.P_CONJ, pr.P_CONJ0, pr.P_COPY) else 2), 0   # in place where the kernels allow it
            cases.append((op | (d << 8) | (a << 16) | (b << 24), pa, pb, half // 2 + rnd.randrange(NLINE // 2), 1 if n % 8 == 7 else 0))
    cases.sort(key=lambda c: c[4])
    n_b = sum(c[4] for c in cases)
    n_a = len(cases) - n_b
    inp = tmp_path / "step.in"
    head = np.array([NPOOL, NLINE, n_a, n_b], np.uint32)
    body = np.array([c[:4] for c in cases], np.uint32)
    inp.write_bytes(head.tobytes() + limbs_np(pool_words).tobytes() + limbs_np(line_words).tobytes() + body.tobytes())
    _run(["step", inp, tmp_path / "step.out"], timeout=300)
    got = np.fromfile(tmp_path / "step.out", dtype=np.uint32).reshape(len(cases), 36, 9)
    # expected stored forms: m or m + p for every form of the flat result
    lo = []
    for w, pa, pb, li, col in cases:
        op, d, a, b = pr.decode(w)
        regs = [pool[pa], pool[pb]]
        x = regs[a]
        if op == pr.P_SQR: y = pr.f12_sqr(x)
        elif op == pr.P_MUL: y = pr.f12_mul(x, regs[b])
        elif op == pr.P_MULL: y = pr.f12_mul(lines[li], x)
        elif op == pr.P_CONJ: y = pr.frob(x, 6)
        elif op == pr.P_CONJ0: y = pr.conj0(x)
        elif op == pr.P_COPY: y = x
        else: y = pr.frob(x, pr.FROB_POWER[op])
        lo += [pr.to_mont(f) for c0, c1 in pr.flat_to_reg(y) for f in forms(c0, c1)]
    want_lo = limbs_np(lo).reshape(len(cases), 36, 9)
    want_hi = plus_p(want_lo)
    ok = np.all(got == want_lo, axis=2) | np.all(got == want_hi, axis=2)
    bad = np.argwhere(~ok)
    if len(bad):
        msgs = []
        for ci, fi in bad[:12]:
            w, pa, pb, li, col = cases[ci]
            op, d, a, b = pr.decode(w)
            msgs.append(f"{OP_NAME[op]} d={d} a={a} b={b} column {'B' if col else 'A'} pool ({pa}, {pb}) line {li}: coefficient {fi // 6} "
                        f"form {FORM_NAME[fi % 6]}")
        classes = sorted({OP_NAME[pr.decode(cases[ci][0])[0]] for ci in np.unique(bad[:, 0])})
        pytest.fail(f"{len(bad)} wrong stored forms in {len(set(bad[:, 0]))} cases; operations {classes}:\n" + "\n".join(msgs))


def test_in_fq_star_verdict(tmp_path):
    rnd = random.Random(77)
    z = [(0, 0)] * 6
    c = rnd.randrange(1, P)
    regs = []   # (coefs, representative choice: True = every form m + p, i.e. zeros as the limb string p; None = random)
    for high in (True, False, None):
        regs += [
            ([(c, 0)] + z[1:], high),                  # in Fq*
            ([(1, 0)] + z[1:], high),
            ([(P - 1, 0)] + z[1:], high),
            (z, high),                                 # zero
            ([(0, c)] + z[1:], high),                  # Fq2 outside Fq
            ([(c, c)] + z[1:], high),
            ([(c, 1)] + z[1:], high),
        ]
        for k in range(1, 6):                          # one non-zero higher coefficient, in either coordinate, beside c or 0
            for co in ((1, 0), (0, 1), (c, 0)):
                regs.append(([(c, 0)] + [co if i == k else (0, 0) for i in range(1, 6)], high))
                regs.append(([(0, 0)] + [co if i == k else (0, 0) for i in range(1, 6)], high))
    words = []
    for coefs, high in regs:
        words += reg_words(coefs, rnd, high)
    inp = tmp_path / "check.in"
    inp.write_bytes(np.array([len(regs)], np.uint32).tobytes() + limbs_np(words).tobytes())
    _run(["check", inp, tmp_path / "check.out"], timeout=120)
    got = np.fromfile(tmp_path / "check.out", dtype=np.uint32)
    want = [1 if pr.f12_in_fq_star(pr.reg_to_flat(coefs)) else 0 for coefs, _ in regs]
    assert sum(want) == 9 and len(want) - sum(want) > 90
    wrong = [(regs[i][0], bool(regs[i][1]), int(got[i])) for i in range(len(regs)) if got[i] != want[i]]
    assert not wrong, wrong[:8]


def _piece_words(rnd, xz, y, z3, high=None):
    return [rep(v, rnd.random() < 0.5 if high is None else high) for v in (xz, y, z3)]


def _ready(pt, z):
    """affine point (or None) -> line-ready residues (X Z, Y, Z^3) with Z = z; identity: random X Z and Y, Z^3 = 0"""
    if pt is None: return None
    z3 = pow(z, 3, P)
    return (pt[0] * z3 % P, pt[1] * z3 % P, z3)


def _pieces_for(rnd, srs, parts, kind):
    """L_j, R_j affine (None: identity) for one check"""
    g = srs.g
    i = rnd.randrange(len(g) - 1)
    if kind == "all_identity": return [None] * parts, [None] * parts
    sc = [rnd.randrange(1, pr.R) for _ in range(parts)]
    L = [pr.pyref.g1_mul(a, g[i]) for a in sc]
    Rr = [pr.pyref.g1_mul(a, g[i + 1]) for a in sc]
    if kind == "identity_mixed":
        for j in range(0, parts, 2): L[j] = Rr[j] = None
    elif kind == "repeated" and parts > 1:
        L[1], Rr[1] = L[0], Rr[0]
    elif kind == "negation" and parts > 1:
        L[1], Rr[1] = pr.g1_neg(L[0]), pr.g1_neg(Rr[0])
    elif kind == "off_by_one":
        j = rnd.randrange(parts); Rr[j] = pr.pyref.g1_add(Rr[j], g[i + 1])
    elif kind == "swapped_j" and parts > 1:
        L[0], L[1] = L[1], L[0]
    elif kind == "sides_swapped":
        L, Rr = Rr, L
    return L, Rr


def _encode_pieces(rnd, pieces_l, pieces_r, parts):
    """one check's 2 parts line-ready pieces (rows (2c) parts + j, (2c + 1) parts + j); identities with Z^3 stored as 0 or as p and
    non-zero X Z, Y (an identity must not contribute its coordinates); returns (words, residues per piece or None)"""
    words, res = [], []
    for side in (pieces_l, pieces_r):
        for pt in side:
            r = _ready(pt, rnd.randrange(1, P) if rnd.random() < 0.8 else 1)
            if r is None:
                xz, y = rnd.randrange(1, P), rnd.randrange(1, P)
                w = _piece_words(rnd, xz, y, 0)
                w[2] = P if rnd.random() < 0.5 else 0
                words += w
                res.append(None)
            else:
                words += _piece_words(rnd, *r)
                res.append(r)
    return words, res


def _split_shape(parts):
    return next(s for s, k in pr.msm_split_pairs() if k == parts and s > 0) if parts > 1 else 26


def test_pair_lines_match_sparse_products(tmp_path, srs):
    rnd = random.Random(31)
    jobs, words = [], []
    kinds = ["plain", "identity_mixed", "repeated", "negation", "all_identity"]
    for parts in range(1, 7):
        shift = _split_shape(parts)
        checks = []
        for kind in kinds:
            L, Rr = _pieces_for(rnd, srs, parts, kind)
            w, res = _encode_pieces(rnd, L, Rr, parts)
            words += w
            checks.append(res)
        jobs.append((shift, parts, checks))
    at = 0
    blob = [np.array([len(jobs)], np.uint32).tobytes()]   # job headers, each followed by its pieces
    for shift, parts, checks in jobs:
        n = len(checks)
        cnt = n * 2 * parts * 3
        blob.append(np.array([shift, parts, n], np.uint32).tobytes())
        blob.append(limbs_np(words[at:at + cnt]).tobytes())
        at += cnt
    inp = tmp_path / "lines.in"
    inp.write_bytes(b"".join(blob))
    (tmp_path / "params").write_bytes(srs.params_raw)
    _run(["lines", tmp_path / "params", inp, tmp_path / "lines.out"], timeout=300)
    got = np.fromfile(tmp_path / "lines.out", dtype=np.uint32).reshape(-1, 12, 9)
    tabs = np.fromfile(tmp_path / "lines.out.tables", dtype=np.uint32).reshape(-1, 6, 9)
    its = pr.iteration_lines()
    oi, ti, wrong = 0, 0, []
    for shift, parts, checks in jobs:
        rows = [[pr.line_residues([pr.from_limbs(tabs[ti + r * 102 + l][q]) for q in range(6)]) for l in range(102)] for r in range(2 * parts)]
        ti += 2 * parts * 102
        for c, res in enumerate(checks):
            for it, (first, cnt) in enumerate(its):
                want = pr.f12_one()
                for li in range(first, first + cnt):
                    for j in range(parts):
                        for side in (0, 1):
                            r = res[side * parts + j]
                            if r is not None:
                                want = pr.f12_mul(want, pr.sparse_value_ready(rows[2 * j + side][li], *r))
                v = [pr.from_limbs(got[oi][q]) for q in range(12)]
                oi += 1
                if any(x >= 2 * P for x in v) or any(int(l) > MASK for l in got[oi - 1].ravel()):
                    wrong.append((parts, c, it, "representative not below 2p"))
                coefs = [(pr.mont_value(v[2 * k]), pr.mont_value(v[2 * k + 1])) for k in range(6)]
                if pr.reg_to_flat(coefs) != want:
                    wrong.append((parts, c, it, "value"))
    assert oi == len(got)
    assert not wrong, f"{len(wrong)} wrong iteration products (parts, check, iteration, what): {wrong[:10]}"


def test_check_verdicts_match_pyref(tmp_path, srs):
    rnd = random.Random(47)
    s_g2, g2 = pr.srs_g2(srs)
    kinds = ["plain", "identity_mixed", "off_by_one", "swapped_j", "sides_swapped"]
    blob, want = [], []
    split_jobs = []
    for parts in (1, 2, 3, 6):
        shift = _split_shape(parts)
        ws, exp = [], []
        for kind in kinds:
            L, Rr = _pieces_for(rnd, srs, parts, kind)
            w, _ = _encode_pieces(rnd, L, Rr, parts)
            ws += w
            fold = lambda pieces: pr.pyref.msm([(pow(2, shift * j, pr.R), q) for j, q in enumerate(pieces) if q is not None])
            exp.append(pr.pyref.pairing_check(fold(L), fold(Rr), s_g2, g2))
        split_jobs.append((shift, parts, ws, exp))
    jobs = 0
    for one_stream in (0, 1):
        for shift, parts, ws, exp in split_jobs:
            blob.append(np.array([one_stream, shift, parts, len(exp)], np.uint32).tobytes() + limbs_np(ws).tobytes())
            want += exp
            jobs += 1
    # whole points (pairing_check_enqueue): Jacobian pairs with random Z
    g = srs.g
    a = rnd.randrange(1, pr.R)
    pairs = [(g[0], g[1]), (pr.pyref.g1_mul(a, g[2]), pr.pyref.g1_mul(a, g[3])), (g[1], g[1]), (g[2], g[1]),
             (pr.pyref.g1_mul(a, g[2]), pr.pyref.g1_add(pr.pyref.g1_mul(a, g[3]), g[3])), (None, None), (None, g[4]), (g[4], None)]
    ws = []
    for left, right in pairs:
        for pt in (left, right):
            X, Y, Z = pr.jacobian(pt, rnd.randrange(1, P))
            w = [rep(v, rnd.random() < 0.5) for v in (X, Y, Z)]
            if pt is None and rnd.random() < 0.5: w[2] = P
            ws += w
        want.append(pr.pyref.pairing_check(left, right, s_g2, g2))
    blob.append(np.array([2, 0, 0, len(pairs)], np.uint32).tobytes() + limbs_np(ws).tobytes())
    jobs += 1
    assert True in want and False in want
    inp = tmp_path / "verdict.in"
    inp.write_bytes(np.array([jobs], np.uint32).tobytes() + b"".join(blob))
    (tmp_path / "params").write_bytes(srs.params_raw)
    _run(["verdict", tmp_path / "params", inp, tmp_path / "verdict.out"], timeout=300)
    got = [bool(x) for x in np.fromfile(tmp_path / "verdict.out", dtype=np.uint32)]
    assert len(got) == len(want)
    assert got == want


# ====================================================================== the launch tail (PairTail)
TAIL_COUNTS = [1, 2, 63, 64, 65, 128]
TAIL_PARTS = [1, 2, 6]
TAIL_WORDS = [1, 4095, 4096, 4097, 2047, 2048, 2049]       # (a copying workgroup takes 2048 words)
TAIL_SKIPS = ["inside", "both_ends", "empty", "from_start", "to_end"]
TAIL_DST_SPARE = 16
FF = 0xffffffff


def _tail_skip(kind, n_words):
    if kind == "both_ends": return 0, n_words
    if kind == "empty": return n_words // 2, n_words // 2
    if kind == "from_start": return 0, max(1, n_words // 3)
    if kind == "to_end": return min(n_words - 1, 2 * n_words // 3), n_words
    return (n_words // 3, max(n_words // 3 + 1, 2 * n_words // 3)) if n_words > 1 else (0, 1)


@pytest.fixture(scope="module")
def tail_run(tmp_path_factory, srs):
    """one child process for the 36 launches with a tail, one for the same checks without"""
    import msm_reference as ref
    tmp = tmp_path_factory.mktemp("tail")
    rnd = random.Random(53)
    pool = [ref.mul(rnd.randrange(1, pr.R), ref.G) for _ in range(12)]
    weighted = {}

    def times(pt, e):
        if (pt, e) not in weighted:
            weighted[(pt, e)] = ref.mul(pow(2, e, pr.R), pt)
        return weighted[(pt, e)]

    # the checks of a launch: four per split, of which a job takes the first n
    checks = {}
    for parts in TAIL_PARTS:
        shift = _split_shape(parts)
        ws = []
        for kind in ("plain", "off_by_one", "identity_mixed", "plain"):
            L, Rr = _pieces_for(rnd, srs, parts, kind)
            w, _ = _encode_pieces(rnd, L, Rr, parts)
            ws.append(w)
        checks[parts] = (shift, ws)
    jobs, blob, vblob = [], [], []
    for i in range(36):
        count, parts = TAIL_COUNTS[i % 6], TAIL_PARTS[(i // 6) % 3]
        n_words = TAIL_WORDS[i % 7]
        lo, hi = _tail_skip(TAIL_SKIPS[i % 5], n_words)
        assert 0 <= lo <= hi <= n_words
        n = 1 + i % 4
        shift, ws = checks[parts]
        ready = [v for w in ws[:n] for v in w]
        # the tail's points: ordinary ones, identity pieces, the identity as a sum of pieces that are not (piece 0 = -2^shift piece 1)
        words, want = [], []
        for q in range(count):
            pcs = [rnd.choice(pool) for _ in range(parts)]
            if q % 5 == 1:
                pcs = [None if rnd.random() < 0.5 else p for p in pcs]
            elif q % 5 == 2:
                pcs = [None] * parts
            elif q % 5 == 3 and parts > 1:
                pcs = [ref.neg(times(pcs[1], shift)), pcs[1]] + [None] * (parts - 2)
            whole = None
            for j, p in enumerate(pcs):
                whole = ref.add(whole, times(p, shift * j) if p is not None else None)
            if q % 5 == 3 and parts > 1:
                assert whole is None
            want.append(whole)
            for p in pcs:
                X, Y, Z = pr.jacobian(p, rnd.randrange(1, P))
                if p is None: X, Y = rnd.randrange(1, P), rnd.randrange(1, P)
                w = [rep(v, rnd.random() < 0.5) for v in (X, Y, Z)]
                if p is None and rnd.random() < 0.5: w[2] = P
                words += w
        src = np.random.RandomState(i).randint(0, 1 << 32, size=n_words, dtype=np.uint64).astype("<u4")
        src[src == FF] = 0            # (the preset stands for "not written")
        blob.append(np.array([shift, parts, n, count, n_words, lo, hi], np.uint32).tobytes() + limbs_np(ready).tobytes() + limbs_np(words).tobytes() + src.tobytes())
        vblob.append(np.array([0, shift, parts, n], np.uint32).tobytes() + limbs_np(ready).tobytes())
        jobs.append(dict(count=count, parts=parts, shift=shift, n=n, n_words=n_words, lo=lo, hi=hi, want=want, src=src))
    (tmp / "params").write_bytes(srs.params_raw)
    (tmp / "tail.in").write_bytes(np.array([len(jobs)], np.uint32).tobytes() + b"".join(blob))
    (tmp / "verdict.in").write_bytes(np.array([len(jobs)], np.uint32).tobytes() + b"".join(vblob))
    _run(["tail", tmp / "params", tmp / "tail.in", tmp / "tail.out"], timeout=300)
    _run(["verdict", tmp / "params", tmp / "verdict.in", tmp / "verdict.out"], timeout=300)
    out = np.fromfile(tmp / "tail.out", dtype=np.uint32)
    plain = np.fromfile(tmp / "verdict.out", dtype=np.uint32)
    at = vat = 0
    for j in jobs:
        s = j["count"] + 1
        def take(words):
            nonlocal at
            v = out[at:at + words]; at += words
            return v
        j["ok"] = take(j["n"]).tolist()
        j["whole"] = take(27 * s).reshape(s, 27)
        j["dev_bytes"], j["dev_ident"] = take(16 * s).reshape(s, 16), take(s)
        j["host_bytes"], j["host_ident"] = take(16 * s).reshape(s, 16), take(s)
        j["dst"] = take(j["n_words"] + TAIL_DST_SPARE)
        j["plain_ok"] = plain[vat:vat + j["n"]].tolist(); vat += j["n"]
    assert at == len(out) and vat == len(plain)
    return jobs


def test_tail_covers_its_shapes(tail_run):
    assert {(j["count"], j["parts"]) for j in tail_run} == {(c, k) for c in TAIL_COUNTS for k in TAIL_PARTS}
    assert {(j["n_words"], j["lo"] == j["hi"], j["lo"] == 0, j["hi"] == j["n_words"]) for j in tail_run} >= \
        {(w, e, a, b) for w in (4095, 4096, 4097) for e, a, b in ((True, False, False), (False, True, True), (False, False, False))}
    assert {j["n"] for j in tail_run} == {1, 2, 3, 4}


def test_tail_points_and_bytes(tail_run):
    """point q < count: the whole point is sum_j 2^(shift j) piece_j, the device and the host block hold its exact bytes and identity flag;
    the spare element behind each output keeps its preset: no lane takes q = count for a point"""
    import msm_reference as ref
    import record_reference as rr
    kinds = set()
    for j in tail_run:
        tag = (j["count"], j["parts"])
        for q, want in enumerate(j["want"]):
            w = j["whole"][q].tolist()
            assert rr.in_range(w) and ref.jac_point(w) == want, (tag, q)
            by, ident = rr.point_to_bytes(want)
            assert j["dev_bytes"][q].tobytes() == by and int(j["dev_ident"][q]) == ident, (tag, q)
            assert j["host_bytes"][q].tobytes() == by and int(j["host_ident"][q]) == ident, (tag, q)
            kinds.add(want is None)
        c = j["count"]
        assert (j["whole"][c] == FF).all() and (j["dev_bytes"][c] == FF).all() and (j["host_bytes"][c] == FF).all(), (tag, "the spare element was written")
        assert j["dev_ident"][c] == FF and j["host_ident"][c] == FF, (tag, "the spare element was written")
    assert kinds == {True, False}


def test_tail_copies_all_but_the_skipped_range(tail_run):
    for j in tail_run:
        n, lo, hi = j["n_words"], j["lo"], j["hi"]
        tag = (n, lo, hi)
        assert (j["dst"][:lo] == j["src"][:lo]).all() and (j["dst"][hi:n] == j["src"][hi:n]).all(), tag
        assert (j["dst"][lo:hi] == FF).all(), (tag, "a word inside the skipped range was written")
        assert (j["dst"][n:] == FF).all(), (tag, "written past n_words")


def test_tail_leaves_the_verdicts_alone(tail_run):
    """the verdicts of a launch with a tail are those of the same checks without one (the `verdict` mode, compared with pyref above); by
    construction the plain checks (0 and 3) pass and the one whose right side is off by one (1) fails"""
    for j in tail_run:
        assert j["ok"] == j["plain_ok"], (j["count"], j["parts"], j["ok"], j["plain_ok"])
        assert all(j["ok"][i] == want for i, want in ((0, 1), (1, 0), (3, 1)) if i < j["n"]), (j["count"], j["parts"], j["ok"])
