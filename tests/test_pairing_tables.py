"""The pairing's host-built tables (halo2_verifier_amd/csrc/pairing.hip, params.hip) against a big-integer pairing, without a GPU.

tests/cpp/pairing_tables.hip dumps the three physical operation tables (pairing_program(false), pairing_program(true),
pairing_program2() after pair_rename_registers), the Frobenius constants, the Miller-loop line coefficients of s_g2 and -g2 of the
golden SRS and the split tables of PairingDevice::split_lines (split_line_rows).  tests/pairing_reference.py then
  * checks the tables' schedules on the physical registers (what k_pairing / k_pairing2 need to be race free),
  * interprets the tables over flat Fq12 with the true Frobenius maps, the lines evaluated from the dumped coefficients at
    Jacobian points with random Z, and compares the value that reaches P_CHECK with lambda * y^M (lambda in Fq*), y the pairing
    product by pyref's textbook Miller loop and final exponentiation, M the hard part's fixed multiple."""
import os
import random
import subprocess

import pytest

import pairing_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = pr.msm_split_pairs()


@pytest.fixture(scope="module")
def tables(tmp_path_factory, srs):
    d = tmp_path_factory.mktemp("pairing_tables")
    exe, params = d / "pairing_tables", d / "params"
    cmd = ["hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-o", str(exe),
           os.path.join(ROOT, "tests", "cpp", "pairing_tables.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("hipcc failed: " + r.stderr[-2000:])
    params.write_bytes(srs.params_raw)
    r = subprocess.run([str(exe), str(params)] + ["%d:%d" % sp for sp in SPLITS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    t = pr.parse_tables(r.stdout)
    t["sg2_res"] = [pr.line_residues(x) for x in t["sg2"]]
    t["ng2_res"] = [pr.line_residues(x) for x in t["ng2"]]
    t["split_res"] = {k: [[pr.line_residues(x) for x in row] for row in rows] for k, rows in t["split"].items()}
    return t


def _schedules(t):
    c = t["const"]
    return {
        "single": (pr.single_steps(t["prog1"]), c["PAIR1_REGS"], c["N_LINES"], [0], c["PAIR_MAX_OPS"]),
        "merged": (pr.single_steps(t["prog1m"]), c["PAIR1_REGS"], c["PAIR_ITERS"], [0], c["PAIR_MAX_OPS"]),
        "two_stream": (pr.two_stream_steps(t["prog2"]), c["PAIR2_REGS"], c["PAIR_ITERS"], [0, 1], c["PAIR2_MAX_STEPS"]),
    }


@pytest.mark.parametrize("name", ["single", "merged", "two_stream"])
def test_schedule_is_race_free_and_complete(tables, name):
    steps, n_regs, n_lines, initial, max_len = _schedules(tables)[name]
    assert pr.check_schedule(steps, n_regs, n_lines, initial, max_len) == []


def test_schedule_checker_sees_the_races_it_is_for(tables):
    """the checker's own test: an in-place Frobenius, a product into a register the other column reads, a read of a register never
    written, a line used twice, a missing P_CHECK"""
    steps, n_regs, n_lines, initial, max_len = _schedules(tables)["two_stream"]
    check = lambda s: pr.check_schedule(s, n_regs, n_lines, initial, max_len)
    i = next(i for i, st in enumerate(steps) if any(w and pr.decode(w)[0] == pr.P_FROB2 for w in st))
    c = next(c for c, w in enumerate(steps[i]) if w and pr.decode(w)[0] == pr.P_FROB2)
    op, d, a, b = pr.decode(steps[i][c])
    bad = [list(s) for s in steps]
    bad[i][c] = pr.P_FROB2 | (a << 8) | (a << 16)
    assert any("writes register" in e for e in check(bad))
    i = next(i for i, st in enumerate(steps) if all(st) and pr.decode(st[0])[0] == pr.P_MUL and pr.decode(st[1])[0] == pr.P_MUL)
    op, d, a, b = pr.decode(steps[i][0])
    bad = [list(s) for s in steps]
    bad[i][1] = pr.P_SQR | (pr.decode(steps[i][1])[1] << 8) | (d << 16)
    assert any("collide" in e for e in check(bad))
    bad = [list(s) for s in steps]
    bad[0][0] = pr.P_SQR | (bad[0][0] & 0xff00) | ((n_regs - 1) << 16)
    assert any("before it is written" in e for e in check(bad))
    bad = [list(s) for s in steps]
    j = next(j for j, st in enumerate(bad) if st[0] and pr.decode(st[0])[0] == pr.P_MULL and pr.decode(st[0])[3] == 1)
    bad[j][0] = (bad[j][0] & 0xffffff) | (0 << 24)
    assert any("line use" in e for e in check(bad))
    assert any("P_CHECK" in e for e in check(bad[:-1]))


def test_frobenius_constants_are_the_frobenius_map(tables):
    """gamma_n[k] w^k = w^(k p^n) (odd n: x^(p^n) conjugates the coefficients, u^(p^n) = -u), every constant a stored
    representative below 2p"""
    for n in range(1, 5):
        wpn = pr.frob(pr.W, n)
        acc = pr.f12_one()
        for k in range(6):
            g0, g1 = tables["gamma"][(n, k)]
            assert g0 < 2 * pr.P and g1 < 2 * pr.P
            lhs = pr.f12_mul(pr.fq2_flat(0, pr.mont_value(g0), pr.mont_value(g1)), pr.pyref.f12_pow(pr.W, k))
            assert lhs == acc, (n, k)
            acc = pr.f12_mul(acc, wpn)
        u = pr.fq2_flat(0, 0, 1)
        assert pr.frob(u, n) == (u if n % 2 == 0 else pr.fq2_flat(0, 0, -1))


def test_conj_is_the_p6_frobenius():
    rnd = random.Random(3)
    x = [rnd.randrange(pr.P) for _ in range(12)]
    assert pr.frob(x, 6) == [(-v if k % 2 else v) % pr.P for k, v in enumerate(x)]


def _line_values_single(t, p0, p1):
    """pairing_program(false): line l = s_g2 line l at p0 times -g2 line l at p1 (k_pairing's own evaluation)"""
    return [pr.f12_mul(pr.sparse_value(t["sg2_res"][l], p0), pr.sparse_value(t["ng2_res"][l], p1)) for l in range(len(t["sg2_res"]))]


def _line_values_merged(rows, pieces_l, pieces_r):
    """merged iterations (k_pair_lines): the product over the iteration's lines, the parts j and both sides; rows[2 j + side]"""
    out = []
    for first, cnt in pr.iteration_lines():
        v = pr.f12_one()
        for li in range(first, first + cnt):
            for j in range(len(pieces_l)):
                v = pr.f12_mul(v, pr.sparse_value(rows[2 * j][li], pieces_l[j]))
                v = pr.f12_mul(v, pr.sparse_value(rows[2 * j + 1][li], pieces_r[j]))
        out.append(v)
    return out


def _assert_value(final, left, right, s_g2, g2):
    want, holds = pr.expected_value(left, right, s_g2, g2)
    assert pr.pyref.pairing_check(left, right, s_g2, g2) == holds
    assert pr.f12_ratio_in_fq_star(final, want), "the check's end value is not lambda * y^M"
    assert pr.f12_in_fq_star(final) == holds
    return holds


def _cases(srs):
    """(left, right, expected verdict): SRS relations e(a g_i, s_g2) = e(a g_{i+1}, g2), near misses, identities"""
    rnd = random.Random(11)
    g = srs.g
    a = rnd.randrange(1, pr.R)
    la, ra = pr.pyref.g1_mul(a, g[3]), pr.pyref.g1_mul(a, g[4])
    return [
        (g[0], g[1], True),
        (la, ra, True),
        (g[5], g[6], True),
        (la, pr.pyref.g1_add(ra, g[4]), False),       # one multiple off
        (g[1], g[1], False),
        (g[1], g[0], False),                           # sides swapped
        (None, None, True),
        (None, g[2], False),
        (g[2], None, False),
    ]


def test_single_stream_tables_compute_the_pairing(tables, srs):
    s_g2, g2 = pr.srs_g2(srs)
    rnd = random.Random(5)
    prog1, prog1m, prog2 = pr.single_steps(tables["prog1"]), pr.single_steps(tables["prog1m"]), pr.two_stream_steps(tables["prog2"])
    seen = set()
    for left, right, holds in _cases(srs):
        p0, p1 = pr.jacobian(left, rnd.randrange(1, pr.P)), pr.jacobian(right, rnd.randrange(1, pr.P))
        final, _ = pr.run_program(prog1, _line_values_single(tables, p0, p1), [0])
        assert _assert_value(final, left, right, s_g2, g2) == holds
        # the same lines merged per iteration, through the merged single-stream table and the two-stream table
        rows = [tables["sg2_res"], tables["ng2_res"]]
        merged = _line_values_merged(rows, [p0], [p1])
        f1, _ = pr.run_program(prog1m, merged, [0])
        f2, _ = pr.run_program(prog2, merged, [0, 1])
        assert pr.f12_ratio_in_fq_star(f1, final) and pr.f12_ratio_in_fq_star(f2, final)
        assert pr.f12_in_fq_star(f1) == pr.f12_in_fq_star(f2) == holds
        seen.add(holds)
    assert seen == {True, False}


@pytest.mark.parametrize("shift,parts", SPLITS)
def test_split_tables_compute_the_pairing_of_the_folded_points(tables, srs, shift, parts):
    """checks over split accumulators: the pieces L_j, R_j through split_lines' tables stand for left = sum_j 2^(shift j) L_j (and
    right likewise); holding relations (with identity pieces mixed in) and, for some pairs, a near miss"""
    s_g2, g2 = pr.srs_g2(srs)
    rows = tables["split_res"][(shift, parts)]
    assert len(rows) == 2 * parts and all(len(r) == tables["const"]["N_LINES"] for r in rows)
    rnd = random.Random(shift * 7 + parts)
    g = srs.g
    i = rnd.randrange(0, len(g) - 1)
    scal = [rnd.randrange(1, pr.R) if (j + parts) % 3 else 0 for j in range(parts)]   # some pieces are the identity
    L = [pr.pyref.g1_mul(a, g[i]) if a else None for a in scal]
    Rr = [pr.pyref.g1_mul(a, g[i + 1]) if a else None for a in scal]
    near = (shift + parts) % 4 == 1
    if near:   # one piece off by one multiple of its base
        jj = rnd.randrange(parts)
        Rr[jj] = pr.pyref.g1_add(Rr[jj], g[i + 1])
    fold = lambda pieces: pr.pyref.msm([(pow(2, shift * j, pr.R), p) for j, p in enumerate(pieces) if p is not None])
    left, right = fold(L), fold(Rr)
    zl = [pr.jacobian(p, rnd.randrange(1, pr.P)) for p in L]
    zr = [pr.jacobian(p, rnd.randrange(1, pr.P)) for p in Rr]
    lines = _line_values_merged(rows, zl, zr)
    final, _ = pr.run_program(pr.two_stream_steps(tables["prog2"]), lines, [0, 1])
    assert _assert_value(final, left, right, s_g2, g2) == (not near)
    if parts in (1, 6) or near:
        f1, _ = pr.run_program(pr.single_steps(tables["prog1m"]), lines, [0])
        assert pr.f12_ratio_in_fq_star(f1, final)


def test_merged_and_two_stream_tables_agree_on_any_lines(tables):
    """On arbitrary line values (no pairing behind them) the two tables agree up to a factor in Fq*, and not exactly: the carried
    scalar nu (pairing_program: no inversion) is a factor in Fq, which conjugation leaves alone, and pairing_program's signed-window
    x-powers take a^-k as conj(a^k) — the inverse on the cyclotomic part of r = nu f^((p^6 - 1)(p^2 + 1)) but not on nu —, while
    pairing_program2's right-to-left x-powers only multiply.  The two end values differ in their power of nu alone."""
    rnd = random.Random(9)
    prog1m, prog2 = pr.single_steps(tables["prog1m"]), pr.two_stream_steps(tables["prog2"])
    for _ in range(2):
        lines = [[rnd.randrange(pr.P) for _ in range(12)] for _ in range(tables["const"]["PAIR_ITERS"])]
        f1, _ = pr.run_program(prog1m, lines, [0])
        f2, _ = pr.run_program(prog2, lines, [0, 1])
        assert pr.f12_ratio_in_fq_star(f1, f2)
        assert f1 != f2
        assert not pr.f12_in_fq_star(f1)
