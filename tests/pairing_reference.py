"""Big-integer reference for the pairing kernels (halo2_verifier_amd/csrc/pairing.hip), independent of the library's own tower.

Fq12 is oracle/pyref.py's flat Fq[w] / (w^12 - 18 w^6 + 82).  The kernels hold an Fq12 as six coefficients c0 + c1 u of
Fq2[w] / (w^6 - xi), xi = 9 + u; with u = w^6 - 9 coefficient k maps to flat[k] += c0 - 9 c1, flat[k + 6] += c1.

Here: the operation-table decoding and a schedule checker for the physical registers, an interpreter of the tables over flat Fq12
(Frobenius maps as 12 x 12 matrices made from w^(p^n), never from the library's gamma tables), the sparse line values the kernels
evaluate (a Y + b X Z w + c Z^3 w^3, 1 at an identity point), and the expected end value of a check: lambda * y^M with lambda in Fq*,
y = e(left, s_g2) e(right, -g2) by pyref's Miller loops and plain final exponentiation, M the multiple of the hard part below."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402

P, R = pyref.P, pyref.R
RINV = pow(1 << 261, -1, P)          # the kernels' Montgomery radix: nine 29-bit limbs
BN_X = 4965661367192848881
# The hard part of the final exponentiation after Fuentes-Castaneda, Knapp and Rodriguez-Henriquez ("Faster hashing to G2", SAC 2011)
# as used for BN curves (e.g. Aranha et al.; Duquesne and Ghammam): it computes f^(M (p^4 - p^2 + 1) / r), M = 2x(6x^2 + 3x + 1)
M_HARD = 2 * BN_X * (6 * BN_X * BN_X + 3 * BN_X + 1)
assert math.gcd(M_HARD, R) == 1

P_SQR, P_MUL, P_MULL, P_CONJ, P_FROB, P_CONJ0, P_COPY, P_CHECK, P_FROB2, P_FROB3, P_FROB4 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
FROB_POWER = {P_FROB: 1, P_FROB2: 2, P_FROB3: 3, P_FROB4: 4}
PRODUCTS = (P_SQR, P_MUL, P_MULL)
ATE_LOW = 0x9d797039be763ba8


# ------------------------------------------------------------------ representations
def mont_value(v):
    """the residue of a stored representative (the integer the nine limbs spell, Montgomery form R = 2^261)"""
    return v * RINV % P


def to_mont(x):
    return x * (1 << 261) % P


def limbs(v):
    return [(v >> (29 * l)) & 0x1fffffff for l in range(8)] + [v >> (29 * 8)]


def from_limbs(ls):
    return sum(int(x) << (29 * l) for l, x in enumerate(ls))


def fq2_flat(k, c0, c1):
    """the coefficient c0 + c1 u at w^k (k < 6) as a flat Fq12"""
    f = [0] * 12
    f[k] = (c0 - 9 * c1) % P
    f[k + 6] = c1 % P
    return f


def reg_to_flat(coefs):
    """six (c0, c1) residues -> flat Fq12"""
    f = [0] * 12
    for k, (c0, c1) in enumerate(coefs):
        f[k] = (f[k] + c0 - 9 * c1) % P
        f[k + 6] = (f[k + 6] + c1) % P
    return f


def flat_to_reg(f):
    """flat Fq12 -> six (c0, c1) residues (c1 = flat[k + 6], c0 = flat[k] + 9 c1)"""
    return [((f[k] + 9 * f[k + 6]) % P, f[k + 6] % P) for k in range(6)]


f12_mul, f12_one = pyref.f12_mul, pyref.f12_one
W = [0, 1] + [0] * 10
F12_ZERO = [0] * 12


def f12_sqr(a): return f12_mul(a, a)


def f12_in_fq_star(a): return a[0] % P != 0 and all(x % P == 0 for x in a[1:])


def f12_ratio_in_fq_star(a, b):
    """a = lambda b with lambda in Fq* (b != 0)"""
    i = next(i for i in range(12) if b[i])
    lam = a[i] * pow(b[i], -1, P) % P
    return lam != 0 and all((a[t] - lam * b[t]) % P == 0 for t in range(12))


# ------------------------------------------------------------------ Frobenius maps as matrices
_FROB = {}


def frob_matrix(n):
    """columns: (w^(p^n))^i, so that x^(p^n) = sum_i x_i (w^(p^n))^i (the coefficients lie in Fq, which the map fixes)"""
    if n not in _FROB:
        wp = pyref.f12_pow(W, P ** n)
        cols, c = [], f12_one()
        for _ in range(12):
            cols.append(c)
            c = f12_mul(c, wp)
        _FROB[n] = cols
    return _FROB[n]


def frob(x, n):
    cols = frob_matrix(n)
    out = [0] * 12
    for i, xi in enumerate(x):
        if xi:
            col = cols[i]
            for t in range(12):
                out[t] += xi * col[t]
    return [v % P for v in out]


def conj0(x):
    """P_CONJ0: the conjugate of register coefficient 0 (an Fq2 value); the other coefficients become 0"""
    c0, c1 = flat_to_reg(x)[0]
    return fq2_flat(0, c0, -c1)


# ------------------------------------------------------------------ operation tables
def decode(w):
    return w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24


def reads_of(op, a, b):
    if op == P_MUL: return [a, b]
    if op in (P_SQR, P_MULL, P_CONJ, P_CONJ0, P_COPY, P_CHECK) or op in FROB_POWER: return [a]
    return []


def writes_of(op, d):
    return None if op in (0, P_CHECK) else d


def check_schedule(steps, n_regs, n_lines, initial, max_len):
    """steps: a list of columns per step (one word each, 0 = nothing).  Returns a list of violations (empty = sound)."""
    bad = []
    if len(steps) > max_len: bad.append(f"{len(steps)} steps > {max_len}")
    written = set(initial)
    line_use = [0] * n_lines
    checks = [(i, c) for i, st in enumerate(steps) for c, w in enumerate(st) if w and decode(w)[0] == P_CHECK]
    if len(checks) != 1: bad.append(f"{len(checks)} P_CHECK")
    elif checks[0][0] != len(steps) - 1 or any(w for c, w in enumerate(steps[-1]) if c != checks[0][1]):
        bad.append("P_CHECK is not the last operation")
    for i, st in enumerate(steps):
        acc = []
        for c, w in enumerate(st):
            if not w: continue
            op, d, a, b = decode(w)
            if op not in (P_SQR, P_MUL, P_MULL, P_CONJ, P_FROB, P_CONJ0, P_COPY, P_CHECK, P_FROB2, P_FROB3, P_FROB4):
                bad.append(f"step {i} col {c}: unknown op {op}"); continue
            rd, wr = reads_of(op, a, b), writes_of(op, d)
            if op == P_MULL:
                if b >= n_lines: bad.append(f"step {i} col {c}: line {b} >= {n_lines}")
                else: line_use[b] += 1
            for r in rd + ([wr] if wr is not None else []):
                if r >= n_regs: bad.append(f"step {i} col {c}: register {r} >= {n_regs}")
            for r in rd:
                if r not in written: bad.append(f"step {i} col {c}: register {r} read before it is written")
            acc.append((c, op, rd, wr))
        for c, op, rd, wr in acc:
            if wr is None: continue
            if (op in PRODUCTS or op in FROB_POWER) and wr in [r for _, _, rr, _ in acc for r in rr]:
                bad.append(f"step {i} col {c}: op {op} writes register {wr}, which the step reads")
            for c2, op2, rd2, wr2 in acc:
                if c2 != c and (wr == wr2 or wr in rd2):
                    bad.append(f"step {i}: columns {c} and {c2} collide on register {wr}")
        for c, op, rd, wr in acc:
            if wr is not None: written.add(wr)
    if any(u != 1 for u in line_use): bad.append(f"line use counts {sorted(set(line_use))}, not all 1")
    return bad


def run_program(steps, lines, initial, frob_fn=frob):
    """interpret a table over flat Fq12: every operation of a step reads the registers as they were before the step.
    lines[l]: the flat value of line l.  Returns (value of the P_CHECK register, registers)."""
    reg = {r: f12_one() for r in initial}
    final = None
    for st in steps:
        out = []
        for w in st:
            if not w: continue
            op, d, a, b = decode(w)
            if op == P_SQR: out.append((d, f12_sqr(reg[a])))
            elif op == P_MUL: out.append((d, f12_mul(reg[a], reg[b])))
            elif op == P_MULL: out.append((d, f12_mul(lines[b], reg[a])))
            elif op == P_CONJ: out.append((d, frob_fn(reg[a], 6)))
            elif op == P_CONJ0: out.append((d, conj0(reg[a])))
            elif op == P_COPY: out.append((d, list(reg[a])))
            elif op in FROB_POWER: out.append((d, frob_fn(reg[a], FROB_POWER[op])))
            elif op == P_CHECK: final = list(reg[a])
        for d, v in out:
            reg[d] = v
    return final, reg


def single_steps(prog):
    return [[w] for w in prog]


def two_stream_steps(prog2):
    return [[prog2[2 * i], prog2[2 * i + 1]] for i in range(len(prog2) // 2)]


# ------------------------------------------------------------------ line tables and their values
def iteration_lines():
    """merged iteration it -> (first line, count): doubling line, plus the addition line where 6x + 2 has a set bit; 64, 65: the
    two Frobenius corrections"""
    its, line = [], 0
    for i in range(63, -1, -1):
        cnt = 1 + ((ATE_LOW >> i) & 1)
        its.append((line, cnt))
        line += cnt
    its += [(line, 1), (line + 1, 1)]
    return its


def sparse_value(lc, pt):
    """line coefficients (a, b, c), each an Fq2 residue pair, at the Jacobian point pt = (X, Y, Z) residues (None or Z = 0:
    identity): a Y + b X Z w + c Z^3 w^3, or 1"""
    if pt is None or pt[2] % P == 0: return f12_one()
    X, Y, Z = pt
    (a0, a1), (b0, b1), (c0, c1) = lc
    xz, z3 = X * Z % P, pow(Z, 3, P)
    f = fq2_flat(0, a0 * Y, a1 * Y)
    g = fq2_flat(1, b0 * xz, b1 * xz)
    h = fq2_flat(3, c0 * z3, c1 * z3)
    return [(f[t] + g[t] + h[t]) % P for t in range(12)]


def sparse_value_ready(lc, xz, y, z3):
    """the same at a piece given line-ready as (X Z, Y, Z^3) residues (k_pair_lines): 1 when Z^3 = 0"""
    if z3 % P == 0: return f12_one()
    (a0, a1), (b0, b1), (c0, c1) = lc
    f = fq2_flat(0, a0 * y, a1 * y)
    g = fq2_flat(1, b0 * xz, b1 * xz)
    h = fq2_flat(3, c0 * z3, c1 * z3)
    return [(f[t] + g[t] + h[t]) % P for t in range(12)]


def jacobian(pt, z):
    """affine (x, y) or None -> (X, Y, Z) with Z = z"""
    if pt is None: return (0, 1, 0)
    return (pt[0] * z * z % P, pt[1] * z * z * z % P, z % P)


def g1_neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def expected_value(left, right, s_g2, g2):
    """y^M for y = e(left, s_g2) e(right, -g2), pyref's construction, and pyref's verdict"""
    ng2 = (g2[0], ((-g2[1][0]) % P, (-g2[1][1]) % P))
    f = f12_mul(pyref.miller_loop(s_g2, left), pyref.miller_loop(ng2, right))
    y = pyref.f12_pow(f, (P ** 12 - 1) // R)
    return pyref.f12_pow(y, M_HARD), y == f12_one()


def srs_g2(srs):
    """srs_util's G2 tuples (x.c0, x.c1, y.c0, y.c1) -> pyref's ((x0, x1), (y0, y1)) for (s_g2, g2)"""
    t = lambda q: ((q[0], q[1]), (q[2], q[3]))
    return t(srs.s_g2), t(srs.g2)


def parse_tables(text):
    """tests/cpp/pairing_tables.hip's output"""
    out = dict(split={}, gamma={})
    for ln in text.split("\n"):
        f = ln.split()
        if not f: continue
        if f[0] == "const":
            out["const"] = {f[i]: int(f[i + 1]) for i in range(1, len(f), 2)}
        elif f[0] in ("prog1", "prog1m", "prog2"):
            out[f[0]] = [int(x, 16) for x in f[2:]]
            assert len(out[f[0]]) == int(f[1])
        elif f[0] == "gamma":
            out["gamma"][(int(f[1]), int(f[2]))] = (int(f[3], 16), int(f[4], 16))
        elif f[0] in ("sg2", "ng2"):
            out.setdefault(f[0], []).append([int(x, 16) for x in f[2:8]])
        elif f[0] == "split":
            shift, parts, row = int(f[1]), int(f[2]), int(f[3])
            rows = out["split"].setdefault((shift, parts), [[] for _ in range(2 * parts)])
            rows[row].append([int(x, 16) for x in f[5:11]])
    return out


def line_residues(raw):
    """six stored representatives (a0 a1 b0 b1 c0 c1) -> ((a0, a1), (b0, b1), (c0, c1)) residues"""
    v = [mont_value(x) for x in raw]
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


def msm_split_pairs():
    """every (shift, parts) the MSM planner can hand the split pairing (halo2_verifier_amd/csrc/msm.hip: msm_plan picks a window
    width c in 2 .. 15 with ceil(130 / c) windows; msm_enqueue_multi cuts them into parts of wpp = ceil(windows / want) windows,
    want in 2 .. MSM_MAX_PARTS, shift = c wpp), and parts 1 .. 6 at shift 0 beside them"""
    pairs = set()
    for c in range(2, 16):
        w = (130 + c - 1) // c
        for want in range(2, 7):
            wpp = (w + want - 1) // want
            pairs.add((c * wpp, (w + wpp - 1) // wpp))
    pairs |= {(0, k) for k in range(1, 7)}
    return sorted(pairs)
