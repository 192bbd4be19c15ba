"""Operand tuples for tests/cpp/field_units.hip and the exact big-integer model of the field products of csrc/bn254.hip.h.

A field element is nine limbs of 29 bits (the top limb takes what is left), R = 2^261.  The Montgomery product of the integers a and
b is the integer t = (a b + M p) / 2^261 with M = -a b p^-1 mod 2^261: product scanning picks M one 29-bit digit per column, and M is
the only value below 2^261 that makes the division exact, so t is determined by a, b and p alone, whatever order a column's terms
are added in.  The routines leave t as eight 29-bit limbs and a top limb.  dot2 puts a0 b0 + a1 b1 in the place of a b, sqdot a0^2 + a1 b1.

The rest of the header is modelled the same way, one function per group of the program (GROUPS at the end): the corrected and lazy
linear forms, from_wide, the conversions, the inverses and powers, and the square roots of curve.hip.h.  Every one is an exact
function of integers, so every expected limb, word and flag is determined; the models assert their own bounds.

Shared by test_gpu_field_units.py (device code, both forms) and test_field_units_host.py (the C++ form on the host)."""
import random
import struct

P = {"fq": 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
     "fr": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
BITS = 29
MASK = (1 << BITS) - 1
R = 1 << (9 * BITS)
LANES = 64
PINV = {f: pow(p, -1, R) for f, p in P.items()}


def limbs(x):
    assert 0 <= x < R
    return [(x >> (BITS * i)) & MASK for i in range(9)]


def out_limbs(t):
    """t as the routines leave it: eight 29-bit limbs, then everything above them"""
    return [(t >> (BITS * i)) & MASK for i in range(8)] + [t >> (BITS * 8)]


def mont(field, s):
    """(s + M p) / 2^261 for the integer s = a b or a0 b0 + a1 b1"""
    p = P[field]
    m = -s * PINV[field] % R
    t, rem = divmod(s + m * p, R)
    assert rem == 0
    return t


def tuples(field):
    """[(class name, a0, b0, a1, b1)]: every operand class at least once, a multiple of 64 long (padded with zero tuples)"""
    p = P[field]
    rnd = random.Random(29 if field == "fq" else 31)
    out = []
    # non-canonical representatives and the values around them, every pair; the second product of dot2 takes the pair in reverse
    edge = [0, 1, p - 1, p, p + 1, 2 * p - 1]
    for a in edge:
        for b in edge:
            out.append(("edge", a, b, b, edge[(edge.index(a) + 1) % len(edge)]))
    # the fullest columns: every limb 2^29 - 1 (the top limb too: the value is 2^261 - 1)
    full = R - 1
    out.append(("full", full, full, full, full))
    out.append(("full", full, 2 * p - 1, rnd.randrange(2 * p), full))
    # one limb set and all others zero: every column's first and last term
    for i in range(9):
        hot, lone = MASK << (BITS * i), 1 << (BITS * i)
        out.append(("one limb", hot, MASK << (BITS * (8 - i)), lone, full))
        out.append(("one limb", hot, rnd.randrange(2 * p), rnd.randrange(2 * p), lone))
        out.append(("one limb", rnd.randrange(2 * p), hot, hot, hot))
    # the lazy linear forms: up to 8p on both sides (lazy_lin's documented bound)
    out.append(("lazy", 8 * p - 1, 8 * p - 1, 8 * p - 1, 8 * p - 1))
    for k in range(1, 8):
        out.append(("lazy", k * p + rnd.randrange(p), (8 - k) * p + rnd.randrange(p), 7 * p + rnd.randrange(p), k * p + rnd.randrange(p)))
    # a == b: the product against the squaring
    for a in (p - 1, 2 * p - 1, full, 8 * p - 1, rnd.randrange(2 * p), rnd.randrange(2 * p)):
        out.append(("equal", a, a, a, a))
    for _ in range(40):
        out.append(("random",) + tuple(rnd.randrange(2 * p) for _ in range(4)))
    while len(out) % LANES:
        out.append(("padding", 0, 0, 0, 0))
    return out


def encode(tup):
    return b"".join(struct.pack("<9I", *limbs(x)) for _, *ops in tup for x in ops)


def expect(field, tup):
    """per tuple {"mul": limbs, "sqr": limbs, "dot2": limbs, "sqdot": limbs}"""
    return [{"mul": out_limbs(mont(field, a0 * b0)), "sqr": out_limbs(mont(field, a0 * a0)), "dot2": out_limbs(mont(field, a0 * b0 + a1 * b1)),
             "sqdot": out_limbs(mont(field, a0 * a0 + a1 * b1))}
            for _, a0, b0, a1, b1 in tup]


def parse(stdout, routines):
    """the program's lines -> per tuple {routine: limbs}; the routine names must come in the given order"""
    rows = [l.split() for l in stdout.strip().split("\n")]
    assert len(rows) % len(routines) == 0
    got = []
    for t in range(len(rows) // len(routines)):
        d = {}
        for j, name in enumerate(routines):
            row = rows[t * len(routines) + j]
            assert row[0] == name and len(row) == 10, row
            d[name] = [int(x, 16) for x in row[1:]]
        got.append(d)
    return got


def check(field, tup, got, routines):
    """every routine of every tuple against the model; `routines` maps a routine's name to the model's key"""
    want = expect(field, tup)
    assert len(got) == len(tup)
    classes = set()
    for k, (t, g, w) in enumerate(zip(tup, got, want)):
        classes.add(t[0])
        for name, key in routines.items():
            assert g[name] == w[key], f"{field} tuple {k} ({t[0]}): {name} of {[hex(x) for x in t[1:]]} is {[hex(x) for x in g[name]]}, not {[hex(x) for x in w[key]]}"
    assert classes >= {"edge", "full", "one limb", "lazy", "equal", "random"}


# ---------------------------------------------------------------------------------------------------------------------
# The further groups of the program (field_units FIELD MODE GROUP).  A case is (class name, operands ...); every list is a multiple
# of 64 long, padded with zero cases.  Per group: the case list, its encoding, the model of every routine, and the checks that do
# not go through limbs at all.

def consts(field):
    """the header's constants as integers: ONE = R, R2 = R^2, M256 = 2^256 R (all mod p), K266 = 2^266 mod p"""
    p = P[field]
    return {"ONE": R % p, "R2": R * R % p, "M256": (R << 256) % p, "K266": (1 << 266) % p}


def words(x, n):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def value(ws, bits=BITS):
    return sum(w << (bits * i) for i, w in enumerate(ws))


def _pad(cases, zero):
    while len(cases) % LANES:
        cases.append(("padding",) + zero)
    assert len(cases) <= 4 * LANES          # at most four launches per group and field
    return cases


def canonical(field, a):
    p = P[field]
    assert 0 <= a < 2 * p
    return a - p if a >= p else a


def add(field, a, b):
    p = P[field]
    assert 0 <= a < 2 * p and 0 <= b < 2 * p
    return a + b if a + b < 2 * p else a + b - 2 * p


def sub(field, a, b):
    p = P[field]
    assert 0 <= a < 2 * p and 0 <= b < 2 * p
    return a - b if a >= b else a - b + 2 * p


def lazy_lin(field, k, sa, sb, a, b):
    """the plain integer k p - sa a - sb b: no reduction, and it must be a value of nine limbs"""
    r = k * P[field] - sa * a - sb * b
    assert 0 <= r < R, (k, sa, sb, hex(a), hex(b))
    return r


# every lazy_lin<K, SA, SB> the library instantiates (test_field_units_host.py searches csrc/ for them), on the operands (c, d)
LAZY_FORMS = {"lazy_sub": (2, -1, 1), "lazy_neg": (2, 0, 1), "lazy_neg2": (4, 0, 2), "lazy_dbl": (0, -2, 0), "lazy_add2": (0, -1, -2),
              "lazy_lin_8_1_2": (8, 1, 2)}


# ---- 1. linear forms: (class, a, b, c, d); a, b below 2p for the corrected forms, c below 4p and d at most 2p for the lazy ones (the
# widest operands their callers state: lazy_sub(D, X3) with D < 4.2p in g1_dbl_inl is the one wider, and K = 8 needs c + 2d <= 8p)
def linear_cases(field):
    p = P[field]
    rnd = random.Random(101 if field == "fq" else 103)
    out = []
    edge = [0, 1, p - 1, p, p + 1, 2 * p - 1]
    for a in edge:
        for b in edge:
            out.append(("edge", a, b, a, b))
    for s in (2 * p - 1, 2 * p, 2 * p + 1):
        for a in (p, 2 * p - 1, 2, rnd.randrange(2, p), rnd.randrange(p, 2 * p - 1)):
            out.append(("sum", a, s - a, a, s - a))
    for x in (0, 1, p - 2, rnd.randrange(p - 1)):
        for a, b in ((x, p + x), (p + x, x), (x, x + 1), (x + 1, x), (x, x), (p + x, p + x)):
            out.append(("difference", a, b, a, b))
    top = p >> (8 * BITS)
    for i in range(9):
        hot = (MASK if i < 8 else top) << (BITS * i)
        lone = 1 << (BITS * i)
        out.append(("one limb", hot, lone, hot, lone))
        out.append(("one limb", lone, hot, lone, hot))
        out.append(("one limb", hot, hot, hot, hot))
    low = (1 << (8 * BITS)) - 1                # the eight low limbs full
    for a, b in ((low, 1), (1, low), (top << (8 * BITS) | low, 1), (top << (8 * BITS), 1), (0, 1), (1 << (8 * BITS), low), (1 << (8 * BITS), 1),
                 (2 * p - 1, 2 * p - 1), (p + low, p - low), (low + 1, low)):
        out.append(("carry", a, b, a, b))
    for c, d in ((4 * p - 1, 2 * p), (0, 2 * p), (4 * p - 1, 0), (0, 0), (2 * p, 2 * p), (3 * p + low, p + 1)):
        out.append(("lazy", rnd.randrange(2 * p), rnd.randrange(2 * p), c, d))
    for _ in range(10):
        out.append(("lazy", rnd.randrange(2 * p), rnd.randrange(2 * p), rnd.randrange(4 * p), rnd.randrange(2 * p + 1)))
    for _ in range(40):
        a, b = rnd.randrange(2 * p), rnd.randrange(2 * p)
        out.append(("random", a, b, a, b))
    return _pad(out, (0, 0, 0, 0))


def linear_encode(cases):
    return b"".join(struct.pack("<9I", *limbs(x)) for _, *ops in cases for x in ops)


def linear_expect(field, case):
    p = P[field]
    _, a, b, c, d = case
    e = {"add": out_limbs(add(field, a, b)), "sub": out_limbs(sub(field, a, b)), "neg": out_limbs(sub(field, 0, a)), "dbl": out_limbs(add(field, a, a)),
         "canonical": out_limbs(canonical(field, a)), "is_zero": [int(a in (0, p))], "eq": [int((a - b) % p == 0)]}
    for name, (k, sa, sb) in LAZY_FORMS.items():
        e[name] = out_limbs(lazy_lin(field, k, sa, sb, c, d))
    return e


def linear_extra(field, case, got, device):
    p = P[field]
    _, a, b, c, d = case
    for name in ("add", "sub", "neg", "dbl", "canonical"):
        assert all(w <= MASK for w in got[name][:8]) and value(got[name]) < 2 * p, (name, got[name])
    assert value(got["add"]) % p == (a + b) % p and value(got["sub"]) % p == (a - b) % p and value(got["canonical"]) < p


# ---- 2. from_wide: (class, the nine signed accumulators)
def wide_top(field, acc):
    """the swept ninth limb of V = sum acc[l] 2^(29 l), which must lie in [0, 2^261); every step of the sweep must fit 64 bits"""
    assert len(acc) == 9
    carry = 0
    for l in range(9):
        t = acc[l] + carry
        assert -(1 << 63) <= acc[l] < 1 << 63 and -(1 << 63) <= t < 1 << 63
        carry = t >> BITS
    v = value(acc)
    assert 0 <= v < R, hex(v)
    return v >> (8 * BITS)


def from_wide(field, acc):
    p = P[field]
    q = wide_top(field, acc) // ((p >> (8 * BITS)) + 1)
    r = value(acc) - q * p
    assert 0 <= r < 2 * p, (q, hex(r))
    return r


def wide_corrects(field, acc):
    """whether the routine's quotient estimate (top floor(2^40 / d)) >> 40 falls one short of floor(top / d), so that its correction step runs"""
    top, d = wide_top(field, acc), (P[field] >> (8 * BITS)) + 1
    est = (top * ((1 << 40) // d)) >> 40
    assert est in (top // d, top // d - 1)
    return est == top // d - 1


# top limbs at which the estimate falls short (k d + r with r < ~1.96 k, d = 0x30644f for both fields), and their nearest neighbours at which it does not
_D = 0x30644f
WIDE_CORRECTION_TOPS = [_D, _D + 1, 2 * _D, 7 * _D + 13, 64 * _D + 125, 100 * _D, 128 * _D + 250, 150 * _D + 293, 169 * _D, 169 * _D + 330]
WIDE_EXACT_TOPS = [_D - 1, _D + 2, 7 * _D + 14, 100 * _D - 1, 169 * _D - 1, 169 * _D + 331]


def _spread(v, rnd, amount=32):
    """the limbs of v with amounts moved between neighbours: the same value, accumulators of both signs up to 2^35"""
    acc = limbs(v)
    for l in range(8):
        x = rnd.randrange(-amount, amount + 1)
        acc[l + 1] += x
        acc[l] -= x << BITS
    assert value(acc) == v and all(abs(x) <= 1 << 35 for x in acc)
    return acc


def wide_cases(field):
    p = P[field]
    assert (p >> (8 * BITS)) + 1 == _D
    rnd = random.Random(211 if field == "fq" else 223)
    out = []
    big = 1 << 35
    # accumulators of both signs up to 2^35 in size; the top one brings the value into range (with acc[7] = 2^35 it may be negative)
    out.append(("signed", [big] * 8 + [1 << 20]))
    out.append(("signed", [-big] * 8 + [1 << 20]))
    out.append(("signed", [big, -big] * 4 + [1 << 20]))
    out.append(("signed", [-big] * 7 + [big, -63]))
    out.append(("signed", [0] * 7 + [big, -64]))
    out.append(("signed", [1] + [0] * 6 + [big, -64]))
    for _ in range(12):
        out.append(("signed", [rnd.randrange(-big, big + 1) for _ in range(8)] + [rnd.randrange(128, (1 << BITS) - 128)]))
    for _ in range(4):
        out.append(("signed", [rnd.randrange(-big, big + 1) for _ in range(7)] + [big, rnd.randrange(-60, 0)]))
    for v in (0, 1, 2, MASK, 1 << BITS, p - 1, p, p + 1, 2 * p):
        out.append(("near zero", limbs(v)))
    for v in (1 << BITS, 1 << (4 * BITS), p, 3 * p + 1):
        out.append(("near zero", _spread(v, rnd)))
    for v in (R - 1, R - 2, R - 1 - MASK, R - p, R - (1 << (8 * BITS)), R - (1 << (8 * BITS)) - 1):
        out.append(("near top", limbs(v)))
        out.append(("near top", _spread(v, rnd, 1)))
    # the callers' weightings.  g1_dbl_inl and g1_dbl_quad: X3 = E^2 + 9p - 2D on the limbs, E^2 < 1.1p, D = 4 X B < 4.2p
    nine_p = out_limbs(9 * p)
    for f, xb in ((0, p * 103 // 100), (p * 11 // 10, 0), (p, p), (0, 0)) + tuple((rnd.randrange(p * 11 // 10), rnd.randrange(p * 103 // 100)) for _ in range(6)):
        fl, dl = limbs(f), limbs(4 * xb)
        out.append(("doubling", [fl[l] + nine_p[l] - 2 * dl[l] for l in range(9)]))
    # the line products' fold: limb sums of up to six partial products below 1.05p each, lo + 9 hs -+ ho with 6p, or 60p less it
    pl = limbs(p)
    lim = p * 105 // 100
    for kind in (0, 1, 2) * 3:
        lo, hs, ho = ([sum(col) for col in zip(*(limbs(rnd.randrange(lim)) for _ in range(n)))] for n in (6, 6, 5))
        pos = [lo[l] + 9 * hs[l] for l in range(9)]
        out.append(("fold", [pos[l] - ho[l] + 6 * pl[l] if kind == 0 else pos[l] + ho[l] if kind == 1 else 60 * pl[l] - pos[l] - ho[l] for l in range(9)]))
    out.append(("fold", [6 * x for x in pl]))
    out.append(("fold", [60 * x for x in pl]))
    # the six stored forms of a coefficient re + im u, both below 4p: alpha re + beta im + kappa p
    forms = [(1, 0, 0), (0, 1, 0), (0, -1, 4), (9, -1, 4), (1, 9, 0), (-1, -9, 40)]
    for re, im in ((4 * p - 1, 4 * p - 1), (0, 0), (0, 4 * p - 1), (4 * p - 1, 0), (rnd.randrange(4 * p), rnd.randrange(4 * p))):
        rl, il = limbs(re), limbs(im)
        for alpha, beta, kappa in forms:
            out.append(("coefficient", [alpha * rl[l] + beta * il[l] + kappa * pl[l] for l in range(9)]))
    # the sparse products' fold: v = xs + wy ys + wo yo of values below 1.05p, stored as v + 2p or as 14p - v
    for wy, wo, negate in ((9, -1, False), (9, 1, False), (9, 1, True), (1, 0, False), (1, 0, True), (0, 0, False), (0, 0, True)):
        for xs, ys, yo in ((0, 0, lim - 1), (lim - 1, lim - 1, lim - 1), tuple(rnd.randrange(lim) for _ in range(3))):
            v = [limbs(xs)[l] + wy * limbs(ys)[l] + wo * limbs(yo)[l] for l in range(9)]
            out.append(("sparse", [14 * pl[l] - v[l] if negate else v[l] + 2 * pl[l] for l in range(9)]))
    for k, top in enumerate(WIDE_CORRECTION_TOPS):
        v = top << (8 * BITS) | rnd.randrange(1 << (8 * BITS))
        out.append(("correction", _spread(v, rnd) if k % 2 else limbs(v)))
    for top in WIDE_EXACT_TOPS:
        out.append(("no correction", limbs(top << (8 * BITS) | rnd.randrange(1 << (8 * BITS)))))
    for _ in range(20):
        out.append(("random", limbs(rnd.randrange(R))))
    return _pad([(c, tuple(acc)) for c, acc in out], ((0,) * 9,))


def wide_encode(cases):
    return b"".join(struct.pack("<9q", *acc) for _, acc in cases)


def wide_expect(field, case):
    return {"from_wide": out_limbs(from_wide(field, case[1]))}


def wide_extra(field, case, got, device):
    assert wide_corrects(field, case[1]) == (case[0] == "correction") or case[0] not in ("correction", "no correction")
    assert value(got["from_wide"]) % P[field] == value(case[1]) % P[field]


# ---- 3. conversions: (class, a, W): the representative a for to_raw / to_bytes / is_odd, the 512-bit integer W = lo + 2^256 hi for the rest
def from_raw(field, x):
    assert 0 <= x < 1 << 256                  # pack29 is plain repacking: the limbs' value is x
    return mont(field, x * consts(field)["R2"])


def to_raw(field, a):
    return canonical(field, mont(field, a))   # one Montgomery pass against the limb string 1, then the canonical representative


def from_uniform(field, w):
    lo, hi = from_raw(field, w & ((1 << 256) - 1)), from_raw(field, w >> 256)
    return add(field, lo, mont(field, hi * consts(field)["M256"]))


def convert_cases(field):
    p = P[field]
    rnd = random.Random(307 if field == "fq" else 311)
    full = (1 << 256) - 1
    out = []
    for x in (0, 1, p - 1, p, p + 1, full):
        out.append(("bytes", rnd.randrange(2 * p), x))
    seams = sorted({0, 255} | {BITS * i for i in range(9)} | {BITS * i - 1 for i in range(1, 9)})
    for bit in seams:
        out.append(("seam", 1 << bit, 1 << bit))                        # (a is brought below 2p just below: bit 255 alone is not)
        out.append(("seam", (1 << bit) - 1 if bit else 0, (1 << (256 + bit)) | (full ^ (1 << bit))))
    out = [(c, a % (2 * p), w) for c, a, w in out]
    r1 = R % p
    for v in (0, 1, 2, p - 2, p - 1):
        out.append(("representative", v * r1 % p, rnd.randrange(1 << 512)))           # the two spellings of the value v
        out.append(("representative", v * r1 % p + p, rnd.randrange(1 << 512)))
    for a in (0, 1, 2, p - 2, p - 1, p, p + 1, p + 2, 2 * p - 2, 2 * p - 1):
        out.append(("representative", a, rnd.randrange(1 << 512)))
    for w in (0, (1 << 512) - 1, full, full << 256, p, p << 256, (p - 1) | (p - 1) << 256):
        out.append(("uniform", rnd.randrange(2 * p), w))
    for _ in range(40):
        out.append(("random", rnd.randrange(2 * p), rnd.randrange(1 << 512)))
    for _ in range(8):
        out.append(("random", rnd.randrange(2 * p), rnd.randrange(p)))                  # bytes that from_bytes accepts
    return _pad(out, (0, 0))


def convert_encode(cases):
    return b"".join(struct.pack("<9I16I", *limbs(a), *words(w, 16)) for _, a, w in cases)


def convert_expect(field, case):
    p = P[field]
    _, a, w = case
    x = w & ((1 << 256) - 1)
    raw = to_raw(field, a)
    return {"from_raw": out_limbs(from_raw(field, x)), "to_raw": words(raw, 8), "from_bytes_ok": [int(x < p)],
            "from_bytes": out_limbs(from_raw(field, x) if x < p else 0), "to_bytes": words(raw, 8),
            "from_mont256": out_limbs(mont(field, x * consts(field)["K266"])), "from_uniform_words": out_limbs(from_uniform(field, w)),
            "from_u32": out_limbs(from_raw(field, x & 0xffffffff)), "is_odd": [raw & 1]}


def convert_extra(field, case, got, device):
    p = P[field]
    _, a, w = case
    rinv = pow(R, -1, p)
    assert canonical(field, value(got["from_uniform_words"])) == w * R % p
    assert canonical(field, value(got["from_raw"])) == (w & ((1 << 256) - 1)) * R % p
    assert value(got["to_raw"], 32) == a * rinv % p and got["is_odd"] == [a * rinv % p & 1]
    assert canonical(field, value(got["from_mont256"])) == (w & ((1 << 256) - 1)) * 32 % p


# ---- 4. inverse and powers: (class, a, e, x): a.pow_u32(e), a.pow_limbs(x)
def pow_u32(field, a, e):
    """the routine's own schedule: MSB first, the first set bit takes a as it is"""
    r, started = consts(field)["ONE"], False
    for i in range(31, -1, -1):
        if started:
            r = mont(field, r * r)
        if (e >> i) & 1:
            r = mont(field, r * a) if started else a
            started = True
    return r


def pow_limbs(field, a, x):
    """16 table entries, four squarings per digit from the top, no product for a zero digit"""
    one = consts(field)["ONE"]
    tbl = [one, a]
    for _ in range(2, 16):
        tbl.append(mont(field, tbl[-1] * a))
    r = one
    for i in range(63, -1, -1):
        for _ in range(4):
            r = mont(field, r * r)
        d = (x >> (4 * i)) & 15
        if d:
            r = mont(field, r * tbl[d])
    return r


def inv_safegcd(field, a):
    p, r2 = P[field], consts(field)["R2"]
    c = canonical(field, a)
    t = pow(c, -1, p) if c else 0
    return mont(field, t * mont(field, r2 * r2))


def inverse_cases(field):
    p = P[field]
    rnd = random.Random(401 if field == "fq" else 409)
    alt = int("55" * 32, 16) % p
    vals = [0, 1, 2, 3, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, p, p + 1, 2 * p - 1, alt]
    for k in (30, 60, 128, 253):
        vals += [1 << k, (1 << k) - 1]
    exps = [0, 1, 2, 1 << 31, (1 << 32) - 1]
    xs = [0, 1, p - 2, (1 << 256) - 1, (p + 1) // 4, 15 << 252, 1 << 255, 0x10]
    out = []
    for i, a in enumerate(vals):
        for j, e in enumerate(exps):
            out.append(("value", a, e, xs[(i + j) % len(xs)] if j else rnd.randrange(1 << 256)))
    assert {c[2] for c in out} == set(exps)
    _pad(out, (0, 0, 0))
    seen = set()
    while len(seen) < LANES:                     # one whole wave of random values, every lane another
        seen.add(rnd.randrange(2 * p))
    for a in sorted(seen):
        out.append(("random", a, rnd.randrange(1 << 32), rnd.randrange(1 << 256)))
    return _pad(out, (0, 0, 0))


def inverse_encode(cases):
    return b"".join(struct.pack("<9I9I", *limbs(a), e, *words(x, 8)) for _, a, e, x in cases)


def inverse_expect(field, case):
    _, a, e, x = case
    return {"inv_safegcd": out_limbs(inv_safegcd(field, a)), "inv_fermat": out_limbs(pow_limbs(field, a, P[field] - 2)),
            "pow_u32": out_limbs(pow_u32(field, a, e)), "pow_limbs": out_limbs(pow_limbs(field, a, x))}


def inverse_extra(field, case, got, device):
    p = P[field]
    _, a, e, x = case
    rinv = pow(R, -1, p)
    for name in ("inv_safegcd", "inv_fermat"):
        inv = canonical(field, value(got[name]))
        assert inv * a % p == (R * R % p if a % p else 0) and (a % p or inv == 0), (name, hex(a))      # inv(0) is zero, in either spelling
    assert a % p or value(got["inv_safegcd"]) == 0
    # the value held is a / R: its powers, whatever the schedule
    assert value(got["pow_u32"]) % p == pow(a * rinv, e, p) * R % p and value(got["pow_limbs"]) % p == pow(a * rinv, x, p) * R % p


# ---- 5. square roots (Fq): (class, a)
def root_cases(field):
    assert field == "fq"
    p = P[field]
    rnd = random.Random(503)
    r1 = R % p
    out = [("zero", 0), ("p", p)]
    for x in (1, 2):
        out.append(("curve", (x ** 3 + 3) * r1 % p))
    for _ in range(12):
        sq = rnd.randrange(1, p) ** 2 % p
        out.append(("residue", sq * r1 % p))
        out.append(("non-residue", (p - sq) * r1 % p))          # p = 3 mod 4: -1 is no square
    for c, a in list(out[4:12]):
        out.append(("high", a + p))                               # the other spelling, residues and non-residues alike
    for _ in range(20):
        out.append(("random", rnd.randrange(2 * p)))
    return _pad(out, (0,))


def root_encode(cases):
    return b"".join(struct.pack("<9I", *limbs(a)) for _, a in cases)


def root_expect(field, case):
    return {}


def root_extra(field, case, got, device):
    p = P[field]
    c, a = case
    x = a * pow(R, -1, p) % p
    want = pow(x, (p + 1) // 4, p) * R % p
    residue = x == 0 or pow(x, (p - 1) // 2, p) == 1
    assert residue if c in ("zero", "p", "residue") else not residue if c == "non-residue" else True
    names = ["sqrt_w4"] + (["sqrt_loop_chain", "sqrt_loop_inl"] if device else [])
    assert set(got) == set(names)
    for name in names:
        r = value(got[name])
        assert all(w <= MASK for w in got[name][:8]) and r < 2 * p, (name, got[name])
        assert r % p == want, (name, hex(a))
        assert (mont(field, r * r) % p == a % p) == residue, (name, hex(a))
    if device:
        assert got["sqrt_loop_chain"] == got["sqrt_loop_inl"], hex(a)     # a Montgomery product's result does not depend on its form


# group -> its routines (name, words, device only), cases, encoding, model, further checks and the classes that must occur
GROUPS = {
    "linear": dict(routines=[(n, 9, False) for n in ("add", "sub", "neg", "dbl", "canonical")] + [("is_zero", 1, False), ("eq", 1, False)] + [(n, 9, False) for n in LAZY_FORMS],
                   cases=linear_cases, encode=linear_encode, expect=linear_expect, extra=linear_extra,
                   classes={"edge", "sum", "difference", "one limb", "carry", "lazy", "random"}),
    "wide": dict(routines=[("from_wide", 9, False)], cases=wide_cases, encode=wide_encode, expect=wide_expect, extra=wide_extra,
                 classes={"signed", "near zero", "near top", "doubling", "fold", "coefficient", "sparse", "correction", "no correction", "random"}),
    "convert": dict(routines=[("from_raw", 9, False), ("to_raw", 8, False), ("from_bytes_ok", 1, False), ("from_bytes", 9, False), ("to_bytes", 8, False), ("from_mont256", 9, False),
                              ("from_uniform_words", 9, False), ("from_u32", 9, False), ("is_odd", 1, False)],
                    cases=convert_cases, encode=convert_encode, expect=convert_expect, extra=convert_extra,
                    classes={"bytes", "seam", "representative", "uniform", "random"}),
    "inverse": dict(routines=[(n, 9, False) for n in ("inv_safegcd", "inv_fermat", "pow_u32", "pow_limbs")],
                    cases=inverse_cases, encode=inverse_encode, expect=inverse_expect, extra=inverse_extra, classes={"value", "random"}),
    "root": dict(routines=[("sqrt_w4", 9, False), ("sqrt_loop_chain", 9, True), ("sqrt_loop_inl", 9, True)],
                 cases=root_cases, encode=root_encode, expect=root_expect, extra=root_extra,
                 classes={"zero", "p", "curve", "residue", "non-residue", "high", "random"}),
}
FIELDS = {"linear": ["fq", "fr"], "wide": ["fq", "fr"], "convert": ["fq", "fr"], "inverse": ["fq", "fr"], "root": ["fq"]}


def parse_group(stdout, group, device):
    """the program's lines -> per case {routine: words}; names and word counts must be the group's, in its order"""
    routines = [(n, w) for n, w, dev in GROUPS[group]["routines"] if device or not dev]
    rows = [l.split() for l in stdout.strip().split("\n")]
    assert len(rows) % len(routines) == 0
    got = []
    for t in range(len(rows) // len(routines)):
        d = {}
        for j, (name, nwords) in enumerate(routines):
            row = rows[t * len(routines) + j]
            assert row[0] == name and len(row) == 1 + nwords, row
            d[name] = [int(x, 16) for x in row[1:]]
        got.append(d)
    return got


def check_group(field, group, cases, got, device):
    """every routine of every case against its model, then the checks that know no limbs; every operand class must have occurred"""
    g = GROUPS[group]
    assert len(got) == len(cases) and len(cases) % LANES == 0
    classes = set()
    for k, (case, have) in enumerate(zip(cases, got)):
        classes.add(case[0])
        for name, want in g["expect"](field, case).items():
            assert have[name] == want, f"{field} {group} case {k} ({case[0]}): {name} of {case[1:]} is {[hex(x) for x in have[name]]}, not {[hex(x) for x in want]}"
        g["extra"](field, case, have, device)
    assert classes >= g["classes"], g["classes"] - classes
