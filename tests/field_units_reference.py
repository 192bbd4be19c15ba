"""Operand tuples for tests/cpp/field_units.hip and the exact big-integer model of the field products of csrc/bn254.hip.h.

A field element is nine limbs of 29 bits (the top limb takes what is left), R = 2^261.  The Montgomery product of the integers a and
b is the integer t = (a b + M p) / 2^261 with M = -a b p^-1 mod 2^261: product scanning picks M one 29-bit digit per column, and M is
the only value below 2^261 that makes the division exact, so t is determined by a, b and p alone, whatever order a column's terms
are added in.  The routines leave t as eight 29-bit limbs and a top limb.  dot2 puts a0 b0 + a1 b1 in the place of a b, sqdot a0^2 + a1 b1.

Shared by test_gpu_field_units.py (device code, both forms) and test_field_units_host.py (the C++ form on the host)."""
import random
import struct

P = {"fq": 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47,
     "fr": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
BITS = 29
MASK = (1 << BITS) - 1
R = 1 << (9 * BITS)
LANES = 64


def limbs(x):
    assert 0 <= x < R
    return [(x >> (BITS * i)) & MASK for i in range(9)]


def out_limbs(t):
    """t as the routines leave it: eight 29-bit limbs, then everything above them"""
    return [(t >> (BITS * i)) & MASK for i in range(8)] + [t >> (BITS * 8)]


def mont(field, s):
    """(s + M p) / 2^261 for the integer s = a b or a0 b0 + a1 b1"""
    p = P[field]
    m = -s * pow(p, -1, R) % R
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
