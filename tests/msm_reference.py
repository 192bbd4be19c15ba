"""Big-integer reference for the MSM kernels (halo2_verifier_amd/csrc/msm.hip) and the G1 group law they run (curve.hip.h),
independent of the library's own arithmetic: plain affine / Jacobian G1 over Python integers, the stored forms of the kernels
(Montgomery residues with R = 2^261 in nine 29-bit limbs, as m or as m + p), the GLV eigenvalue from the lattice constants of
glv_decompose, and the scalar classes of tests/test_gpu_msm_units.py.  Nothing here ports a kernel."""
import random

from pairing_reference import P, R, from_limbs, limbs, mont_value, to_mont

G = (1, 2)
# curve.hip.h g1_beta_times: the cube root of unity of phi(x, y) = (beta x, y)
BETA = 0x30644e72e131a0295e6dd9e7e0acccb0c28f069fbb966e3de4bd44e5607cfd48
# msm.hip glv_decompose: the lattice basis (a1, b1), (a2, b2) with a_i + b_i lambda = 0 (mod r); a2 = -b1
A1 = 0x6f4d8248eeb859fc8211bbeb7d4f1128
B1N = 0x89d3256894d213e3
B2 = 0x6f4d8248eeb859fd0be4e1541221250b
LAMBDA = A1 * pow(B1N, -1, R) % R
assert (LAMBDA * LAMBDA + LAMBDA + 1) % R == 0
assert (A1 - B1N * LAMBDA) % R == 0 and (B1N + B2 * LAMBDA) % R == 0
assert pow(BETA, 3, P) == 1 and BETA != 1


# ------------------------------------------------------------------ G1 over big integers (None = the identity)
def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - 3) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def dbl(pt):
    if pt is None or pt[1] == 0:
        return None
    x, y = pt
    m = 3 * x * x * pow(2 * y, -1, P) % P
    x3 = (m * m - 2 * x) % P
    return (x3, (m * (x - x3) - y) % P)


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        return dbl(p) if p[1] == q[1] else None
    m = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x3 = (m * m - p[0] - q[0]) % P
    return (x3, (m * (p[0] - x3) - p[1]) % P)


def jac_to_affine(X, Y, Z):
    """residues (X, Y, Z) of a Jacobian point -> affine (x, y) = (X / Z^2, Y / Z^3), None for Z = 0"""
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi * zi * zi % P)


def _jdbl(X, Y, Z):
    if Z == 0 or Y == 0:
        return (0, 1, 0)
    A, B = X * X % P, Y * Y % P
    C = B * B % P
    D = 4 * X * B % P
    E = 3 * A % P
    X3 = (E * E - 2 * D) % P
    return (X3, (E * (D - X3) - 8 * C) % P, 2 * Y * Z % P)


def _jadd_affine(X, Y, Z, q):
    if Z == 0:
        return (q[0], q[1], 1)
    ZZ = Z * Z % P
    U2, S2 = q[0] * ZZ % P, q[1] * Z * ZZ % P
    if U2 == X:
        return _jdbl(X, Y, Z) if S2 == Y else (0, 1, 0)
    H, r = (U2 - X) % P, (S2 - Y) % P
    HH = H * H % P
    HHH, V = H * HH % P, X * HH % P
    X3 = (r * r - HHH - 2 * V) % P
    return (X3, (r * (V - X3) - Y * HHH) % P, Z * H % P)


def mul(k, pt):
    """[k] pt for any integer k (reduced mod r)"""
    k %= R
    if pt is None or k == 0:
        return None
    acc = (0, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jdbl(*acc)
        if bit == "1":
            acc = _jadd_affine(*acc, pt)
    return jac_to_affine(*acc)


def multiples(count, pt=G):
    """[1 pt, 2 pt, ..., count pt]"""
    out, cur = [], None
    for _ in range(count):
        cur = add(cur, pt)
        out.append(cur)
    return out


def msm(scalars, points):
    """sum_i scalars[i] * points[i], term by term (a few hundred terms at the most)"""
    acc = None
    for k, pt in zip(scalars, points):
        acc = add(acc, mul(k, pt))
    return acc


def msm_by_logs(scalars, logs, pt=G):
    """the same sum when points[i] = logs[i] * pt: one scalar multiplication"""
    return mul(sum(k * m for k, m in zip(scalars, logs)) % R, pt)


def phi(pt):
    return None if pt is None else (BETA * pt[0] % P, pt[1])


assert on_curve(G) and mul(LAMBDA, (G[0], G[1])) == phi(G), "lambda and beta do not belong together"
assert mul(R - 1, G) == neg(G) and add(mul(5, G), mul(7, G)) == mul(12, G)


# ------------------------------------------------------------------ the kernels' stored forms
def fq_words(x, plus_p=False):
    """nine limbs of the Montgomery form of the residue x, as m (below p) or as m + p"""
    return limbs(to_mont(x % P) + (P if plus_p else 0))


def fq_value(words):
    return mont_value(from_limbs(words))


def fq_in_range(words):
    """limbs below 2^29, the value below 2p"""
    return all(0 <= int(w) < (1 << 29) for w in words) and from_limbs(words) < 2 * P


def jac_words(pt, z=1, reps=(False, False, False)):
    """27 words of the Jacobian form (x z^2, y z^3, z) of an affine point; None: (0, 1, 0), the library's identity"""
    if pt is None:
        return fq_words(0, reps[0]) + fq_words(1, reps[1]) + fq_words(0, reps[2])
    return fq_words(pt[0] * z * z, reps[0]) + fq_words(pt[1] * z * z * z, reps[1]) + fq_words(z, reps[2])


def jac_point(words):
    """27 words -> the affine point they stand for"""
    return jac_to_affine(fq_value(words[0:9]), fq_value(words[9:18]), fq_value(words[18:27]))


def affine_bytes(pt):
    """64 canonical bytes x | y (zeros: the identity)"""
    return bytes(64) if pt is None else int(pt[0]).to_bytes(32, "little") + int(pt[1]).to_bytes(32, "little")


def scalar_words(k):
    assert 0 <= k < R
    return [(k >> (32 * i)) & 0xffffffff for i in range(8)]


# ------------------------------------------------------------------ scalar classes
def edge_scalars():
    out = [0, 1, 2, R - 1, R - 2, LAMBDA, LAMBDA + 1, LAMBDA - 1, R - LAMBDA, LAMBDA * LAMBDA % R]
    for i in range(254):
        out += [(1 << i) % R, ((1 << i) - 1) % R, (R - (1 << i)) % R]
    return out


NEG_K1 = [1 << 126, (1 << 126) - 1, (1 << 126) + (1 << 64), A1 - 1]
NEG_J = [1, 2, 3, 1 << 20, 1 << 62]


def negative_half_scalars():
    """[(k, k1, j)]: k = k1 - j lambda mod r, which glv_decompose's flooring splits into exactly (k1, -j): (k1, -j) lies in the cell"""
    assert all(in_cell(k1, -j) for k1 in NEG_K1 for j in NEG_J)
    return [((k1 - j * LAMBDA) % R, k1, j) for k1 in NEG_K1 for j in NEG_J]


def width_magnitudes(c):
    """magnitudes in [2^64, 2^126) for window width c: all ones, the digit 2^(c-1) in every window, 2^(c-1) + 1 in every window,
    only the top bit"""
    def every_window(d):
        v, w = 0, 0
        while (d << (c * w)).bit_length() <= 126:
            v |= d << (c * w)
            w += 1
        return v
    mags = [(1 << 126) - 1, every_window(1 << (c - 1)), every_window((1 << (c - 1)) + 1), 1 << 125]
    assert all((1 << 64) <= m < (1 << 126) for m in mags)
    return mags


def in_cell(k1, k2):
    """(k1, k2) = alpha (a1, b1) + beta (a2, b2) with alpha, beta in [0, 1): the halves exact floors leave (alpha r = k1 b2 - a2 k2,
    beta r = a1 k2 + a2 k1, the determinant being r)"""
    return 0 <= k1 * B2 - B1N * k2 < R and 0 <= A1 * k2 + B1N * k1 < R


def width_scalars(c):
    """[(k, k1, k2)]: k = k1 + k2 lambda with both halves from width_magnitudes(c): that region lies inside the lattice cell, so it
    decomposes to itself"""
    m = width_magnitudes(c)
    assert all(in_cell(k1, k2) for k1 in m for k2 in m)
    return [((k1 + k2 * LAMBDA) % R, k1, k2) for k1 in m for k2 in m]


def random_scalars(seed, count=200):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(count)]
