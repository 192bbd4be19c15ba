"""Point hints in Python integers (include/h2v_hints.h): what G1Affine::from_bytes makes of a compressed point, the hint rows of
proofs, when a hint is USED, and the adversarial hint sets that the tests of the hinted decompression share.

BN254: y^2 = x^3 + 3 over F_p, p = 3 mod 4, so a square root of a residue a is a^((p + 1) / 4).  The compressed form is x as 32
little-endian bytes with the flags in byte 31: 0x40 = the parity of the canonical y, 0x80 = the identity."""
import random

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
FLAG_SIGN, FLAG_IDENTITY = 0x40, 0x80
HINT_SETS = ("right", "zero", "other_root", "plus_p", "random", "lane0_wrong", "even_lanes")
WAVE = 64


def le32(v):
    return int(v).to_bytes(32, "little")


def encode(x, sign=0, identity=0):
    """the compressed form of a point with this x (any integer below 2^254) and these flags"""
    b = bytearray(le32(x))
    assert not b[31] & 0xc0
    b[31] |= (FLAG_SIGN if sign else 0) | (FLAG_IDENTITY if identity else 0)
    return bytes(b)


def decode(point32):
    """-> the canonical y of G1Affine::from_bytes(point32), or None where it fails: x >= p, the identity flag (the identity's own
    encoding decodes in the reference, but is no point of a proof: the verifier refuses it either way), x^3 + 3 not a square"""
    b = bytearray(point32)
    assert len(b) == 32
    flags = b[31]
    b[31] &= 0x3f
    x = int.from_bytes(b, "little")
    if x >= P or flags & FLAG_IDENTITY:
        return None
    rhs = (x ** 3 + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    if (y & 1) != (1 if flags & FLAG_SIGN else 0):   # (y = 0 does not occur: G1 has prime order)
        y = P - y
    return y


def is_hit(point32, hint32):
    """a hint is USED exactly when the point decodes and the hint's 32 bytes equal its canonical y"""
    y = decode(point32)
    return y is not None and bytes(hint32) == le32(y)


def points_of(offsets, proof):
    return [bytes(proof[o:o + 32]) for o in offsets]


def rows(offsets, proofs):
    """the hint rows of whole proofs: per proof the canonical y of its points in the order of `offsets`, 32 zero bytes for a point
    that does not decode -> bytes"""
    return b"".join(le32(decode(pt) or 0) for proof in proofs for pt in points_of(offsets, proof))


def count_misses(points, hints32):
    """points: the compressed points in launch order (proof-major); hints32: 32 bytes per point -> the number of hints not used"""
    return sum(0 if is_hit(pt, hints32[32 * i:32 * i + 32]) else 1 for i, pt in enumerate(points))


def hint_set(kind, points, seed=0):
    """One of HINT_SETS over the points (compressed, in launch order: lane t of the decompression owns point t) -> 32 bytes per point.
      right        the canonical y (zeros where the point does not decode)
      zero         all zero
      other_root   p - y: on the curve, the wrong parity
      plus_p       y + p: the right residue, not canonical (every y + p is below 2^256)
      random       seeded random bytes
      lane0_wrong  right, except the first point of every wave of 64: one miss per wave, the worst case of the in-kernel fallback
      even_lanes   right on even points, zero on odd ones"""
    assert kind in HINT_SETS, kind
    rnd = random.Random(seed)
    out = []
    for t, pt in enumerate(points):
        y = decode(pt)
        right = le32(y or 0)
        if kind == "right":
            h = right
        elif kind == "zero":
            h = bytes(32)
        elif kind == "other_root":
            h = le32(P - y) if y is not None else bytes(32)
        elif kind == "plus_p":
            h = le32(y + P) if y is not None else bytes(32)
        elif kind == "random":
            h = bytes(rnd.randrange(256) for _ in range(32))
        elif kind == "lane0_wrong":
            h = le32((y or 0) ^ 2) if t % WAVE == 0 else right      # (a flipped bit that keeps the parity: only the curve check can tell)
        else:
            h = right if t % 2 == 0 else bytes(32)
        out.append(h)
    return b"".join(out)


def non_residue_x(start=1):
    """the first x >= start with x^3 + 3 a non-residue: a compressed point that does not decode"""
    x = start
    while pow((x ** 3 + 3) % P, (P - 1) // 2, P) != P - 1:
        x += 1
    return x


def random_point(rnd):
    """a random decodable compressed point with a random sign flag"""
    while True:
        pt = encode(rnd.randrange(P), rnd.randrange(2))
        if decode(pt) is not None:
            return pt
