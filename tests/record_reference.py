"""Big-integer reference for the record, byte-conversion and launch-tail kernels (halo2_verifier_amd/csrc/util.hip,
k_gather_multipliers in verify_kernels.hip, pair_tail_role in pairing.hip), written from their definitions in include/h2v.h and
csrc/internal.h over the affine G1 arithmetic and the limb helpers of tests/msm_reference.py.  Nothing here ports a kernel.

A record ([failed, parts, shift, reserved][left piece 0 .. 5][right piece 0 .. 5], H2V_ACC_RECORD_BYTES) stands per side for
    sum_j 2^(shift j) piece_j,   j < parts.
A fold into (parts, shift) adds records of that cut piece by piece; a well-formed record of another cut is put together and joins
piece 0 (weight 1); a malformed record — parts outside 1 .. 6, or a foreign cut with shift (parts - 1) > MAX_SPAN — contributes
the identity and counts as max(failed, 1) failed proofs.  The failure count of a group saturates at 2^32 - 1."""
import msm_reference as ref
from msm_reference import P, R

FQ_P = P
FR_R = R
PIECES = 6                  # include/h2v.h H2V_ACC_RECORD_PIECES
RECORD_WORDS = 4 + 2 * PIECES * 27
MAX_SPAN = 256              # csrc/util.hip ACC_RECORD_MAX_SPAN; what a launch exports stays at or below max_exported_span() = 128
U32 = 0xffffffff
IDENTITY_WORDS = ref.fq_words(0) + ref.fq_words(1) + ref.fq_words(0)


def max_exported_span():
    """the largest shift (parts - 1) over every cut a launch can export (csrc/msm.hip: msm_plan's c in 2 .. 15 with ceil(130 / c)
    windows, cut into parts of wpp = ceil(windows / want) windows, want in 2 .. 6, shift = c wpp)"""
    best = 0
    for c in range(2, 16):
        w = (130 + c - 1) // c
        for want in range(2, PIECES + 1):
            wpp = (w + want - 1) // want
            best = max(best, c * wpp * ((w + wpp - 1) // wpp - 1))
    return best


# ------------------------------------------------------------------ records
class Record:
    """one record as the fold sees it: header words and the affine points (None: the identity) its 2 x 6 pieces stand for"""
    def __init__(self, failed, parts, shift, left, right, reserved=0):
        self.failed, self.parts, self.shift, self.reserved = failed, parts, shift, reserved
        self.left = list(left) + [None] * (PIECES - len(left))
        self.right = list(right) + [None] * (PIECES - len(right))
        assert len(self.left) == PIECES and len(self.right) == PIECES

    def side(self, s):
        return self.right if s else self.left


def weighted_sum(pieces, shift):
    """sum_j 2^(shift j) pieces[j]"""
    acc = None
    for j, pt in enumerate(pieces):
        acc = ref.add(acc, ref.mul(pow(2, shift * j, R), pt))
    return acc


def record_value(rec, side):
    return weighted_sum(rec.side(side)[:rec.parts], rec.shift)


def record_kind(rec, parts, shift):
    """'same' (adds piece by piece), 'foreign' (put together, joins piece 0) or 'malformed'"""
    if not 1 <= rec.parts <= PIECES:
        return "malformed"
    if rec.parts == parts and (rec.shift == shift or parts == 1):
        return "same"
    return "foreign" if rec.shift * (rec.parts - 1) <= MAX_SPAN else "malformed"


def fold(recs, groups, parts, shift):
    """recs[i][g] -> (pieces[g][side][j] as affine points, failed[g])"""
    pieces = [[[None] * parts for _ in range(2)] for _ in range(groups)]
    failed = [0] * groups
    for row in recs:
        assert len(row) == groups
        for g, rec in enumerate(row):
            kind = record_kind(rec, parts, shift)
            for s in (0, 1):
                if kind == "same":
                    for j in range(parts):
                        pieces[g][s][j] = ref.add(pieces[g][s][j], rec.side(s)[j])
                elif kind == "foreign":
                    pieces[g][s][0] = ref.add(pieces[g][s][0], record_value(rec, s))
            failed[g] = min(U32, failed[g] + (rec.failed if kind != "malformed" else max(rec.failed, 1)))
    return pieces, failed


def folded_value(pieces_gs, shift):
    return weighted_sum(pieces_gs, shift)


def export_header(statuses, parts, shift):
    """the four header words of an exported record: the non-zero statuses of the group's proofs, the cut, 0"""
    return [sum(1 for s in statuses if s != 0), parts, shift, 0]


def ready_of(words27):
    """(X Z, Y, Z^3) as field values of a stored Jacobian point"""
    X, Y, Z = (ref.fq_value(words27[9 * i:9 * i + 9]) for i in range(3))
    return (X * Z % P, Y, Z * Z * Z % P)


def values_of(words27):
    return tuple(ref.fq_value(words27[9 * i:9 * i + 9]) for i in range(3))


def in_range(words, coords=3):
    return all(ref.fq_in_range(words[9 * i:9 * i + 9]) for i in range(coords))


# ------------------------------------------------------------------ bytes
def point_to_bytes(pt):
    """-> (64 bytes x | y little-endian canonical, identity flag)"""
    return (bytes(64), 1) if pt is None else (pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"), 0)


def point_from_bytes(b):
    """64 bytes -> (point, flag): all zero is the identity (flag 0); a coordinate not below p or a point off the curve is refused
    (flag 1, the identity)"""
    assert len(b) == 64
    if b == bytes(64):
        return None, 0
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
    if x >= P or y >= P or (y * y - x * x * x - 3) % P:
        return None, 1
    return (x, y), 0


def scalar_from_bytes(b):
    """32 bytes -> (eight 32-bit words, flag): a value not below r is refused (flag 1, zero words)"""
    v = int.from_bytes(b, "little")
    if v >= R:
        return [0] * 8, 1
    return [(v >> (32 * i)) & U32 for i in range(8)], 0
