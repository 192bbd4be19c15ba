"""tests/record_reference.py held against what the project already trusts: msm_reference's weighted sums, the oracle library's
point encoding and scalar canonicity (Fr::from_repr behind h2o_g1_msm).  No GPU."""
import ctypes
import random

import msm_reference as ref
import oracle_lib
import record_reference as rr
from msm_reference import P, R
from srs_util import g1_xy


def _points(seed, count):
    rnd = random.Random(seed)
    return [ref.mul(rnd.randrange(1, R), ref.G) for _ in range(count)], rnd


def test_exported_span_is_below_the_bound():
    """every cut a launch can export asks for at most 128 doublings, and the bound the fold accepts leaves room above it"""
    assert rr.max_exported_span() == 128 <= rr.MAX_SPAN
    import pairing_reference as pr
    assert max(s * (k - 1) for s, k in pr.msm_split_pairs()) == rr.max_exported_span()


def test_fold_equals_the_weighted_sum_of_all_pieces():
    """a fold of well-formed records — of the fold's cut and of others — stands for the sum of every piece with its weight"""
    pts, rnd = _points(11, 40)
    for parts, shift in ((1, 0), (2, 65), (3, 44), (6, 22)):
        cuts = [(parts, shift), (parts, shift + 1 if parts > 1 else 7), (max(1, parts - 1), 5), (min(6, parts + 1), 2), (1, 0), (6, 43)]
        recs, scalars, points = [], [[], []], [[], []]
        for i, (k, sh) in enumerate(cuts * 2):
            sides = []
            for s in (0, 1):
                ps = [rnd.choice(pts + [None]) for _ in range(k)]
                sides.append(ps)
                scalars[s] += [pow(2, sh * j, R) for j in range(k)]
                points[s] += ps
            recs.append([rr.Record(i, k, sh, sides[0], sides[1])])
        pieces, failed = rr.fold(recs, 1, parts, shift)
        assert failed == [sum(range(len(recs)))]
        for s in (0, 1):
            assert rr.folded_value(pieces[0][s], shift) == ref.msm(scalars[s], points[s])
        kinds = {rr.record_kind(r[0], parts, shift) for r in recs}
        assert kinds == {"same", "foreign"}


def test_malformed_records_and_saturation():
    g = ref.G
    for bad in (rr.Record(0, 0, 0, [], []), rr.Record(0, 7, 0, [g] * 6, [g] * 6), rr.Record(3, 2, rr.MAX_SPAN + 1, [g, g], [g, g]),
                rr.Record(0, 6, 52, [g] * 6, [g] * 6)):
        assert rr.record_kind(bad, 1, 0) == "malformed"
        pieces, failed = rr.fold([[bad], [rr.Record(0, 1, 0, [g], [g])]], 1, 1, 0)
        assert pieces[0][0][0] == g and failed == [max(bad.failed, 1)]
    assert rr.record_kind(rr.Record(0, 2, rr.MAX_SPAN, [g, g], [g, g]), 1, 0) == "foreign"
    assert rr.record_kind(rr.Record(0, 2, 1000, [g, g], [g, g]), 2, 1000) == "same"          # nothing is put together: no bound
    assert rr.record_kind(rr.Record(0, 1, 0xffffffff, [g], [g]), 3, 44) == "foreign"          # a whole point has no doublings
    half = rr.Record(0x80000000, 1, 0, [g], [g])
    assert rr.fold([[half], [half]], 1, 1, 0)[1] == [0xffffffff]
    assert rr.fold([[half], [half], [half]], 1, 1, 0)[1] == [0xffffffff]


def test_point_bytes_round_trip_and_agree_with_the_oracle(srs, oracle):
    """to_bytes and from_bytes are inverse on the SRS points, and the bytes are the oracle's: h2o_g1_msm reads them as the same points
    (1 * P comes back as the same bytes, P + Q as those of the reference's sum)"""
    pts = srs.g[:32]
    for i, pt in enumerate(pts):
        b, ident = rr.point_to_bytes(pt)
        assert ident == 0 and b == g1_xy(pt) and rr.point_from_bytes(b) == (pt, 0)
        assert oracle_lib.g1_msm(oracle, [1], [b]) == b
        assert oracle_lib.g1_msm(oracle, [1, 1], [b, rr.point_to_bytes(pts[i - 1])[0]]) == rr.point_to_bytes(ref.add(pt, pts[i - 1]))[0]
    assert rr.point_to_bytes(None) == (bytes(64), 1) and rr.point_from_bytes(bytes(64)) == (None, 0)
    assert oracle_lib.g1_msm(oracle, [0], [rr.point_to_bytes(pts[0])[0]]) == bytes(64)
    x, y = pts[3]
    for bad in ((x, (y + 1) % P), (x, 0), (0, y), (P, y), (x, P), (x + P, y) if x + P < 1 << 256 else (P, y), (x | 1 << 255, y)):
        assert rr.point_from_bytes(bad[0].to_bytes(32, "little") + bad[1].to_bytes(32, "little")) == (None, 1), bad
    # the oracle refuses the off-curve encodings as well (-2)
    out, ident = ctypes.create_string_buffer(64), ctypes.c_int(0)
    for bad in ((x, (y + 1) % P), (x, 0), (0, y)):
        bb = bad[0].to_bytes(32, "little") + bad[1].to_bytes(32, "little")
        assert oracle.h2o_g1_msm((1).to_bytes(32, "little"), bb, 1, out, ctypes.byref(ident)) == -2


def scalar_edges():
    vals = [0, 1, R - 1, R, R + 1, 1 << 254, (1 << 256) - 1]
    for k in range(8):
        vals += [R + (1 << (32 * k)), R - (1 << (32 * k))]
    return vals


def test_scalar_canonicity_agrees_with_the_oracle(srs, oracle):
    """refused exactly when the oracle's Fr::from_repr refuses (h2o_g1_msm returns -1 for a scalar it cannot read)"""
    base = g1_xy(srs.g[0])
    out, ident = ctypes.create_string_buffer(64), ctypes.c_int(0)
    rnd = random.Random(5)
    seen = set()
    for v in scalar_edges() + [rnd.randrange(1 << 256) for _ in range(50)]:
        b = v.to_bytes(32, "little")
        words, flag = rr.scalar_from_bytes(b)
        rc = oracle.h2o_g1_msm(b, base, 1, out, ctypes.byref(ident))
        assert (rc == -1) == (flag == 1) and rc in (0, -1), hex(v)
        assert flag == (1 if v >= R else 0)
        assert words == ([0] * 8 if flag else [(v >> (32 * i)) & 0xffffffff for i in range(8)])
        seen.add(flag)
    assert seen == {0, 1}
