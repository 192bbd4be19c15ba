"""The field header csrc/bn254.hip.h on the HOST against the big-integer models of tests/field_units_reference.py, on the very cases
test_gpu_field_units.py gives the device code: a disagreement on the GPU then points at the device code and not at the model.  The
products (mul_inl, sqr_inl, dot2_inl, sqdot_inl) limb by limb, and the further groups of tests/cpp/field_units.hip: the corrected and
lazy linear forms, from_wide, the conversions, the inverses and powers, and the straight-line square root of curve.hip.h.  Every
comparison is exact.  No GPU needed."""
import os
import re
import subprocess

import pytest

import field_units_reference as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTINES = {"mul_inl": "mul", "sqr_inl": "sqr", "dot2_inl": "dot2", "sqdot_inl": "sqdot"}
GROUP_FIELDS = [(g, f) for g, fields in fu.FIELDS.items() for f in fields]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("field_units") / "field_units"
    src = os.path.join(ROOT, "tests", "cpp", "field_units.hip")
    r = subprocess.run(["hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-o", str(out), src], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail("hipcc failed: " + r.stderr[-2000:])
    return str(out)


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_host_products_match_big_integers(exe, field):
    tup = fu.tuples(field)
    r = subprocess.run([exe, field, "host"], input=fu.encode(tup), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = fu.parse(r.stdout.decode(), list(ROUTINES))
    fu.check(field, tup, got, ROUTINES)
    for k, (t, g) in enumerate(zip(tup, got)):
        if t[1] == t[2]:
            assert g["mul_inl"] == g["sqr_inl"], f"{field} tuple {k}: the product of equal operands is not the squaring"


def test_limbs_of_2_to_29_or_more_are_refused(exe):
    bad = b"\x00\x00\x00\x20" + bytes(4 * 35)
    r = subprocess.run([exe, "fq", "host"], input=bad, capture_output=True, timeout=300)
    assert r.returncode == 2


@pytest.mark.parametrize("group,field", GROUP_FIELDS)
def test_host_group_matches_big_integers(exe, group, field):
    g = fu.GROUPS[group]
    cases = g["cases"](field)
    r = subprocess.run([exe, field, "host", group], input=g["encode"](cases), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    fu.check_group(field, group, cases, fu.parse_group(r.stdout.decode(), group, device=False), device=False)


@pytest.mark.parametrize("group", [g for g in fu.GROUPS if g != "wide"])
def test_a_group_refuses_limbs_of_2_to_29_or_more(exe, group):
    g = fu.GROUPS[group]
    blob = bytearray(g["encode"](g["cases"]("fq")[:1]))
    blob[32:36] = b"\x00\x00\x00\x20"            # the top limb of the first operand
    r = subprocess.run([exe, "fq", "host", group], input=bytes(blob), capture_output=True, timeout=300)
    assert r.returncode == 2 and "bad input" in r.stderr.decode()


def test_the_roots_are_of_fq_alone_and_an_unknown_group_is_usage(exe):
    for args in (["fr", "host", "root"], ["fq", "host", "no_such_group"], ["fq", "host", "linear", "more"]):
        r = subprocess.run([exe] + args, input=b"", capture_output=True, timeout=300)
        assert r.returncode == 2 and r.stderr.decode().startswith("usage: field_units"), (args, r.returncode, r.stderr)


def test_every_lazy_lin_the_library_instantiates_is_in_the_linear_group():
    csrc = os.path.join(ROOT, "halo2_verifier_amd", "csrc")
    found = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(csrc, name)) as f:
                found |= {tuple(int(x) for x in m) for m in re.findall(r"lazy_lin<\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*>", f.read())}
    assert found == set(fu.LAZY_FORMS.values()), found ^ set(fu.LAZY_FORMS.values())
    with open(os.path.join(ROOT, "tests", "cpp", "field_units.hip")) as f:
        src = f.read()
    for name in fu.LAZY_FORMS:
        assert '{"%s", 9, false}' % name in src, name


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_the_pinned_from_wide_cases_take_the_correction_step(field):
    d = (fu.P[field] >> 232) + 1
    m = (1 << 40) // d
    for top in fu.WIDE_CORRECTION_TOPS:
        assert top < 1 << 29 and (top * m) >> 40 == top // d - 1, hex(top)
    for top in fu.WIDE_EXACT_TOPS:
        assert top < 1 << 29 and (top * m) >> 40 == top // d, hex(top)
    cases = fu.wide_cases(field)
    kinds = {c: [fu.wide_corrects(field, acc) for k, acc in cases if k == c] for c in ("correction", "no correction")}
    assert len(kinds["correction"]) >= 8 and all(kinds["correction"]) and kinds["no correction"] and not any(kinds["no correction"])
    assert {(fu.wide_top(field, acc)) for k, acc in cases if k == "correction"} == set(fu.WIDE_CORRECTION_TOPS)


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_the_models_hold_their_own_bounds(field):
    p = fu.P[field]
    for bad in (lambda: fu.lazy_lin(field, 2, 0, 1, 0, 2 * p + 1),            # 2p - d below zero
                lambda: fu.lazy_lin(field, 0, -2, 0, fu.R // 2, 0),           # 2c of 2^261 or more
                lambda: fu.lazy_lin(field, 8, 1, 2, 4 * p, 2 * p + 1),
                lambda: fu.from_wide(field, [-1] + [0] * 8),                  # V below zero
                lambda: fu.from_wide(field, [0] * 8 + [1 << 29]),             # V of 2^261 or more
                lambda: fu.from_wide(field, [1 << 63] + [0] * 8),             # an accumulator that is no int64
                lambda: fu.add(field, 2 * p, 0), lambda: fu.sub(field, 0, 2 * p), lambda: fu.canonical(field, 2 * p),
                lambda: fu.from_raw(field, 1 << 256)):
        with pytest.raises(AssertionError):
            bad()
    # the largest value from_wide takes still comes out below 2p (the model asserts it), and so does every top limb's worst case
    d = (p >> 232) + 1
    for top in (d - 1, 2 * d - 1, 169 * d - 1, (1 << 29) - 1):
        assert fu.from_wide(field, fu.limbs(top << 232 | ((1 << 232) - 1))) < 2 * p
    c = fu.consts(field)
    assert fu.mont(field, c["R2"]) == c["ONE"] and fu.mont(field, c["ONE"]) == 1
