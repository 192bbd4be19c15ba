"""The device code of the field products (csrc/bn254.hip.h: mul_inl, sqr_inl, dot2_inl, sqdot_inl and the chained forms mul_chain, sqr_chain,
dot2_chain, sqdot_chain of field_chain.hip.h), for Fq and Fr, limb by limb against Python big integers.  build/field_units (tests/cpp/field_units.hip,
built by csrc/Makefile with the library's flags) runs one workgroup of 64 lanes per launch, each lane one operand tuple of
tests/field_units_reference.py: non-canonical representatives, the fullest columns, single limbs, lazy forms up to 8p, equal operands
and seeded random ones.  Every comparison is exact; the two forms must also agree with each other limb for limb.  The further groups of the
program put the rest of the header through the AMDGPU back end in the same way: sums, differences and the lazy linear forms, from_wide,
the conversions, the inverses and powers, and the square roots of curve.hip.h (the loop forms in both product forms)."""
import os
import subprocess

import pytest

import field_units_reference as fu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "halo2_verifier_amd", "csrc", "build", "field_units")
ROUTINES = {"mul_inl": "mul", "mul_chain": "mul", "sqr_inl": "sqr", "sqr_chain": "sqr", "dot2_inl": "dot2", "dot2_chain": "dot2", "sqdot_inl": "sqdot", "sqdot_chain": "sqdot"}


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_device_products_match_big_integers_in_both_forms(field):
    assert os.path.exists(EXE), EXE + " is missing: build() makes it (halo2_verifier_amd/csrc/Makefile)"
    tup = fu.tuples(field)
    r = subprocess.run([EXE, field, "gpu"], input=fu.encode(tup), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = fu.parse(r.stdout.decode(), list(ROUTINES))
    fu.check(field, tup, got, ROUTINES)
    for k, (t, g) in enumerate(zip(tup, got)):
        if t[1] == t[2]:
            assert g["mul_chain"] == g["sqr_chain"] and g["mul_inl"] == g["sqr_inl"], f"{field} tuple {k}: a product of equal operands is not the squaring"


@pytest.mark.parametrize("group,field", [(g, f) for g, fields in fu.FIELDS.items() for f in fields])
def test_device_group_matches_big_integers(group, field):
    """the rest of the header on the device (field_units FIELD gpu GROUP): the linear forms, from_wide, the conversions, the inverses and powers
    and the three square roots, on the cases that test_field_units_host.py puts through the host code, against the same models, exactly"""
    assert os.path.exists(EXE), EXE + " is missing: build() makes it (halo2_verifier_amd/csrc/Makefile)"
    g = fu.GROUPS[group]
    cases = g["cases"](field)
    r = subprocess.run([EXE, field, "gpu", group], input=g["encode"](cases), capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    fu.check_group(field, group, cases, fu.parse_group(r.stdout.decode(), group, device=True), device=True)
