"""The C++ form of the field products (csrc/bn254.hip.h: mul_inl, sqr_inl, dot2_inl, sqdot_inl) on the HOST, limb by limb against the big-integer
model of tests/field_units_reference.py, on the very tuples test_gpu_field_units.py gives the device code: a disagreement on the GPU
then points at the device code and not at the model.  No GPU needed."""
import os
import subprocess

import pytest

import field_units_reference as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTINES = {"mul_inl": "mul", "sqr_inl": "sqr", "dot2_inl": "dot2", "sqdot_inl": "sqdot"}


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
