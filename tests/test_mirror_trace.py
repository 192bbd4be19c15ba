"""The host mirrors hand the C ABI today what they handed it when the fixtures were recorded: every call, every argument, every return
value and every refusal.  Python: tests/mirror_trace.py records halo2_verifier_amd through a stand-in library.  C++: tests/cpp/mirror_trace.cpp
walks include/h2v.hpp over tests/cpp/h2v_stub.cpp, built with the address and undefined-behaviour sanitizers.  No GPU, no real library."""
import json
import os

import pytest

import caller_harness as ch
import mirror_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def recorded():
    return mirror_trace.record()


@pytest.fixture(scope="module")
def fixture():
    with open(mirror_trace.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_and_the_scenario_list_agree(recorded, fixture):
    for kind in ("scenarios", "refusals"):
        assert sorted(recorded[kind]) == sorted(fixture[kind])


@pytest.mark.parametrize("name", sorted(mirror_trace.scenarios()))
def test_python_mirror_sends_what_it_sent(recorded, fixture, name):
    got, want = recorded["scenarios"][name], fixture["scenarios"][name]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]   # the entry points reached, in order
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got["returned"] == want["returned"]


def test_python_mirror_refuses_what_it_refused(recorded, fixture):
    assert all(v[0] in ("ValueError", "TypeError") for v in fixture["refusals"].values())
    for name, want in fixture["refusals"].items():
        assert recorded["refusals"][name] == want, name


def test_recording_leaves_the_loaded_library_alone():
    from halo2_verifier_amd import _lib
    before = _lib._LIB
    mirror_trace.record()
    assert _lib._LIB is before


def test_cpp_mirror_sends_what_it_sent(tmp_path):
    exe = ch.build("mirror_trace", tmp_path, sanitize=True, stubs=("h2v_stub",))
    out = ch.run(exe, timeout=120).stdout
    with open(os.path.join(GOLDEN, "mirror_calls_cpp.txt")) as f:
        want = f.read()
    assert out.splitlines() == want.splitlines()
