"""The command lines of the five kernel unit harnesses (tests/cpp/*_units.hip over tests/cpp/units.h): without arguments or with an
unknown mode a program prints a usage line that names every mode and ends with status 2, and a file-reading mode given an empty
input file ends with status 2 and "input too short" — both before any HIP call, so no GPU is needed.  A program that is not built
is skipped."""
import os

import pytest

import units_harness as uh

# program -> (its modes, the operands before IN OUT of each)
PROGRAMS = {
    "msm_units": {m: [] for m in ["law", "digits", "msm", "scale"]},
    "pairing_units": {"step": [], "check": [], "lines": ["PARAMS"], "verdict": ["PARAMS"], "tail": ["PARAMS"]},
    "verify_units": {m: [] for m in ["decompress", "stream", "insteval", "frvm", "fold", "multipliers", "gather", "ragged"]},
    "util_units": {m: [] for m in ["fold", "export", "to_bytes", "bases", "scalars", "to_jacobian", "copy", "merge_fold"]},
    "field_units": {m: None for m in ["fq", "fr", "gpu", "host", "products", "linear", "wide", "convert", "inverse", "root"]},      # (text over stdin: no file-reading mode)
}


def _built(name):
    path = os.path.join(uh.ROOT, "halo2_verifier_amd", "csrc", "build", name)
    if not os.path.exists(path):
        pytest.skip(path + " is not built")


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_usage_names_every_mode(name):
    _built(name)
    r = uh.start(name, [])
    assert r.returncode == 2, (r.returncode, r.stderr)
    usage = [l for l in r.stderr.splitlines() if l.startswith("usage: " + name)]
    assert len(usage) == 1, r.stderr
    named = set(usage[0].replace("|", " ").split())
    assert set(PROGRAMS[name]) <= named, (sorted(set(PROGRAMS[name]) - named), usage[0])
    r = uh.start(name, ["no_such_mode", "a", "b"])
    assert r.returncode == 2 and "usage: " + name in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("name,mode", [(n, m) for n in sorted(PROGRAMS) for m, pre in PROGRAMS[n].items() if pre is not None])
def test_empty_input_is_too_short(name, mode, tmp_path):
    _built(name)
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    out = tmp_path / "out.bin"
    r = uh.start(name, [mode] + [empty] * len(PROGRAMS[name][mode]) + [empty, out])
    assert r.returncode == 2 and "input too short" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()
