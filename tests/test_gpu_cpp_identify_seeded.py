"""The C++ mirror (include/h2v.hpp) of identification on a SEEDED accumulation: tests/cpp/identify_seeded.cpp resumes the first half's
accumulator with AccumulatorStrategy::with, queues the second half and finalize_identify() runs h2v_verify_batch_seeded_identify.  The
printed verdict, channels, statuses and the seed's own verdict are compared with the CPU oracle."""
import os
import random
import subprocess

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_finalize_identify_on_a_seeded_accumulation(tmp_path):
    from halo2_verifier_amd import _lib
    lib = _lib.lib_path()
    exe = tmp_path / "identify_seeded"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "identify_seeded.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 12, seed=85, threads=4)
    rnd = random.Random(87)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    d = tmp_path
    (d / "params.bin").write_bytes(s.params)
    (d / "vk.bin").write_bytes(s.vk)
    (d / "rand.bin").write_bytes(b"".join(r.to_bytes(32, "little") for r in rand[6:]))

    def run(P, I):
        _, _, left, right = circuits.oracle_verify_batch(s, P[:6], I[:6], rand[:6])
        (d / "seed.bin").write_bytes(left + right)
        lines = [f"{len(P) - 6}"]
        for p, inst in zip(P[6:], I[6:]):
            flat = b"".join(v for col in inst for v in col)
            lines.append(" ".join([str(len(inst))] + [str(len(c)) for c in inst] + [p.hex(), flat.hex() or "-"]))
        (d / "items.txt").write_text("\n".join(lines) + "\n")
        out = subprocess.run([str(exe), str(d)], check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
        return out, circuits.oracle_pairing_check(s, left, right)

    for case in ("good", "bad_second_half", "bad_seed"):
        Pc, Ic = list(P), list(I)
        if case == "bad_second_half":   # a wrong public input: only the pairing rejects it
            Ic[9] = [[circuits.le32(5)] + I[9][0][1:]]
        if case == "bad_seed":
            Ic[2] = [[circuits.le32(5)] + I[2][0][1:]]
        out, seed_passes = run(Pc, Ic)
        ok, st, left, right = circuits.oracle_verify_batch(s, Pc, Ic, rand)   # the whole accumulation: what the resumed one must equal
        assert ok is (case == "good") and st == [0] * 12 and seed_passes is (case != "bad_seed")
        single = [circuits.oracle_verify_single(s, p, i) for p, i in zip(Pc[6:], Ic[6:])]
        assert single == ([0, 0, 0, -2, 0, 0] if case == "bad_second_half" else [0] * 6)
        m = [l for l in out if l.startswith("identify ")][0].split()
        assert (m[1] == "1") == ok and bytes.fromhex(m[2]) == left and bytes.fromhex(m[3]) == right
        assert [int(x) for x in m[4:]] == single
        assert f"seed_ok {int(seed_passes)}" in out
        checks = int([l for l in out if l.startswith("range_checks ")][0].split()[1])
        assert (checks > 0) == (case == "bad_second_half")
        plain = [l for l in out if l.startswith("plain ")][0].split()
        assert plain[1:] == m[1:4]
    s.free()
