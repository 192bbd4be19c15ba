"""The C++ mirror (include/h2v.hpp) of identification over proofs of two VerifyingKeys: tests/cpp/identify_keys.cpp queues them on
one AccumulatorStrategy in call order and finalize_identify_keys() runs h2v_verify_batch_keys_identify.  The printed verdict,
channels and statuses are compared with the CPU oracle."""
import os
import random
import subprocess

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_finalize_identify_keys_over_two_vks(tmp_path):
    from halo2_verifier_amd import _lib
    lib = _lib.lib_path()
    exe = tmp_path / "identify_keys"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "identify_keys.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 6, seed=81, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 6, seed=82, threads=4)
    items = []
    for j in range(6):
        items += [(s8, P8[j], I8[j]), (s4, P4[j], I4[j])]
    rnd = random.Random(83)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    d = tmp_path
    (d / "params.bin").write_bytes(s8.params)
    (d / "vk0.bin").write_bytes(s8.vk)
    (d / "vk1.bin").write_bytes(s4.vk)
    (d / "rand.bin").write_bytes(b"".join(r.to_bytes(32, "little") for r in rand))

    def run(items):
        lines = [f"2 {len(items)}"]
        for s, p, inst in items:
            flat = b"".join(v for col in inst for v in col)
            lines.append(" ".join([str(0 if s is s8 else 1), str(len(inst))] + [str(len(c)) for c in inst] + [p.hex(), flat.hex() or "-"]))
        (d / "items.txt").write_text("\n".join(lines) + "\n")
        return subprocess.run([str(exe), str(d)], check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()

    for case in ("good", "bad"):
        if case == "bad":   # a wrong public input on the second key: only the pairing rejects it
            items[7] = (s4, P4[3], [[circuits.le32(5)] + I4[3][0][1:]])
        out = run(items)
        ok, st, left, right = circuits.oracle_accumulate(items, rand)
        assert ok is (case == "good") and st == [0] * len(items)
        single = [circuits.oracle_verify_single(s, p, i) for s, p, i in items]
        assert single == ([0] * len(items) if case == "good" else [0] * 7 + [-2] + [0] * 4)
        m = [l for l in out if l.startswith("identify ")][0].split()
        assert (m[1] == "1") == ok and bytes.fromhex(m[2]) == left and bytes.fromhex(m[3]) == right
        assert [int(x) for x in m[4:]] == single
        checks = int([l for l in out if l.startswith("range_checks ")][0].split()[1])
        assert (checks == 0) == (case == "good")
        assert "identify_refused -19" in out   # finalize_identify keeps its one-VK contract
    s8.free(); s4.free()
