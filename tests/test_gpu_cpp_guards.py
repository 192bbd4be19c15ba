"""The C++ mirror at the trait seam (include/h2v.hpp Accumulator::process_guards, check_guards): tests/cpp/guards_harness.cpp feeds one
resident accumulator proofs through process and then the CPU oracle's Guards through process_guards, and another one Guards alone;
both must equal the library's one verify_batch and the CPU oracle over all the proofs, and the verdicts per Guard the oracle's
verify_single proof by proof."""
import os
import random
import subprocess

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_guards_equal_process_and_the_oracle(tmp_path):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import _lib
    lib = _lib.lib_path()
    exe = tmp_path / "guards_harness"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "guards_harness.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 9, seed=61, threads=4)
    rnd = random.Random(62)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    (tmp_path / "params.bin").write_bytes(s.params)
    (tmp_path / "vk0.bin").write_bytes(s.vk)
    (tmp_path / "rand.bin").write_bytes(b"".join(r.to_bytes(32, "little") for r in rand))
    for case in ("good", "bad"):
        if case == "bad":   # a wrong public input in the Guards' leg: its Guard's own check fails, and with it the one pairing
            I[6] = [[circuits.le32(5)] + I[6][0][1:]]
        lines = [f"1 {len(P)}"]
        guards = []
        for p, inst in zip(P, I):
            flat = b"".join(v for col in inst for v in col)
            lines.append(" ".join(["0", str(len(inst))] + [str(len(c)) for c in inst] + [p.hex(), flat.hex() or "-"]))
            rc, g = circuits.oracle_guard(s, p, inst)
            assert rc == 0
            guards.append(" ".join(b"".join(g[k]).hex() or "-" for k in ("left_scalars", "left_bases", "right_scalars", "right_bases")))
        (tmp_path / "items.txt").write_text("\n".join(lines) + "\n")
        (tmp_path / "guards.txt").write_text("\n".join(guards) + "\n")
        for cut in (4, 0):
            out = subprocess.run([str(exe), str(tmp_path), str(cut)], check=True, capture_output=True, text=True, timeout=300).stdout.splitlines()
            exp = circuits.oracle_verify_batch(s, P, I, rand)
            assert ctx.verify_batch(P, I, rand) == exp and exp[0] is (case == "good")
            for name in ("mixed", "guards"):
                m = [l for l in out if l.startswith(name + " ")][0].split()
                assert (m[1] == "1", bytes.fromhex(m[2]), bytes.fromhex(m[3]), int(m[4]), int(m[5])) == (exp[0], exp[2], exp[3], len(P), 0), (case, cut, name)
            each = [l for l in out if l.startswith("each")][0].split()[1:]
            assert [e == "1" for e in each] == [circuits.oracle_verify_single(s, p, i) == 0 for p, i in zip(P, I)]
            assert "refused" in out
    ctx.close()
    s.free()
