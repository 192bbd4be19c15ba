"""The C++ mirror at the trait seam (include/h2v.hpp Accumulator::process_guards, check_guards): tests/cpp/guards_harness.cpp feeds one
resident accumulator proofs through process and then the CPU oracle's Guards through process_guards, and another one Guards alone;
both must equal the library's one verify_batch and the CPU oracle over all the proofs, and the verdicts per Guard the oracle's
verify_single proof by proof."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_guards_equal_process_and_the_oracle(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("guards_harness", tmp_path)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 9, seed=61, threads=4)
    rnd = random.Random(62)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    ch.write_dir(tmp_path, s.params, vks=[s.vk], rand=rand)
    for case in ("good", "bad"):
        if case == "bad":   # a wrong public input in the Guards' leg: its Guard's own check fails, and with it the one pairing
            I[6] = [[circuits.le32(5)] + I[6][0][1:]]
        guards = []
        for p, inst in zip(P, I):
            rc, g = circuits.oracle_guard(s, p, inst)
            assert rc == 0
            guards.append(g)
        ch.write_dir(tmp_path, items_txt=ch.items_text(P, I, keys=[0] * len(P)), guards_txt=ch.guards_text(guards))
        for cut in (4, 0):
            out = ch.run(exe, [tmp_path, cut]).stdout.splitlines()
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
