"""The C++ mirror (include/h2v.hpp) of identification on a SEEDED accumulation: tests/cpp/identify_seeded.cpp resumes the first half's
accumulator with AccumulatorStrategy::with, queues the second half and finalize_identify() runs h2v_verify_batch_seeded_identify.  The
printed verdict, channels, statuses and the seed's own verdict are compared with the CPU oracle."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_finalize_identify_on_a_seeded_accumulation(tmp_path):
    exe = ch.build("identify_seeded", tmp_path)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 12, seed=85, threads=4)
    rnd = random.Random(87)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand[6:])

    def run(P, I):
        _, _, left, right = circuits.oracle_verify_batch(s, P[:6], I[:6], rand[:6])
        ch.write_dir(d, seed_bin=left + right, items_txt=ch.items_text(P[6:], I[6:]))
        out = ch.run(exe, [d]).stdout.splitlines()
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
