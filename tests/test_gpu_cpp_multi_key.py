"""The C++ mirror (include/h2v.hpp) over proofs of two VerifyingKeys: tests/cpp/multi_key.cpp queues them on one
AccumulatorStrategy in call order, exactly as the reference's loop of verify_proof calls would, and finalize() runs
h2v_verify_batch_keys.  Every line it prints is compared with the CPU oracle."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_accumulator_strategy_over_two_vks(tmp_path):
    exe = ch.build("multi_key", tmp_path)
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 5, seed=51, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 5, seed=52, threads=4)
    items = []
    for j in range(5):
        items += [(s8, P8[j], I8[j]), (s4, P4[j], I4[j])]
    rnd = random.Random(53)
    rand = [rnd.randrange(1, R_MOD) for _ in items]

    def run(items):
        d = ch.write_dir(tmp_path, s8.params, vks=[s8.vk, s4.vk], rand=rand, items_txt=ch.keyed_items_text(items, (s8, s4)))
        return ch.run(exe, [d]).stdout.splitlines()

    for case in ("good", "bad"):
        if case == "bad":   # a wrong public input on the second key: the one pairing fails, every status stays 0
            items[3] = (s4, P4[1], [[circuits.le32(5)] + I4[1][0][1:]])
        out = run(items)
        ok, st, left, right = circuits.oracle_accumulate(items, rand)
        assert ok is (case == "good")
        m = [l for l in out if l.startswith("multi ")][0].split()
        assert (m[1] == "1") == ok and bytes.fromhex(m[2]) == left and bytes.fromhex(m[3]) == right and [int(x) for x in m[4:]] == st
        assert "identify_refused -19" in out and "seeded_refused -19" in out
    s8.free(); s4.free()
