"""The C++ mirror (include/h2v.hpp) of identification over proofs of two VerifyingKeys: tests/cpp/identify_keys.cpp queues them on
one AccumulatorStrategy in call order and finalize_identify_keys() runs h2v_verify_batch_keys_identify.  The printed verdict,
channels and statuses are compared with the CPU oracle."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_finalize_identify_keys_over_two_vks(tmp_path):
    exe = ch.build("identify_keys", tmp_path)
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 6, seed=81, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 6, seed=82, threads=4)
    items = []
    for j in range(6):
        items += [(s8, P8[j], I8[j]), (s4, P4[j], I4[j])]
    rnd = random.Random(83)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    d = ch.write_dir(tmp_path, s8.params, vks=[s8.vk, s4.vk], rand=rand)

    def run(items):
        ch.write_dir(d, items_txt=ch.keyed_items_text(items, (s8, s4)))
        return ch.run(exe, [d]).stdout.splitlines()

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
