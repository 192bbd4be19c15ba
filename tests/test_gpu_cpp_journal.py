"""The C++ mirror of the leg journal (include/h2v.hpp Accumulator::journal_begin / check_legs / drop_legs) over proofs of two
VerifyingKeys in three legs, one of them holding a proof that only the pairing rejects: tests/cpp/journal_harness.cpp feeds them to
one journaled accumulator, drops the legs whose own pairing fails and prints the bytes; every line is compared with the Python class on
the same legs and with the CPU oracle's accumulation over the kept legs."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_journal_three_legs_over_two_vks(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("journal_harness", tmp_path)
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 5, seed=51, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 5, seed=52, threads=4)
    items = []
    for j in range(5):
        items += [(s8, P8[j], I8[j]), (s4, P4[j], I4[j])]
    items[5] = (s4, P4[2], [[circuits.le32(5)] + I4[2][0][1:]])   # a wrong public input on the second key, in the second leg
    assert circuits.oracle_verify_single(s4, items[5][1], items[5][2]) == -2
    rnd = random.Random(55)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    bounds = [0, 3, 7, 10]
    d = ch.write_dir(tmp_path, s8.params, vks=[s8.vk, s4.vk], rand=rand, items_txt=ch.keyed_items_text(items, (s8, s4)))
    out = ch.run(exe, [d, 3, 7]).stdout.splitlines()

    # the Python class on the same legs
    ctxs = [h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes)) for s in (s8, s4)]
    acc = h2v.Accumulator(ctxs[0], journal=4)
    keys = [0 if s is s8 else 1 for s, _, _ in items]
    for a, b in zip(bounds, bounds[1:]):
        acc.process(ctxs, keys[a:b], [p for _, p, _ in items[a:b]], [i for _, _, i in items[a:b]], rand[a:b])
    py_legs, py_before = acc.check_legs(), acc.finalize()
    acc.drop_legs([2])
    py_after = (*acc.finalize(), *acc.read()[2:], len(acc.check_legs()))
    acc.close()
    for c in ctxs:
        c.close()

    # the oracle: every leg alone, all of them, the kept ones
    legs = [(items[a:b], rand[a:b]) for a, b in zip(bounds, bounds[1:])]
    bits = [circuits.oracle_pairing_check(s8, *circuits.oracle_accumulate(*leg)[2:]) for leg in legs]
    assert bits == [True, False, True]
    exp_legs = [(0, 0, True)] + [(len(leg[0]), 0, bit) for leg, bit in zip(legs, bits)]
    whole = circuits.oracle_accumulate(items, rand)
    kept = circuits.oracle_accumulate(legs[0][0] + legs[2][0], legs[0][1] + legs[2][1])
    assert whole[0] is False and kept[0] is True

    got_legs = [tuple(int(x) for x in l.split()[2:]) for l in out if l.startswith("leg ")]
    assert [(a, b, bool(c)) for a, b, c in got_legs] == py_legs == exp_legs
    b = [l for l in out if l.startswith("before ")][0].split()
    assert (b[1] == "1", bytes.fromhex(b[2]), bytes.fromhex(b[3])) == py_before == (whole[0], whole[2], whole[3])
    assert "dropped 2" in out
    a = [l for l in out if l.startswith("after ")][0].split()
    assert (a[1] == "1", bytes.fromhex(a[2]), bytes.fromhex(a[3]), int(a[4]), int(a[5]), int(a[6])) == py_after == (kept[0], kept[2], kept[3], 6, 0, 3)
    s8.free(); s4.free()
