"""The C++ mirror (include/h2v.hpp Accumulator) over proofs of two VerifyingKeys in two legs: tests/cpp/accumulator_harness.cpp feeds
them to one resident accumulator as they would arrive and prints the bytes; every line is compared with the Python class on the same
legs and with the CPU oracle's one accumulation over all of them."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_accumulator_two_legs_over_two_vks(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("accumulator_harness", tmp_path)
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 5, seed=51, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 5, seed=52, threads=4)
    items = []
    for j in range(5):
        items += [(s8, P8[j], I8[j]), (s4, P4[j], I4[j])]
    rnd = random.Random(54)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    cut = 3
    ctxs = [h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes)) for s in (s8, s4)]

    def run(items):
        d = ch.write_dir(tmp_path, s8.params, vks=[s8.vk, s4.vk], rand=rand, items_txt=ch.keyed_items_text(items, (s8, s4)))
        return ch.run(exe, [d, cut]).stdout.splitlines()

    def python_legs(items):
        acc = h2v.Accumulator(ctxs[0])
        keys = [0 if s is s8 else 1 for s, _, _ in items]
        st = acc.process(ctxs, keys[:cut], [p for _, p, _ in items[:cut]], [i for _, _, i in items[:cut]], rand[:cut])
        first = acc.read()
        st += acc.process(ctxs, keys[cut:], [p for _, p, _ in items[cut:]], [i for _, _, i in items[cut:]], rand[cut:])
        ok, left, right = acc.finalize()
        acc.close()
        return first, (ok, st, left, right)

    for case in ("good", "bad"):
        if case == "bad":   # a wrong public input on the second key, in the second leg: the one pairing fails, every status stays 0
            items[3] = (s4, P4[1], [[circuits.le32(5)] + I4[1][0][1:]])
        out = run(items)
        first, got = python_legs(items)
        exp = circuits.oracle_accumulate(items, rand)
        assert got == exp and exp[0] is (case == "good")
        f = [l for l in out if l.startswith("first ")][0].split()
        assert (bytes.fromhex(f[1]), bytes.fromhex(f[2]), int(f[3]), int(f[4])) == first == (*circuits.oracle_accumulate(items[:cut], rand[:cut])[2:], cut, 0)
        m = [l for l in out if l.startswith("acc ")][0].split()
        assert (m[1] == "1", [int(x) for x in m[4:]], bytes.fromhex(m[2]), bytes.fromhex(m[3])) == exp
        assert f"again {1 if exp[0] else 0}" in out
    for c in ctxs:
        c.close()
    s8.free(); s4.free()
