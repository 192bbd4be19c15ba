"""The C++ mirror of the feed of a staged batch to a resident accumulator (include/h2v.hpp Accumulator::process_batch) through the C
ABI: tests/cpp/batch_legs_harness.cpp stages ten proofs in groups of 3 / 1 / 4 / 2 without a pairing, one of them failing by status,
feeds the finished batch to a journaled accumulator and the same proofs to a second one by process, group by group; every line is
compared with the Python class on the same proofs and with the CPU oracle's one accumulation."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_feed_of_a_batch_in_four_groups(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("batch_legs_harness", tmp_path)
    n, sizes = 10, [3, 1, 4, 2]
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, n, seed=71, threads=4)
    P[5] = P[5][:-96] + b"\xff" * 32 + P[5][-64:]                    # a non-canonical scalar: status -5, in group 2
    rnd = random.Random(72)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    d = ch.write_dir(tmp_path, s.params, vks=[s.vk], rand=rand, items_txt=ch.items_text(P, I, keys=[0] * n))
    out = ch.run(exe, [d, ",".join(map(str, sizes))]).stdout.splitlines()

    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is False and [i for i, v in enumerate(exp[1]) if v] == [5]
    want = ["0", exp[2].hex(), exp[3].hex(), str(n), "1"]
    want_legs = [f"leg 0 0 0 1"] + [f"leg {g + 1} {sz} {1 if g == 2 else 0} 1" for g, sz in enumerate(sizes)]

    # the Python class on the same proofs
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    b = h2v.Batch(ctx, n, 8)
    b.set_group_sizes(sizes)
    b.upload(b"".join(P), len(P[0]), b"".join(v for inst in I for col in inst for v in col), [8], b"".join(r.to_bytes(32, "little") for r in rand))
    b.launch(with_pairing=False)
    b.finish_groups()
    acc = h2v.Accumulator(ctx, journal=2 * len(sizes) + 1)
    added = acc.process_batch(b)
    ok, left, right = acc.finalize()
    py = [str(int(ok)), left.hex(), right.hex(), str(acc.read()[2]), str(acc.read()[3])]
    py_legs = [f"leg {e} {p} {f} {int(bit)}" for e, (p, f, bit) in enumerate(acc.check_legs())]
    acc.process_batch(b)
    again = acc.read()[2:]
    acc.close(); b.close(); ctx.close()

    assert added == (n, 1) and out[0] == f"added {n} 1 0"
    assert [l for l in out if l.startswith("batch ")][0].split()[1:] == py == want
    assert [l for l in out if l.startswith("process ")][0].split()[1:] == want
    assert [l for l in out if l.startswith("leg ")] == py_legs == want_legs
    assert [l for l in out if l.startswith("again ")] == [f"again {again[0]} {again[1]}"] == [f"again {2 * n} 2"]
    assert out[-1] == "refused a null batch"
    s.free()
