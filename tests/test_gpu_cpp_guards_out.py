"""The C++ mirror (include/h2v_guards.hpp) of every proof's Guard out of a launch: tests/cpp/guards_out_harness.cpp launches one small
grouped batch and prints a range's Guards through h2v::guards::to_host, to_device and append; the three must agree with each other
and with Batch.guards in Python, and the finish afterwards with Batch.finish_groups."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_guards_round_trip(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("guards_out_harness", tmp_path, hip=True)
    s = circuits.setup_vector_mul(8, 8)
    n, groups, first, count = 12, 3, 2, 8                       # the range crosses both group boundaries
    P, I = circuits.prove_vector_mul_batch(s, n, seed=177, threads=4)
    rnd = random.Random(178)
    rand = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(n))
    P2 = list(P)
    P2[6] = P2[6][:-96] + b"\xff" * 32 + P2[6][-64:]            # a non-canonical scalar: status -5, a zero row inside the range
    flat, inst = b"".join(P2), b"".join(b"".join(col) for i in I for col in i)
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand, proofs_bin=flat, instances_bin=inst)
    out = ch.run(exe, [d, n, groups, 1024, 8, first, count]).stdout.splitlines()
    assert out[0] == "shape 1 18" and out[1:3] == ["refused -16"] * 2, out[:3]
    host, device, append, guard, finish = out[3:8]
    assert host.startswith("host ") and device == "device" + host[4:]
    status, terms = host[5:].split(" | ")
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    b = h2v.Batch(ctx, n, 8, groups=groups)
    b.upload(flat, 1024, inst, [8], rand)
    b.launch()
    rows = b.guards(first, count)
    cat = lambda k: b"".join(x for r in rows for x in r[k]).hex()
    want = [cat("left_scalars"), cat("left_bases"), cat("right_scalars"), cat("right_bases"), b"".join(r["mult"] for r in rows).hex()]
    assert [int(v) for v in status.split()] == [r["status"] for r in rows] == [0, 0, 0, 0, -5, 0, 0, 0]
    assert terms.split() == want
    assert append == "append 1 | " + " ".join(want[:4])
    assert guard == "guard %d %s" % (count - 1, b"".join(rows[-1]["right_scalars"]).hex())
    ok, st, _, _ = b.finish_groups()
    assert finish.split() == ["finish", "".join(str(int(v)) for v in ok)] + [str(v) for v in st] and ok == [True, False, True]
    b.close(); ctx.close(); s.free()
