"""The C++ mirror (include/h2v.hpp) of a staged batch's finish into device memory: tests/cpp/device_finish_harness.cpp launches one
grouped batch, reads h2v::finish_device's arrays before and after h2v_batch_finish_groups and prints all three; the device lines must
be one line twice, agree with the host line and with Batch.finish_groups in Python, and carry the counts, indices and summary that
follow from the statuses.  It also holds the refusal of a status array in an allocation one byte short (hipMalloc's own size)."""
import random

import pytest

import caller_harness as ch
import circuits
import results_reference as rr
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_finish_device_equals_finish_groups(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("device_finish_harness", tmp_path, hip=True)
    s = circuits.setup_vector_mul(8, 8)
    n, groups = 12, 3
    P, I = circuits.prove_vector_mul_batch(s, n, seed=77, threads=4)
    rnd = random.Random(78)
    rand = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(n))
    I2, P2 = list(I), list(P)
    I2[5] = [[circuits.le32(5)] + I[5][0][1:]]          # a wrong public input: the pairing of group 1 fails
    P2[9] = P2[9][:-96] + b"\xff" * 32 + P2[9][-64:]    # a non-canonical scalar: status -5, in group 2
    flat, inst = b"".join(P2), b"".join(b"".join(col) for i in I2 for col in i)
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand, proofs_bin=flat, instances_bin=inst)
    out = ch.run(exe, [d, n, groups, 1024, 8]).stdout.splitlines()
    assert out[:3] == ["refused -16"] * 3, out[:3]
    before, host, after = out[3], out[4].split(), out[5]
    assert before == after and before.startswith("device ") and host[0] == "host"
    results, failed, index, summary = [part.split() for part in before.split("|")]
    assert results[1:] == host[1:]
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    b = h2v.Batch(ctx, n, 8, groups=groups)
    b.upload(flat, 1024, inst, [8], rand)
    b.launch()
    ok, st, left, right = b.finish_groups()
    assert ok == [True, False, False] and [i for i, v in enumerate(st) if v] == [9]
    assert host[1] == "".join(str(int(v)) for v in ok) and [int(x) for x in host[2:2 + n]] == st
    assert bytes.fromhex(host[2 + n]) == b"".join(left) and bytes.fromhex(host[3 + n]) == b"".join(right)
    assert [int(x) for x in failed] == rr.group_failed(st, groups) == [0, 0, 1]
    assert [int(x) for x in index] == [9] + [0xEEEEEEEE] * (n - 1)
    assert [int(x) for x in summary] == [rr.NO_FAULT, 1, 1, n, groups, rr.FLAG_PAIRING, 0, 0]
    b.close(); ctx.close(); s.free()
