"""The C++ mirror (include/h2v.hpp) of a staged batch's upload from device memory: tests/cpp/device_upload_harness.cpp runs one grouped
batch through h2v_batch_upload and through h2v::upload_device (the same bytes in device memory, rows 48 bytes apart) and prints both
results; they must be one line twice, and equal Batch.upload in Python."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_upload_device_equals_upload(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("device_upload_harness", tmp_path, hip=True)
    s = circuits.setup_vector_mul(8, 8)
    n, groups = 12, 3
    P, I = circuits.prove_vector_mul_batch(s, n, seed=77, threads=4)
    rnd = random.Random(78)
    rand = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(n))
    I2 = list(I)
    I2[5] = [[circuits.le32(5)] + I[5][0][1:]]          # a wrong public input: the pairing of group 1 fails
    flat, inst = b"".join(P), b"".join(b"".join(col) for i in I2 for col in i)
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand, proofs_bin=flat, instances_bin=inst)
    out = ch.run(exe, [d, n, groups, 1024, 8]).stdout.splitlines()
    assert out[1:3] == ["refused -16", "refused -16"], out[1:3]
    host, device = out[0].split(), out[3].split()
    assert host[0] == "host" and device[0] == "device" and host[1:] == device[1:]
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    b = h2v.Batch(ctx, n, 8, groups=groups)
    b.upload(flat, 1024, inst, [8], rand)
    b.launch()
    ok, st, left, right = b.finish_groups()
    assert ok == [True, False, True]
    assert device[1] == "".join(str(int(v)) for v in ok) and [int(x) for x in device[2:2 + n]] == st
    assert bytes.fromhex(device[2 + n]) == b"".join(left) and bytes.fromhex(device[3 + n]) == b"".join(right)
    b.close(); ctx.close(); s.free()
