"""k_expand_draws (h2v_draws_expand_device; draws.expand_tensor / expand_into) against the definition in hashlib: the sizes around a
wave's 16 draws, the carry of the index into its high word, a non-default stream with an output that is 16- but not 32-byte
aligned inside a larger tensor, the bytes around the range, and the refusals before any device work."""
import ctypes
import hashlib

import pytest

pytestmark = pytest.mark.gpu

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
SEED = bytes((13 * i + 1) % 256 for i in range(32))
FIRSTS = (0, 2**32 - 3)
SIZES = (1, 15, 16, 17, 64, 1000)


def ref_expand(seed, first, n):
    return b"".join((int.from_bytes(hashlib.blake2b(seed + (first + j).to_bytes(8, "little"), digest_size=64, person=b"h2v-draws-v1").digest(), "little") % R_MOD)
                    .to_bytes(32, "little") for j in range(n))


@pytest.fixture(scope="module")
def want():
    """the reference, computed once: 1000 draws from each first index (every smaller size is a prefix)"""
    return {first: ref_expand(SEED, first, max(SIZES)) for first in FIRSTS}


def _bytes(t):
    return bytes(t.cpu().numpy().tobytes())


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_hashlib(want, n, first):
    import halo2_verifier_amd as h2v
    t = h2v.expand_tensor(SEED, first, n, 0)
    assert tuple(t.shape) == (n, 32) and str(t.dtype) == "torch.uint8" and t.device.index == 0
    assert _bytes(t) == want[first][:32 * n]
    assert _bytes(t) == h2v.expand(SEED, first, n)        # the host twin, byte for byte


def test_anchors_and_the_last_index():
    import halo2_verifier_amd as h2v
    assert int.from_bytes(_bytes(h2v.expand_tensor(bytes(range(32)), 0, 1, 0)), "little") == 0x0607e6c5ce8f7375ea1844befb5daf4254965d7eb09a39d6c4517fcdd083a836
    assert int.from_bytes(_bytes(h2v.expand_tensor(bytes(range(32)), 2**32, 1, 0)), "little") == 0x0868191628889fa2ded1674ca5f3c1224c59425f1d4237d514fcb7f05d9bd118
    assert int.from_bytes(_bytes(h2v.expand_tensor(bytes(32), 2**64 - 1, 1, 0)), "little") == 0x18dac5e3375e9e19c02fd8bc5fec5b0dd086a06209773b32d1f170ea7301574e
    assert _bytes(h2v.expand_tensor(SEED, 2**64 - 20, 20, 0)) == ref_expand(SEED, 2**64 - 20, 20)
    assert tuple(h2v.expand_tensor(SEED, 5, 0, 0).shape) == (0, 32)


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", SIZES)
def test_other_stream_offset_output_and_untouched_surroundings(want, n, first):
    import torch
    from halo2_verifier_amd import draws
    big = torch.full((16 + 32 * n + 48,), 0x5C, dtype=torch.uint8, device="cuda:0")
    out = big[16:16 + 32 * n].view(n, 32)
    assert out.data_ptr() % 32 == 16
    stream = torch.cuda.Stream(device="cuda:0")
    draws.expand_into(SEED, first, out, stream)
    stream.synchronize()
    got = _bytes(big)
    assert got[:16] == b"\x5c" * 16 and got[16 + 32 * n:] == b"\x5c" * 48
    assert got[16:16 + 32 * n] == want[first][:32 * n]


def test_refusals_come_before_any_device_work():
    import numpy as np
    import torch
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import draws
    lib = draws._library()
    t = torch.full((64, 32), 0x77, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    pa = t.data_ptr()

    def call(device, seed, first, n, addr):
        return lib.h2v_draws_expand_device(device, None, seed, first, n, ctypes.c_void_p(addr))

    def refused(match, *args):
        assert call(*args) == -16
        assert match in h2v._lib.last_error(), h2v._lib.last_error()

    host = np.zeros(32 * 8 + 64, dtype=np.uint8)
    refused("not device memory", 0, SEED, 0, 8, (host.ctypes.data + 15) // 16 * 16)        # a host pointer
    refused("16-byte aligned", 0, SEED, 0, 8, pa + 1)                                     # an odd address
    refused("16-byte aligned", 0, SEED, 0, 8, pa + 8)
    seg = next(x for x in torch.cuda.memory_snapshot() if x["address"] <= pa < x["address"] + x["total_size"])
    end = seg["address"] + seg["total_size"]
    refused("past the pointer's allocation", 0, SEED, 0, 3, end - 64)                      # a range ending past the allocation
    refused("past the pointer's allocation", 0, SEED, 0, seg["total_size"] // 32 + 1, seg["address"])
    refused("wraps", 0, SEED, 2**64 - 4, 5, pa)                                            # wrap-around
    refused("null", 0, None, 0, 8, pa)
    refused("null", 0, SEED, 0, 8, 0)
    refused("no such device", torch.cuda.device_count(), SEED, 0, 8, pa)
    refused("no such device", -1, SEED, 0, 8, pa)
    refused("H2V_DRAWS_DEVICE_MAX", 0, SEED, 0, draws.DEVICE_MAX + 1, pa)                 # more than one launch holds
    torch.cuda.synchronize()
    assert _bytes(t) == b"\x77" * (64 * 32)          # nothing was written
    # the Python mirror refuses what it can see
    with pytest.raises(ValueError, match="2\\^64"):
        draws.expand_tensor(SEED, 2**64 - 4, 5, 0)
    with pytest.raises(ValueError, match="contiguous uint8"):
        draws.expand_into(SEED, 0, t[:, :16])
    with pytest.raises(ValueError, match="device memory"):
        draws.expand_tensor(SEED, 0, 4, "cpu")
    # the same arguments, valid: the call is taken
    assert call(0, SEED, 7, 8, pa) == 0
    torch.cuda.synchronize()
    assert _bytes(t[:8]) == ref_expand(SEED, 7, 8) and _bytes(t[8:]) == b"\x77" * (56 * 32)


def test_a_pointer_of_another_device_is_refused():
    import torch
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import draws
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    t = torch.zeros((8, 32), dtype=torch.uint8, device="cuda:1")
    torch.cuda.synchronize(1)
    assert draws._library().h2v_draws_expand_device(0, None, SEED, 0, 8, ctypes.c_void_p(t.data_ptr())) == -16
    assert "not device memory of" in h2v._lib.last_error()
