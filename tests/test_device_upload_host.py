"""Batch.upload_device / Batch.upload_tensors / ShardedBatch.upload_tensors: every length, type and alignment the Python mirror can see
is checked before the C library is reached (no GPU: the library is a stub that fails when touched)."""
import types

import pytest

import halo2_verifier_amd as h2v


class _Lib:
    def __getattr__(self, name):
        raise AssertionError(f"the C library must not be reached ({name})")


def _batch(max_proofs=16, groups=1, sizes=None, device=0):
    b = object.__new__(h2v.Batch)            # no device: only the marshalling code is under test
    b._lib, b._h, b._keep = _Lib(), None, None
    b.ctx = types.SimpleNamespace(device=device)
    b.max_proofs, b.n, b.groups, b.group_sizes = max_proofs, 0, len(sizes) if sizes else groups, sizes
    return b


class _Device:
    def __init__(self, type="cuda", index=0): self.type, self.index = type, index
    def __repr__(self): return f"{self.type}:{self.index}"


class _Tensor:
    """what upload_tensors reads of a tensor"""
    def __init__(self, shape, stride=None, dtype="torch.uint8", device=None, ptr=0x7f0000000000):
        self.shape, self._stride, self.dtype, self.device, self._ptr = shape, stride or (shape[-1], 1), dtype, device or _Device(), ptr
    def stride(self): return self._stride
    def data_ptr(self): return self._ptr


A = 0x7f0000000000


def test_upload_device_checks_its_numbers():
    b = _batch()
    with pytest.raises(ValueError, match="16-byte aligned"):
        b.upload_device(A + 8, 4, 1024, A, [8], A, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        b.upload_device(A, 4, 1024, A + 4, [8], A, 4)
    with pytest.raises(ValueError, match="16-byte aligned"):
        b.upload_device(A, 4, 1024, A, [8], A + 1, 4)
    with pytest.raises(ValueError, match="multiple of 16"):
        b.upload_device(A, 4, 1032, A, [8], A, 4)
    with pytest.raises(ValueError, match="multiple of 16"):
        b.upload_device(A, 4, 0, A, [8], A, 4)
    with pytest.raises(ValueError, match="proofs_addr is missing"):
        b.upload_device(0, 4, 1024, A, [8], A, 4)
    with pytest.raises(ValueError, match="instances_addr is missing"):
        b.upload_device(A, 4, 1024, None, [8], A, 4)
    with pytest.raises(ValueError, match="capacity"):
        b.upload_device(A, 17, 1024, A, [8], A, 17)
    with pytest.raises(ValueError, match="below n"):
        b.upload_device(A, 4, 1024, A, [8], A, 3)
    with pytest.raises(ValueError, match="n_tail without rand_addr"):
        b.upload_device(A, 4, 1024, A, [8], None, 4)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            b.upload_device(A, bad, 1024, A, [8], A, 4)
        with pytest.raises(ValueError, match=r"\[0, 2\^64\)"):
            b.upload_device(bad, 4, 1024, A, [8], A, 4)
    for bad in (4.0, "4", True, None):
        with pytest.raises(TypeError, match="must be an integer"):
            b.upload_device(A, bad, 1024, A, [8], A, 4)
    with pytest.raises(TypeError, match="column length"):
        b.upload_device(A, 4, 1024, A, [8.0], A, 4)


def test_upload_device_checks_the_groups():
    with pytest.raises(ValueError, match="multiples of the group count"):
        _batch(groups=4).upload_device(A, 6, 1024, A, [8], A, 8)
    with pytest.raises(ValueError, match="multiples of the group count"):
        _batch(groups=4).upload_device(A, 8, 1024, A, [8], A, 10)
    with pytest.raises(ValueError, match="group sizes sum to 11"):
        _batch(sizes=[1, 7, 3]).upload_device(A, 12, 1024, A, [8], A, 12)
    with pytest.raises(ValueError, match="one draw per proof"):
        _batch(sizes=[1, 7, 3]).upload_device(A, 11, 1024, A, [8], A, 22)


def test_upload_tensors_checks_the_tensors():
    b = _batch()
    good = dict(proofs=_Tensor((4, 1024), (1088, 1)), instances=_Tensor((4, 256)), col_lens=[8], rand_tail=_Tensor((4, 32)))

    def refused(exc, match, **change):
        with pytest.raises(exc, match=match):
            b.upload_tensors(**{**good, **change})

    refused(TypeError, "must be a tensor", proofs=b"\0" * 4096)
    refused(TypeError, "uint8", proofs=_Tensor((4, 1024), dtype="torch.int8"))
    refused(TypeError, "uint8", rand_tail=_Tensor((4, 32), dtype="torch.float32"))
    refused(ValueError, "context's device", proofs=_Tensor((4, 1024), device=_Device("cpu", None)))
    refused(ValueError, "context's device", instances=_Tensor((4, 256), device=_Device("cuda", 1)))
    refused(ValueError, "2-D with unit inner stride", proofs=_Tensor((4096,), (1,)))
    refused(ValueError, "2-D with unit inner stride", proofs=_Tensor((4, 1024), (2048, 2)))
    refused(ValueError, "rows overlap", proofs=_Tensor((4, 1024), (512, 1)))
    refused(ValueError, "must hold 4 rows", instances=_Tensor((3, 256)))
    refused(ValueError, "contiguous rows of 256 bytes", instances=_Tensor((4, 128)))
    refused(ValueError, "contiguous rows of 256 bytes", instances=_Tensor((4, 256), (512, 1)))
    refused(ValueError, "contiguous rows of 32 bytes", rand_tail=_Tensor((4, 64)))
    refused(ValueError, "instances missing", instances=None)
    refused(TypeError, "no cuda streams")   # tensors whose module has no streams to order the upload behind (these stand-ins)


def test_upload_tensors_orders_the_streams_then_calls_upload_device(monkeypatch):
    """with a stand-in for the tensors' module: the batch's stream waits for the current one by an event, and the numbers that go on
    are the tensors' (the row stride as proof_stride); the tensors are kept"""
    import sys
    log = []

    class Event:
        def record(self, stream): log.append(("record", stream.cuda_stream))

    class Stream:
        def __init__(self, handle, device=None): self.cuda_stream = handle
        def wait_event(self, ev): log.append(("wait", self.cuda_stream))

    fake = types.ModuleType("faketorch")
    fake.cuda = types.SimpleNamespace(current_stream=lambda device: Stream(111), Event=Event, ExternalStream=Stream)
    monkeypatch.setitem(sys.modules, "faketorch", fake)
    T = type("T", (_Tensor,), {"__module__": "faketorch.tensor"})
    b = _batch()
    monkeypatch.setattr(h2v.Batch, "stream", property(lambda self: 222))
    monkeypatch.setattr(h2v.Batch, "upload_device", lambda self, *a: log.append(("upload_device",) + a))
    p, i, r = T((4, 1024), (1088, 1), ptr=A), T((4, 256), ptr=A + 0x10000), T((8, 32), ptr=A + 0x20000)
    b.upload_tensors(p, i, [8], r)
    assert log == [("record", 111), ("wait", 222), ("upload_device", A, 4, 1088, A + 0x10000, [8], A + 0x20000, 8)]
    assert b._keep == (p, i, r)
    del log[:]
    monkeypatch.setattr(h2v.Batch, "stream", property(lambda self: 111))       # the batch runs on the current stream: nothing to wait for
    b.upload_tensors(p, None, [0], None)
    assert log == [("upload_device", A, 4, 1088, None, [0], None, None)]


def test_sharded_batch_forwards_upload_tensors():
    from halo2_verifier_amd.distributed import ShardedBatch
    calls = []
    sb = object.__new__(ShardedBatch)
    sb.batch = types.SimpleNamespace(upload_tensors=lambda *a: calls.append(a))
    sb.upload_tensors("p", "i", [8], "r")
    assert calls == [("p", "i", [8], "r")]


def test_common_draws_tensor_without_a_group():
    """a world of one: the given draws, or OS draws, as an [n, 32] uint8 tensor (on the CPU here)"""
    import torch
    from halo2_verifier_amd.distributed import common_draws, common_draws_tensor
    t = common_draws_tensor(3, [5, 6, 7], device="cpu")
    assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 32) and bytes(t.numpy().tobytes()) == common_draws(3, [5, 6, 7])
    assert tuple(common_draws_tensor(0, [], device="cpu").shape) == (0, 32)
    t = common_draws_tensor(4, None, device="cpu")
    assert tuple(t.shape) == (4, 32) and all(int.from_bytes(bytes(row.numpy().tobytes()), "little") < h2v.distributed._FR_MODULUS for row in t)
