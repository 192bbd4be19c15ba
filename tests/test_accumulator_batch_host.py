"""Feeding a staged batch to a resident accumulator, without a GPU.

  - the Python mirror (Accumulator.process_batch) checks its argument's type, the open handles and keep_inputs before it makes any C
    call, hands the library the two handles and two counters, and keeps its retained-inputs list as long as the journal;
  - the C++ mirror (Accumulator::process_batch), through tests/cpp/batch_legs_harness.cpp built with the address and
    undefined-behaviour sanitizers as a stand-alone program over the stand-in library (tests/cpp/h2v_stub.cpp + h2v_stub_batch_legs.cpp,
    which read every array with the lengths the calls pass), hands over buffers of the right lengths and refuses a null batch before
    any C call."""
import ctypes
import re

import pytest

import caller_harness as ch
from test_accumulator_host import _unbacked


class _Recorder:
    """stands where the loaded library would: records h2v_accumulator_process_batch and answers with canned counters"""

    def __init__(self, added, failed, rc=0):
        self.calls, self.added, self.failed, self.rc = [], added, failed, rc

    def h2v_accumulator_process_batch(self, acc, batch, n, f):
        self.calls.append((acc.value, batch.value))
        n._obj.value, f._obj.value = self.added, self.failed
        return self.rc


def _batch(handle=0x20, groups=3):
    from halo2_verifier_amd import verifier
    b = verifier.Batch.__new__(verifier.Batch)
    b._lib, b._h, b.groups, b.n = None, ctypes.c_void_p(handle), groups, 0
    return b


def test_process_batch_validates_before_any_c_call():
    acc, ctx = _unbacked()
    acc._h = ctypes.c_void_p(0x10)
    with pytest.raises(TypeError):
        acc.process_batch(ctx)                                     # not a Batch
    with pytest.raises(TypeError):
        acc.process_batch(None)
    closed = _batch(handle=None)
    with pytest.raises(ValueError):
        acc.process_batch(closed)                                  # a closed batch has no handle
    shut, _ = _unbacked()
    with pytest.raises(ValueError):
        shut.process_batch(_batch())                               # a closed accumulator
    acc._keep_inputs = True
    with pytest.raises(ValueError, match="Batch.identify"):
        acc.process_batch(_batch())                                # retained inputs are host bytes: a batch has none


def test_process_batch_call_and_bookkeeping(monkeypatch):
    acc, _ = _unbacked()
    acc._h = ctypes.c_void_p(0x10)
    # journal off: nothing is retained
    acc._lib = _Recorder(9, 0)
    acc._inputs = []
    assert acc.process_batch(_batch(groups=3)) == (9, 0) and acc.last_all_ok is True
    assert acc._lib.calls == [(0x10, 0x20)] and acc._inputs == []
    # journal on: one entry per group, none with inputs
    acc._inputs = [None, ("contexts", "keys", [], [])]
    acc._lib = _Recorder(12, 2)
    assert acc.process_batch(_batch(groups=4)) == (12, 2) and acc.last_all_ok is False
    assert acc._inputs == [None, ("contexts", "keys", [], [])] + [None] * 4
    # an upload of no proofs adds no entry
    acc._lib = _Recorder(0, 0)
    assert acc.process_batch(_batch(groups=4)) == (0, 0) and len(acc._inputs) == 6
    # a refused call raises and leaves the list as it was
    from halo2_verifier_amd import _lib, verifier
    monkeypatch.setattr(_lib, "last_error", lambda: "stand-in")
    acc._lib = _Recorder(0, 0, rc=-19)
    with pytest.raises(verifier.H2VError) as e:
        acc.process_batch(_batch())
    assert e.value.code == -19 and len(acc._inputs) == 6


def test_cpp_mirror_over_the_stand_in_library(tmp_path):
    exe = ch.build("batch_legs_harness", tmp_path, sanitize=True, stubs=("h2v_stub", "h2v_stub_batch_legs"))
    n, sizes = 6, [1, 3, 2]
    ch.write_dir(tmp_path, b"p" * 100, vks=[b"v" * 50], rand=bytes(range(32)) * n, items_txt=ch.stand_in_items_text(n))
    out = ch.run(exe, [tmp_path, ",".join(map(str, sizes))], timeout=120).stdout.splitlines()
    up = [l for l in out if l.startswith("h2v_batch_upload ")]
    assert len(up) == 1 and re.fullmatch(r"h2v_batch_upload batch=\S+ n=6 proof_len=40 ncols=2 n_tail=6 proofs=240:[0-9a-f]{16} inst=384:[0-9a-f]{16} tail=192:[0-9a-f]{16}", up[0])
    assert [l for l in out if l.startswith("h2v_batch_set_group_sizes ")] == ["h2v_batch_set_group_sizes batch=0xb000 sizes=[1,3,2]"]
    feeds = [l for l in out if l.startswith("h2v_accumulator_process_batch ")]
    assert len(feeds) == 2 and len(set(feeds)) == 1                 # the null batch never reaches the library
    assert re.fullmatch(r"h2v_accumulator_process_batch acc=\S+ batch=0xb000 added=asked,asked", feeds[0])
    assert "added 6 1 0" in out and "refused a null batch" in out
    assert len([l for l in out if l.startswith("h2v_accumulator_process ")]) == len(sizes)
    # the batch goes before the context that made it
    assert out.index("h2v_batch_destroy batch=0xb000") < min(i for i, l in enumerate(out) if l.startswith("h2v_ctx_destroy "))
