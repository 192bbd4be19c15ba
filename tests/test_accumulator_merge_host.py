"""The merge of resident accumulators without a GPU.

  - the Python mirror checks every length and type the C side would index before it makes any C call;
  - the state layout packs and unpacks as include/h2v.h documents it;
  - the C++ mirror's merge / export_state / merge_states, through tests/cpp/merge_harness.cpp built with the address and
    undefined-behaviour sanitizers over the stand-in library (tests/cpp/h2v_stub.cpp + h2v_stub_merge.cpp, which read every array with
    the lengths the calls pass), hand over buffers of the right lengths and refuse what they must before any C call;
  - distributed.ShardedAccumulator's orchestration over gloo with two CPU ranks and stand-in accumulators (tests/fake_accumulator.py):
    the states are merged in rank order, the draws are common to the ranks, a zero draw raises on every rank, and ranks that hold
    different params are refused at construction."""
import os
import re
import socket
import struct
import sys

import pytest

import caller_harness as ch
import merge_reference as mr
from test_accumulator_host import _unbacked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    acc, _ = _unbacked()
    acc._h = __import__("ctypes").c_void_p(0x10)
    return acc


def test_merge_validates_before_any_c_call():
    acc, _ = _unbacked()
    a, b = _source(), _source()
    with pytest.raises(TypeError):
        acc.merge([a, "not an accumulator"])
    with pytest.raises(ValueError):
        acc.merge([a, a])                                          # given twice
    with pytest.raises(ValueError):
        acc.merge([acc])                                           # the destination
    with pytest.raises(ValueError):
        acc.merge([a, b], [1])                                     # one draw for two sources
    with pytest.raises(ValueError):
        acc.merge([a], [b"\x01" * 31])                             # a draw of 31 bytes
    with pytest.raises(ValueError):
        acc.merge([a], [-1])
    with pytest.raises(ValueError):
        acc.merge([a], [1 << 256])
    with pytest.raises(ValueError):
        acc.merge([_source() for _ in range(513)])                 # more than MERGE_MAX
    closed, _ = _unbacked()
    with pytest.raises(ValueError):
        acc.merge([closed])                                        # a closed source has no handle


def test_merge_states_validates_before_any_c_call():
    acc, _ = _unbacked()
    good = mr.pack_state(bytes(64), bytes(64), 3, 1)
    with pytest.raises(ValueError):
        acc.merge_states([good[:-1]])                              # a state of 151 bytes
    with pytest.raises(ValueError):
        acc.merge_states([good + b"\x00"])
    with pytest.raises(ValueError):
        acc.merge_states(["x" * 152])                              # not bytes
    with pytest.raises(ValueError):
        acc.merge_states([good, good], [1])                        # one draw for two states
    with pytest.raises(ValueError):
        acc.merge_states([good], [b"\x01" * 33])
    with pytest.raises(ValueError):
        acc.merge_states([good] * 513)


def test_state_layout():
    from halo2_verifier_amd.verifier import Accumulator
    left, right = bytes(range(64)), bytes(range(100, 164))
    state = Accumulator.pack_state(left, right, 0x0102030405060708, 0x11)
    assert state == mr.pack_state(left, right, 0x0102030405060708, 0x11) and len(state) == Accumulator.STATE_BYTES == 152
    assert state[:4] == b"H2VS" and state[4:8] == b"\x01\x00\x00\x00"
    assert state[8:16] == bytes([8, 7, 6, 5, 4, 3, 2, 1]) and state[16:24] == b"\x11" + bytes(7)
    assert state[24:88] == left and state[88:] == right
    assert Accumulator.unpack_state(state) == (left, right, 0x0102030405060708, 0x11)
    for bad in (state[:-1], b"h" + state[1:], state[:4] + b"\x02" + state[5:]):
        with pytest.raises(ValueError):
            Accumulator.unpack_state(bad)
    with pytest.raises(ValueError):
        Accumulator.pack_state(left[:63], right, 0, 0)
    text = open(os.path.join(ROOT, "include", "h2v.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (H2V_ACC_(?:MERGE_MAX|STATE_BYTES|STATE_MAGIC|STATE_VERSION)) (\d+)", text)}
    assert consts == {"H2V_ACC_MERGE_MAX": Accumulator.MERGE_MAX, "H2V_ACC_STATE_BYTES": Accumulator.STATE_BYTES,
                      "H2V_ACC_STATE_MAGIC": Accumulator.STATE_MAGIC, "H2V_ACC_STATE_VERSION": Accumulator.STATE_VERSION}
    assert struct.unpack("<I", b"H2VS")[0] == Accumulator.STATE_MAGIC == mr.STATE_MAGIC


def test_cpp_mirror_over_the_stand_in_library(tmp_path):
    exe = ch.build("merge_harness", tmp_path, sanitize=True, stubs=("h2v_stub", "h2v_stub_merge"))
    n, K = 5, 3
    ch.write_dir(tmp_path, b"p" * 100, vks=[b"v" * 50], rand=bytes(range(32)) * n, draws_bin=bytes(range(1, 33)) * K, items_txt=ch.stand_in_items_text(n))
    out = ch.run(exe, [tmp_path, K], timeout=120).stdout.splitlines()
    merges = [l for l in out if l.startswith("h2v_accumulator_merge ")]
    assert len(merges) == 2                                         # the refused calls never reach the library
    assert re.fullmatch(r"h2v_accumulator_merge acc=\S+ srcs=\[\S+,\S+,\S+\] draws=96:[0-9a-f]{16} out=asked", merges[0])
    assert merges[1].endswith("draws=null out=asked")
    states = [l for l in out if l.startswith("h2v_accumulator_merge_states ")]
    assert len(states) == 1 and re.fullmatch(r"h2v_accumulator_merge_states acc=\S+ n=3 states=456:[0-9a-f]{16} draws=96:[0-9a-f]{16} out=asked", states[0])
    assert len([l for l in out if l.startswith("h2v_accumulator_export_state ")]) == K
    assert [l for l in out if l.startswith(("refused", "accepted"))] == [
        "refused too many sources", "refused draws of a wrong length", "refused states of a wrong length", "refused too many states",
        "refused the destination as a source", "refused a null source"]
    used = "".join("%02x" % (0xd0 + i % 16) for i in range(32 * K))
    assert [l.split()[-1] for l in out if l.startswith(("merge ", "states ", "drawn "))] == [used] * 3


# ---------------------------------------------------------------------------------------------------------------- orchestration over gloo
def _rank_main(rank, world, port, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from halo2_verifier_amd import distributed as h2d
    from fake_accumulator import FakeAccumulator, FakeContext
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {"rank": rank}
    sa = h2d.ShardedAccumulator(FakeContext(), accumulator_factory=FakeAccumulator, device="cpu")
    sa.acc.process(100 + rank)                                      # every rank feeds its own accumulator, no collective
    sa.acc.process(7)
    out["own_state"] = sa.acc.export_state()
    out["fixed"] = sa.finalize([5, 9])
    merged = sa.merged
    out["merged_journal"] = merged.journal
    out["merge_call"] = merged.calls
    out["bits"] = sa.check_ranks()
    out["drawn"] = sa.finalize()                                    # rank 0 draws, broadcasts
    out["first_merged_closed"] = merged.closed
    out["draws"] = sa.last_draws
    try:
        sa.finalize([4, 0])
        out["zero"] = "accepted"
    except ValueError:
        out["zero"] = "refused"
    out["after_zero"] = sa.finalize([5, 9])                         # no rank is left behind in a collective
    sa.close()
    out["all_closed"] = all(a.closed for a in FakeAccumulator.created)
    try:
        h2d.ShardedAccumulator(FakeContext(b"params of rank %d" % rank), accumulator_factory=FakeAccumulator, device="cpu")
        out["mismatch"] = "accepted"
    except ValueError:
        out["mismatch"] = "refused"
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_accumulator_orchestration_over_gloo():
    import torch.multiprocessing as mp
    world = 2
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    try:
        res = sorted((q.get(timeout=120) for _ in range(world)), key=lambda o: o["rank"])
        for p in procs: p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    states = [o["own_state"] for o in res]
    assert states[0] != states[1]
    fixed = [(5).to_bytes(32, "little"), (9).to_bytes(32, "little")]
    for o in res:
        assert o["merged_journal"] == world + 1
        assert o["merge_call"] == [("merge_states", states, fixed)]              # all states, in rank order, with the common draws
        assert o["fixed"] == res[0]["fixed"] == o["after_zero"]
        assert o["bits"] == res[0]["bits"] and len(o["bits"]) == world
        assert o["drawn"] == res[0]["drawn"] != o["fixed"]
        assert o["draws"] == res[0]["draws"] and len(o["draws"]) == 32 * world
        cs = [int.from_bytes(o["draws"][32 * k:32 * k + 32], "little") for k in range(world)]
        assert all(0 < c < mr.ref.R for c in cs) and cs[0] != cs[1]
        assert o["zero"] == "refused" and o["mismatch"] == "refused"
        assert o["first_merged_closed"] is True and o["all_closed"] is True


def test_merge_accumulators_local_with_stand_ins():
    from halo2_verifier_amd import distributed as h2d
    from fake_accumulator import FakeAccumulator, FakeContext
    ctx = FakeContext()
    accs = [FakeAccumulator(ctx) for _ in range(3)]
    for k, a in enumerate(accs):
        a.process(k + 1)
    ok, left, right, bits = h2d.merge_accumulators_local(ctx, accs, [3, 4, 5], accumulator_factory=FakeAccumulator)
    merged = FakeAccumulator.created[-1]
    assert merged.journal == 4 and merged.closed
    assert merged.calls == [("merge_states", [a.export_state() for a in accs], [(c).to_bytes(32, "little") for c in (3, 4, 5)])]
    assert ok is True and bits == [0, 1, 0]
    with pytest.raises(ValueError):
        h2d.merge_accumulators_local(ctx, accs, [3, 0, 5], accumulator_factory=FakeAccumulator)
    with pytest.raises(ValueError):
        h2d.merge_accumulators_local(ctx, accs, [3, 4], accumulator_factory=FakeAccumulator)
