"""The host mirrors of the resident MSM object without a GPU, over the stand-in library tests/cpp/h2v_stub_msm.cpp (which records every
call, reads every array with the lengths the call passes, and can be told to fail):

  - the Python mirror (MSMKZG, DualMSM, eval_many, dual_check_many, Accumulator.add_msms) through ctypes against the stand-in built as a
    shared library: what it marshals, what it refuses before any C call (length mismatches, wrong byte lengths, use after close), and
    that a failing call raises H2VError and leaves the Python object usable;
  - the C++ mirror (Msm, DualMsm, Accumulator::add_msms) through tests/cpp/msm_object_harness.cpp, built with the address and
    undefined-behaviour sanitizers as a stand-alone program over the stand-in: buffers of the right lengths, move semantics, destruction
    order, the exception path, and check_many over an empty vector."""
import ctypes
import os
import re

import pytest

import caller_harness as ch

MSM_SYMBOLS = ["h2v_msm_create", "h2v_msm_destroy", "h2v_msm_append_terms", "h2v_msm_add_msm", "h2v_msm_scale", "h2v_msm_len", "h2v_msm_terms",
               "h2v_msm_eval_many", "h2v_dual_msm_check_many", "h2v_accumulator_add_msms"]


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """the stand-in as a shared library, with the signatures of halo2_verifier_amd/_lib.py"""
    from halo2_verifier_amd import _lib
    so = ch.build("h2v_stub_msm", tmp_path_factory.mktemp("stub"), shared=True, defines=("H2V_STUB_QUIET",))
    lib = ctypes.CDLL(str(so))
    for name in MSM_SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lib.h2v_stub_take_log.restype = ctypes.c_char_p
    lib.h2v_stub_set_fail.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.h2v_stub_set_fail(None, 0)
    lib.h2v_stub_take_log()
    return lib


def _log(lib):
    return lib.h2v_stub_take_log().decode().splitlines()


@pytest.fixture
def ctx(stub, monkeypatch):
    from halo2_verifier_amd import _lib, verifier
    monkeypatch.setattr(_lib, "last_error", lambda: "stand-in")
    c = verifier.Context.__new__(verifier.Context)
    c._lib, c._h = stub, ctypes.c_void_p(0x1000)
    stub.h2v_stub_set_fail(None, 0)
    stub.h2v_stub_take_log()
    yield c
    stub.h2v_stub_set_fail(None, 0)
    c._h = ctypes.c_void_p()   # (nothing to destroy: the context is not the stand-in's)


BASE = bytes(range(64))


def test_the_stand_in_covers_the_symbols():
    from halo2_verifier_amd import _lib
    assert sorted(MSM_SYMBOLS) == sorted(n for n in _lib.SIGNATURES if (n.startswith(("h2v_msm_", "h2v_dual_msm_")) and n != "h2v_msm_g1") or n == "h2v_accumulator_add_msms")


def test_python_marshalling(ctx, stub):
    from halo2_verifier_amd import verifier
    m = verifier.MSMKZG(ctx)
    m.append_term(7, BASE)
    m.append_terms([1, (2).to_bytes(32, "little")], [BASE, bytes(64)])
    m.append_terms([], [])
    assert len(m) == 3
    m.scale(5)
    log = _log(stub)
    assert log[0] == "h2v_msm_create"
    assert re.fullmatch(r"h2v_msm_append_terms m=m\d+:0 n=1 scalars=32:[0-9a-f]{16} bases=64:[0-9a-f]{16}", log[1])
    assert re.fullmatch(r"h2v_msm_append_terms m=m\d+:1 n=2 scalars=64:[0-9a-f]{16} bases=128:[0-9a-f]{16}", log[2])
    assert re.fullmatch(r"h2v_msm_append_terms m=m\d+:3 n=0 scalars=0:[0-9a-f]{16} bases=0:[0-9a-f]{16}", log[3])
    assert re.fullmatch(r"h2v_msm_scale m=m\d+:3 factor=32:[0-9a-f]{16}", log[-1])
    # read-back: ranges, and buffers of the lengths asked for
    assert m.scalars() == [0, 1, 2] and m.scalars(1, 2) == [1, 2] and m.scalars(3) == []
    assert m.bases(2, 1) == [bytes([0x42]) * 64] and len(m.bases()) == 3
    terms = [l for l in _log(stub) if l.startswith("h2v_msm_terms")]
    assert [l.split(" ", 2)[2] for l in terms] == ["first=0 count=3 scalars", "first=1 count=2 scalars", "first=3 count=0 scalars", "first=2 count=1 bases", "first=0 count=3 bases"]
    # eval / check / eval_many / clone
    e = verifier.MSMKZG(ctx)
    assert m.eval() == bytes([0x80]) * 64 and m.check() is False and e.check() is True and e.eval() == bytes(64)
    assert verifier.eval_many([m, e, m]) == ([bytes([0x80]) * 64, bytes(64), bytes([0x82]) * 64], [False, True, False])
    assert verifier.eval_many([]) == ([], [])
    c = m.clone()
    assert len(c) == 3 and c is not m and c._h.value != m._h.value
    log = _log(stub)
    assert any(re.fullmatch(r"h2v_msm_eval_many k=3 =m\d+:3 =m\d+:0 =m\d+:3", l) for l in log)
    assert any(re.fullmatch(r"h2v_msm_add_msm dst=m\d+:0 src=m\d+:3", l) for l in log)
    # close: destroyed once, through the context manager too
    with verifier.MSMKZG(ctx) as w:
        w.append_term(1, BASE)
    c.close(); c.close()
    assert len([l for l in _log(stub) if l.startswith("h2v_msm_destroy")]) == 2
    m.close(); e.close()


def test_python_refuses_before_any_c_call(ctx, stub):
    from halo2_verifier_amd import verifier
    m = verifier.MSMKZG(ctx)
    m.append_terms([1, 2], [BASE, BASE])
    _log(stub)
    for call in (lambda: m.append_terms([1, 2], [BASE]),                 # scalars and bases differ in length
                 lambda: m.append_terms([1], [BASE[:63]]),               # a base of 63 bytes
                 lambda: m.append_term(b"\x01" * 31, BASE),              # a scalar of 31 bytes
                 lambda: m.append_term(1 << 256, BASE),                  # a scalar that does not fit 32 bytes
                 lambda: m.scale(b"\x01" * 33),
                 lambda: m.scale(-1)):
        with pytest.raises(ValueError):
            call()
    assert _log(stub) == []
    with pytest.raises(ValueError):
        m.scalars(1, 2)                                                  # a range past the end: h2v_msm_len, then no h2v_msm_terms
    with pytest.raises(ValueError):
        m.bases(-1, 1)
    assert not [l for l in _log(stub) if not l.startswith("h2v_msm_len")]
    for call in (lambda: m.add_msm("not an object"), lambda: verifier.eval_many([m, None]), lambda: verifier.dual_check_many([m]), lambda: verifier.MSMKZG("not a context")):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        verifier.DualMSM(ctx, m, None)
    assert _log(stub) == []
    # use after close
    d = verifier.MSMKZG(ctx)
    d.close()
    _log(stub)
    for call in (lambda: len(d), lambda: d.append_term(1, BASE), lambda: d.scale(2), lambda: d.scalars(), lambda: d.bases(), lambda: d.eval(), lambda: d.check(),
                 lambda: d.clone(), lambda: d.add_msm(m), lambda: m.add_msm(d), lambda: verifier.eval_many([m, d])):
        with pytest.raises(ValueError, match="closed"):
            call()
    assert _log(stub) == []
    m.close()


def test_python_dual_and_accumulator(ctx, stub):
    from halo2_verifier_amd import verifier
    D = verifier.DualMSM(ctx)
    guard = dict(left_scalars=[1], left_bases=[BASE], right_scalars=[2, 3], right_bases=[BASE, BASE])
    D.scale(9)
    D.add_msm(guard)
    D.add_msm((([4], [BASE]), ([], [])))
    assert (len(D.left), len(D.right)) == (2, 2)
    E = verifier.DualMSM(ctx)
    E.add_msm(D)
    E.right.append_term(1, BASE)
    assert verifier.dual_check_many([D, E]) == ([True, False], [bytes([0x10]) * 64, bytes([0x11]) * 64], [bytes([0x20]) * 64, bytes([0x21]) * 64])
    assert D.check() is True and verifier.dual_check_many([]) == ([], [], [])
    # a malformed Guard is refused before either channel changes
    _log(stub)
    with pytest.raises(ValueError):
        D.add_msm((([1], [BASE]), ([1], [BASE[:10]])))
    with pytest.raises(ValueError):
        D.scale(1 << 256)
    assert _log(stub) == [] and (len(D.left), len(D.right)) == (2, 2)
    # Accumulator.add_msms: a DualMSM, or a pair with None for an empty channel
    acc = verifier.Accumulator.__new__(verifier.Accumulator)
    acc.ctx, acc._lib, acc._h, acc._inputs = ctx, stub, ctypes.c_void_p(0x2000), [None]
    _log(stub)
    acc.add_msms(D)
    acc.add_msms((None, D.right))
    log = _log(stub)
    assert re.fullmatch(r"h2v_accumulator_add_msms acc left=m\d+:2 right=m\d+:2", log[0]) and re.fullmatch(r"h2v_accumulator_add_msms acc left=null right=m\d+:2", log[1])
    assert acc._inputs == [None, None, None]   # journal on: an entry per call
    with pytest.raises(TypeError):
        acc.add_msms((D.left, "x"))
    D.right.close()
    with pytest.raises(ValueError, match="closed"):
        acc.add_msms(D)
    assert [l.split()[0] for l in _log(stub)] == ["h2v_msm_destroy"] and len(acc._inputs) == 3
    acc._h = ctypes.c_void_p()
    D.close(); E.close()


def test_python_failing_call_raises_and_leaves_the_object_usable(ctx, stub):
    from halo2_verifier_amd import verifier
    m = verifier.MSMKZG(ctx)
    m.append_term(1, BASE)
    for name, call in (("h2v_msm_append_terms", lambda: m.append_term(2, BASE)), ("h2v_msm_scale", lambda: m.scale(3)), ("h2v_msm_terms", lambda: m.scalars()),
                       ("h2v_msm_eval_many", lambda: m.eval()), ("h2v_msm_add_msm", lambda: m.clone()), ("h2v_msm_len", lambda: len(m)),
                       ("h2v_dual_msm_check_many", lambda: verifier.DualMSM(ctx, m, m).check())):
        stub.h2v_stub_set_fail(name.encode(), -16)
        with pytest.raises(verifier.H2VError) as e:
            call()
        assert e.value.code == -16, name
        stub.h2v_stub_set_fail(None, 0)
        assert len(m) == 1 and m._h
    # a clone whose add_msm failed was destroyed again
    log = _log(stub)
    i = log.index("h2v_msm_add_msm dst=%s src=%s -> -16" % tuple(re.search(r"dst=(m\d+:0) src=(m\d+:1)", "\n".join(log)).groups()))
    assert log[i + 1].startswith("h2v_msm_destroy m=")
    stub.h2v_stub_set_fail(b"h2v_msm_create", -18)
    with pytest.raises(verifier.H2VError) as e:
        verifier.MSMKZG(ctx)
    assert e.value.code == -18
    stub.h2v_stub_set_fail(None, 0)
    m.append_term(2, BASE)
    assert len(m) == 2
    m.close()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """the sanitizer build of the harness over the stand-in, and a directory with its inputs"""
    tmp_path = tmp_path_factory.mktemp("harness")
    exe = ch.build("msm_object_harness", tmp_path, sanitize=True, stubs=("h2v_stub", "h2v_stub_msm"))
    guards = "\n".join(["aa" * 32 + " " + "bb" * 64 + " " + "cc" * 64 + " " + "dd" * 128, "- - " + "ee" * 32 + " " + "ff" * 64, "11" * 64 + " " + "22" * 128 + " - -"]) + "\n"
    ch.write_dir(tmp_path, b"p" * 100, rand=bytes(range(32)) * 3, factor_bin=bytes([7]) * 32, guards_txt=guards)
    return exe, tmp_path


def test_cpp_mirror_over_the_stand_in_library(harness):
    exe, tmp_path = harness
    env = {k: v for k, v in os.environ.items() if k != "H2V_STUB_FAIL"}
    r = ch.run(exe, [tmp_path], timeout=120, env=env)
    out = r.stdout.splitlines()
    # D: left 1 + 0 + 2 terms, right 2 + 1 + 0; every scale before the Guard it precedes
    assert [l for l in out if l.startswith("hand ")] == ["hand 1 " + "10" * 64 + " " + "20" * 64 + " 3 3"]
    scales = [i for i, l in enumerate(out) if re.fullmatch(r"h2v_msm_scale m=m[12]:\d+ factor=32:[0-9a-f]{16}", l)]
    appends = [i for i, l in enumerate(out) if re.fullmatch(r"h2v_msm_append_terms m=m[12]:\d+ n=\d+ .*", l)]
    assert len(scales) == 6 and len(appends) == 6 and [a > s for s, a in zip(scales, appends)] == [True] * 6
    assert "h2v_msm_append_terms m=m2:0 n=2 scalars=64:%s bases=128:%s" % tuple(re.search(r"m=m2:0 n=2 scalars=64:(\S+) bases=128:(\S+)", r.stdout).groups()) in out
    assert "each 0 0 0" in out                      # the stand-in's rule: ok when both channels have as many terms
    assert "clone 4 3" in out and "empty 0 0" in out and "moved 1 1 2" in out and "refused 8" in out
    assert [l for l in out if l.startswith("h2v_accumulator_add_msms")] == ["h2v_accumulator_add_msms acc left=m1:3 right=m2:3", "h2v_accumulator_add_msms acc left=m1:3 right=null"]
    assert not [l for l in out if l.startswith("h2v_dual_msm_check_many k=0") or l.startswith("h2v_msm_eval_many k=0")]   # an empty vector makes no C call
    # every object created is destroyed exactly once, and all of them before the context
    made = len([l for l in out if l == "h2v_msm_create"])
    gone = [l for l in out if re.fullmatch(r"h2v_msm_destroy m=m\d+:\d+", l)]
    assert made == len(gone) == len(set(l.split(":")[0] for l in gone))
    last = max(i for i, l in enumerate(out) if l.startswith("h2v_msm_destroy"))
    assert last < min(i for i, l in enumerate(out) if l.startswith("h2v_ctx_destroy "))
    # a DualMsm's channels go in reverse order of their construction
    assert out.index("h2v_msm_destroy m=m2:3") < out.index("h2v_msm_destroy m=m1:3")


@pytest.mark.parametrize("fail", ["h2v_msm_scale", "h2v_msm_add_msm", "h2v_dual_msm_check_many", "h2v_accumulator_add_msms", "h2v_msm_create"])
def test_cpp_mirror_exception_paths(harness, fail):
    """A failing call throws Failure with the library's code; every object made so far is destroyed on the way out, before the context."""
    exe, tmp_path = harness
    r = ch.run(exe, [tmp_path], timeout=120, allow_fail=True, env=dict(os.environ, H2V_STUB_FAIL=fail))
    assert r.returncode == 1 and "failure -16" in r.stdout.splitlines(), (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    made = len([l for l in out if l == "h2v_msm_create"])
    gone = [l for l in out if re.fullmatch(r"h2v_msm_destroy m=m\d+:\d+", l)]
    assert made == len(gone) == len(set(l.split(":")[0] for l in gone))
    ctx_gone = [i for i, l in enumerate(out) if l.startswith("h2v_ctx_destroy ")]
    assert len(ctx_gone) == 1 and all(out.index(l) < ctx_gone[0] for l in gone)
    assert out.index("failure -16") > ctx_gone[0]   # the handler runs after the unwinding
