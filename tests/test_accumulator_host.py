"""The resident accumulator's host side without a GPU: the Python class checks every length the C side would index before it makes
any C call, and nothing stands in for a missing device."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoCalls:
    """stands where the loaded library would: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"C call {name} before the arguments were validated")


def _unbacked():
    """an Accumulator and a Context with no library behind them"""
    from halo2_verifier_amd import verifier
    ctx = verifier.Context.__new__(verifier.Context)
    ctx._lib, ctx._h = _NoCalls(), None
    acc = verifier.Accumulator.__new__(verifier.Accumulator)
    acc.ctx, acc._lib, acc._h = ctx, _NoCalls(), None
    return acc, ctx


def test_process_validates_lengths_before_any_c_call():
    acc, ctx = _unbacked()
    p, inst = b"\x00" * 64, [[b"\x01" * 32]]
    with pytest.raises(ValueError):
        acc.process([ctx], [0], [p, p], [inst, inst])              # one key index for two proofs
    with pytest.raises(ValueError):
        acc.process([ctx], [0, 0], [p, p], [inst])                 # one instance list for two proofs
    with pytest.raises(ValueError):
        acc.process([ctx], [0, 0], [p, p], [inst, inst], [1])      # one draw for two proofs
    with pytest.raises(ValueError):
        acc.process([ctx], [0, 1], [p, p], [inst, inst])           # a key index out of range
    with pytest.raises(ValueError):
        acc.process([], [], [], [])                                # no context
    with pytest.raises(ValueError):
        acc.process(ctx, [0], [p], [inst])                         # the one-key form takes no key indices
    with pytest.raises(ValueError):
        acc.process([ctx], None, [p], [inst])                      # several keys need them
    with pytest.raises(ValueError):
        acc.process(ctx, None, [p], [[[b"\x01" * 31]]])            # a scalar of 31 bytes
    with pytest.raises(ValueError):
        acc.process(ctx, None, [p], [inst], [b"\x01" * 33])        # a draw of 33 bytes
    with pytest.raises(TypeError):
        acc.process(ctx, None, ["not bytes"], [inst])


def test_add_msm_validates_lengths_before_any_c_call():
    acc, _ = _unbacked()
    base = b"\x00" * 64
    with pytest.raises(ValueError):
        acc.add_msm(([1, 2], [base]), ([], []))                    # scalars and bases differ in length
    with pytest.raises(ValueError):
        acc.add_msm(([1], [base[:63]]), ([], []))                  # a base of 63 bytes
    with pytest.raises(ValueError):
        acc.add_msm(([], []), ([b"\x01" * 31], [base]))            # a scalar of 31 bytes
    with pytest.raises(ValueError):
        acc.add_msm(([1 << 256], [base]), ([], []))                # a scalar that does not fit 32 bytes


def test_no_device_no_accumulator():
    """Without a HIP device there is no context to carry an accumulator, and no CPU path takes its place; with or without one, the
    entry points refuse a missing context instead of inventing one."""
    import ctypes
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import _lib
    with pytest.raises(TypeError):
        h2v.Accumulator(None)
    out = ctypes.c_void_p()
    assert _lib.load_library().h2v_accumulator_create(None, ctypes.byref(out)) == -16 and not out.value
    if h2v.device_count() == 0:
        srs = open(os.path.join(ROOT, "tests", "golden", "kzg_bn254_8.srs"), "rb").read()
        params = srs[:4] + srs[4:68] + srs[-256:]
        with pytest.raises(h2v.H2VError) as e:
            h2v.Accumulator(h2v.Context(h2v.ParamsKZG(params, h2v.SerdeFormat.RawBytes)))
        assert e.value.code == -18
