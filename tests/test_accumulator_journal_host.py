"""The leg journal's host side without a GPU: the Python class checks every capacity and entry index before it makes any C call, and
identify() refuses to run without the legs' retained inputs."""
import pytest

from test_accumulator_host import _unbacked


def test_journal_begin_validates_the_capacity_before_any_c_call():
    acc, _ = _unbacked()
    for capacity in (-1, 1, 4097, 2.0, "8", None, True):
        with pytest.raises(ValueError):
            acc.journal_begin(capacity)


def test_constructor_validates_the_capacity_before_any_c_call():
    from halo2_verifier_amd import verifier
    _, ctx = _unbacked()
    for capacity in (-1, 1, 4097, 2.5):
        with pytest.raises(ValueError):
            verifier.Accumulator(ctx, journal=capacity)


def test_drop_legs_validates_the_indices_before_any_c_call():
    acc, _ = _unbacked()
    with pytest.raises(ValueError):
        acc.drop_legs([-1])                                        # a negative index
    with pytest.raises(ValueError):
        acc.drop_legs([1, 2.0])                                    # not an integer
    with pytest.raises(ValueError):
        acc.drop_legs(["1"])
    with pytest.raises(ValueError):
        acc.drop_legs([1, 2, 1])                                   # given twice
    with pytest.raises(ValueError):
        acc.drop_legs([0])                                         # the base
    acc._inputs = [None, None, None]                               # a journal of three entries
    with pytest.raises(ValueError):
        acc.drop_legs([3])                                         # past the journal's end


def test_identify_needs_retained_inputs():
    acc, _ = _unbacked()
    with pytest.raises(ValueError):
        acc.identify()


def test_header_and_mirrors_agree_on_the_journal_limit():
    import os
    import re
    from halo2_verifier_amd import verifier
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "h2v.h")).read()
    assert int(re.search(r"#define H2V_ACC_JOURNAL_MAX (\d+)", text).group(1)) == verifier.Accumulator.JOURNAL_MAX == 4096
