"""Batch.set_group_sizes, the uploads behind it and Context.verify_batches check in Python every length the C side will index, before
they ask for the library.  No GPU."""
import pytest

import halo2_verifier_amd as h2v


class _Lib:
    def __getattr__(self, name):
        raise AssertionError(f"the C library must not be reached ({name})")


def _batch(max_proofs=64):
    b = object.__new__(h2v.Batch)
    b._lib, b._h, b.max_proofs, b.groups, b.group_sizes, b.n = _Lib(), None, max_proofs, 1, None, 0
    return b


def _ctx():
    c = object.__new__(h2v.Context)
    c._lib, c._h = _Lib(), None
    return c


S = (5).to_bytes(32, "little")


@pytest.mark.parametrize("sizes", [[3, 0, 2], [0], [4, -1]])
def test_a_zero_or_negative_size_is_refused(sizes):
    with pytest.raises(ValueError, match="at least one proof"):
        _batch().set_group_sizes(sizes)


@pytest.mark.parametrize("sizes", [[2.0, 3], ["4"], [None], [True, 2], [1.5]])
def test_a_size_that_is_no_integer_is_refused(sizes):
    with pytest.raises(TypeError, match="must be an integer"):
        _batch().set_group_sizes(sizes)


def test_group_count_and_capacity():
    with pytest.raises(ValueError, match="1 to 512 groups"):
        _batch(4096).set_group_sizes([1] * 513)
    with pytest.raises(ValueError, match="1 to 512 groups"):
        _batch().set_group_sizes([])
    with pytest.raises(ValueError, match="capacity"):
        _batch(10).set_group_sizes([5, 6])


def test_upload_needs_the_sum_of_the_sizes_and_one_draw_per_proof():
    b = _batch()
    b.groups, b.group_sizes = 3, [1, 2, 1]
    with pytest.raises(ValueError, match="sum to 4 proofs, got 3"):
        b.upload(b"\0" * 3072, 1024, b"\0" * 96, [1], b"\0" * 96)
    with pytest.raises(ValueError, match="sum to 4 proofs, got 5"):
        b.upload_launch(b"\0" * 5120, 1024, b"\0" * 160, [1])
    with pytest.raises(ValueError, match="one draw per proof"):
        b.upload(b"\0" * 4096, 1024, b"\0" * 128, [1], b"\0" * 160)
    with pytest.raises(ValueError, match="one draw per proof"):
        b.upload(b"\0" * 4096, 1024, b"\0" * 128, [1], b"\0" * 96)


def test_verify_batches_checks_before_the_library():
    p = b"\0" * 1024
    with pytest.raises(ValueError, match="at least one proof"):
        _ctx().verify_batches([([p], [[[S]]]), ([], [])])
    with pytest.raises(ValueError, match="instance lists in one batch"):
        _ctx().verify_batches([([p, p], [[[S]]])])
    with pytest.raises(ValueError, match="one scalar per proof"):
        _ctx().verify_batches([([p], [[[S]]]), ([p, p], [[[S]], [[S]]])], rand=[1, 2])
    with pytest.raises(ValueError, match="one instance shape"):
        _ctx().verify_batches([([p], [[[S]]]), ([p], [[[S, S]]])], rand=[1, 2])
    with pytest.raises(ValueError, match="exactly 32 bytes"):
        _ctx().verify_batches([([p], [[[S]]])], rand=[b"\1" * 8])
    with pytest.raises(TypeError):
        _ctx().verify_batches([(["not bytes"], [[[S]]])])
