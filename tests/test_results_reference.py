"""tests/results_reference.py on small cases written out by hand (no GPU)."""
import results_reference as rr


def test_decode_maps_the_four_rank_codes_and_passes_the_rest():
    assert [rr.decode(w) for w in (0, -40, -30, -20, -10)] == [0, -1, -5, -7, -4]
    assert [rr.decode(w) for w in (-2, -123456, 7, -(1 << 31))] == [-2, -123456, 7, -(1 << 31)]


def test_the_rank_codes_are_the_headers():
    """the table against csrc/batch.h and include/h2v.h, read as text"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    batch_h = open(os.path.join(root, "halo2_verifier_amd", "csrc", "batch.h")).read()
    h2v_h = open(os.path.join(root, "include", "h2v.h")).read()
    dev = {k: int(v) for k, v in re.findall(r"#define H2V_DEV_ST_(\w+) \((-\d+)\)", batch_h)}
    abi = {k: int(v) for k, v in re.findall(r"#define H2V_ERR_(\w+) \((-\d+)\)", h2v_h)}
    want = {dev["INVALID_INSTANCES"]: abi["INVALID_INSTANCES"], dev["TRANSCRIPT"]: abi["TRANSCRIPT"], dev["PANIC"]: abi["REFERENCE_PANIC"],
            dev["OPENING"]: abi["OPENING"], 0: 0}
    assert want == rr.DECODE
    assert int(re.search(r"#define H2V_SUMMARY_WORDS (\d+)", h2v_h).group(1)) == rr.SUMMARY_WORDS


def test_counts_of_equal_groups():
    words = [0, -10, 0, 0, -30, -30, 0, 0]
    assert rr.group_failed(words, 1) == [3]
    assert rr.group_failed(words, 2) == [1, 2]
    assert rr.group_failed(words, 4) == [1, 0, 2, 0]
    assert rr.group_failed(words, 8) == [0, 1, 0, 0, 1, 1, 0, 0]
    assert rr.group_failed([], 3) == [0, 0, 0]


def test_counts_of_unequal_groups():
    words = [-10, 0, 0, -20, 0, 5, 0]
    assert rr.group_failed(words, sizes=[1, 3, 2, 1]) == [1, 1, 1, 0]
    assert rr.group_failed(words, sizes=[2, 1, 4]) == [1, 0, 2]


def test_group_ok_needs_all_three_and_no_fault():
    failed, fold, ok = [0, 1, 0, 0], [0, 0, 2, 0], [1, 1, 1, 0]
    assert rr.group_ok(failed, fold, ok, pairing=True) == [1, 0, 0, 0]
    assert rr.group_ok(failed, fold, ok, pairing=False) == [1, 0, 0, 1]          # (the pairing's word is not looked at)
    assert rr.group_ok(failed, fold, [0xdead, 0, 7, 0], pairing=False) == [1, 0, 0, 1]
    assert rr.group_ok(failed, fold, ok, pairing=True, fault=3) == [0, 0, 0, 0]


def test_indices_ascend_and_stop_at_the_cap():
    words = [0, -10, -10, 0, 9, 0, -40]
    assert rr.failed_index(words) == [1, 2, 4, 6]
    assert rr.failed_index(words, 2) == [1, 2]
    assert rr.failed_index(words, 4) == [1, 2, 4, 6]
    assert rr.failed_index(words, 9) == [1, 2, 4, 6]
    assert rr.failed_index([0, 0]) == []


def test_bytes_and_summary():
    blob = bytes(range(128)) + bytes(range(128, 256))
    left, right = rr.split_xy(blob, 2)
    assert left == bytes(range(64)) + bytes(range(128, 192)) and right == bytes(range(64, 128)) + bytes(range(192, 256))
    words = [0, -10, 0, 0]
    got = rr.finish(words, [0, 0], [1, 1], blob, rr.FLAG_PAIRING, groups=2, cap=1)
    assert got == {"status": [0, -4, 0, 0], "group_ok": [0, 1], "left_xy": left, "right_xy": right, "group_failed": [1, 0], "failed_index": [1],
                   "summary": [rr.NO_FAULT, 1, 1, 4, 2, 1, 0, 0]}
    got = rr.finish(words, [0, 0], [1, 1], blob, rr.FLAG_PAIRING | rr.FLAG_FOLDED, sizes=[1, 3], fault=2)
    assert got["group_ok"] == [0, 0] and got["group_failed"] == [0, 1] and got["summary"] == [2, 1, 0, 4, 2, 3, 0, 0]
    assert rr.finish([], [0], [1], bytes(128), 0)["summary"] == [rr.NO_FAULT, 0, 1, 0, 1, 0, 0, 0]
