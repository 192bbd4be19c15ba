"""The readers that every C++ caller program shares (tests/cpp/caller.h), on their own and without a GPU: tests/cpp/caller_selftest.cpp,
a stand-alone program built with the address and undefined-behaviour sanitizers, reads a directory written by caller_harness.items_text
and guards_text and prints what it parsed in the format it read, so the printout must equal the files; a malformed file must end it
with status 2, a message on stderr and nothing on stdout."""
import pytest

import caller_harness as ch


def _v(k):
    return bytes((k + j) % 256 for j in range(32))


PROOFS = [bytes(range(40)), b"\x00\xff" * 33, bytes([7]), bytes(range(200, 256))]
INSTANCES = [[],                                   # no instance columns
             [[]],                                 # one column of length 0: "-" for no values
             [[_v(1), _v(2), _v(3)], [_v(4)]],     # two columns of unequal length
             [[], [_v(5)], []]]
KEYS = [0, 2, 1, 2]
GUARDS = [dict(left_scalars=[_v(9)], left_bases=[_v(10) + _v(11)], right_scalars=[_v(12), _v(13)], right_bases=[_v(14) * 2, _v(15) * 2]),
          dict(left_scalars=[], left_bases=[], right_scalars=[_v(16)], right_bases=[_v(17) * 2]),      # an empty array: "-"
          dict(left_scalars=[], left_bases=[], right_scalars=[], right_bases=[])]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    # (it calls nothing of the library: the stand-in is linked so that the program loads no other)
    return ch.build("caller_selftest", tmp_path_factory.mktemp("caller_selftest"), sanitize=True, stubs=("h2v_stub",))


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "unkeyed"])
def test_the_printout_equals_the_input(selftest, tmp_path, keyed):
    items, guards = ch.items_text(PROOFS, INSTANCES, keys=KEYS if keyed else None), ch.guards_text(GUARDS)
    assert items.splitlines()[0] == ("3 4" if keyed else "4")
    assert items.splitlines()[1:3] == [("0 " if keyed else "") + "0 " + PROOFS[0].hex() + " -", ("2 " if keyed else "") + "1 0 " + PROOFS[1].hex() + " -"]
    assert guards.splitlines()[2] == "- - - -"
    ch.write_dir(tmp_path, items_txt=items, guards_txt=guards)
    r = ch.run(selftest, [tmp_path, "keyed" if keyed else "unkeyed", "guards"], timeout=120)
    assert r.stdout == items + guards
    assert ch.run(selftest, [tmp_path, "keyed" if keyed else "unkeyed"], timeout=120).stdout == items
    # no proof at all is a file like any other
    ch.write_dir(tmp_path, items_txt=ch.items_text([], [], keys=[] if keyed else None), guards_txt="")
    assert ch.run(selftest, [tmp_path, "keyed" if keyed else "unkeyed", "guards"], timeout=120).stdout == ("1 0\n" if keyed else "0\n")


def _line(key, inst, proof_hex, inst_hex):
    return " ".join([str(key), str(len(inst))] + [str(l) for l in inst] + [proof_hex, inst_hex])


GOOD = _line(0, [1, 2], "aabb", "cd" * 96)
MALFORMED = {
    "a_word_of_odd_length": ("1 2\n" + GOOD + "\n" + _line(0, [1, 2], "aab", "cd" * 96) + "\n", None),
    "an_instance_word_of_odd_length": ("1 1\n" + _line(0, [1], "aabb", "cd" * 31 + "c") + "\n", None),
    "a_word_that_is_not_hex": ("1 2\n" + GOOD + "\n" + _line(0, [1, 2], "aabg", "cd" * 96) + "\n", None),
    "a_signed_word": ("1 1\n" + _line(0, [1, 2], "+1", "cd" * 96) + "\n", None),
    "fewer_lines_than_the_header_promises": ("1 3\n" + GOOD + "\n" + GOOD + "\n", None),
    "a_line_cut_short": ("1 2\n" + GOOD + "\n0 2 1 2 aabb\n", None),
    "a_header_alone": ("1 1\n", None),
    "no_header": ("", None),
    "instance_bytes_one_value_short": ("1 1\n" + _line(0, [1, 2], "aabb", "cd" * 64) + "\n", None),
    "instance_bytes_one_value_long": ("1 1\n" + _line(0, [1, 2], "aabb", "cd" * 128) + "\n", None),
    "instance_bytes_one_byte_long": ("1 1\n" + _line(0, [1, 2], "aabb", "cd" * 97) + "\n", None),
    "no_instance_bytes_for_a_column_of_one": ("1 1\n" + _line(0, [1], "aabb", "-") + "\n", None),
    "instance_bytes_without_a_column": ("1 1\n" + _line(0, [], "aabb", "cd" * 32) + "\n", None),
    "a_key_the_header_does_not_count": ("1 1\n" + _line(1, [1, 2], "aabb", "cd" * 96) + "\n", None),
    "a_guard_line_of_three_words": ("1 1\n" + GOOD + "\n", "aa bb cc dd\naa bb cc\n"),
    "a_guard_word_that_is_not_hex": ("1 1\n" + GOOD + "\n", "aa bb cc dd\naa bb zz dd\n"),
    "a_guard_word_of_odd_length": ("1 1\n" + GOOD + "\n", "aa bb cc ddd\n"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_a_malformed_file_is_refused_with_status_2(selftest, tmp_path, name):
    items, guards = MALFORMED[name]
    ch.write_dir(tmp_path, items_txt=items, guards_txt=guards if guards is not None else "")
    r = ch.run(selftest, [tmp_path, "keyed"] + (["guards"] if guards is not None else []), timeout=120, allow_fail=True)
    assert (r.returncode, r.stdout) == (2, "") and r.stderr.strip(), (name, r.returncode, r.stdout[:200], r.stderr[-2000:])


def test_a_missing_file_is_refused_with_status_2(selftest, tmp_path):
    r = ch.run(selftest, [tmp_path, "unkeyed"], timeout=120, allow_fail=True)
    assert (r.returncode, r.stdout) == (2, "") and "items.txt" in r.stderr
    ch.write_dir(tmp_path, items_txt="0\n")
    r = ch.run(selftest, [tmp_path, "unkeyed", "guards"], timeout=120, allow_fail=True)
    assert (r.returncode, r.stdout) == (2, "") and "guards.txt" in r.stderr
