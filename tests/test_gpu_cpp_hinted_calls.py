"""The C++ mirror (include/h2v_hints.hpp) of the calls that take a hint row per proof or none: tests/cpp/hinted_calls.cpp runs
h2v_verify_batch_keys_hinted, h2v_accumulator_process_hinted, h2v_verify_batches_hinted and h2v_batch_set_hint_rows beside the same calls
without hints (include/h2v.hpp) over proofs of two VerifyingKeys whose numbers of points differ.  Each hinted line must be, word for
word, the line of the call without hints, and the counters those of tests/hints_reference.py."""
import random

import pytest

import caller_harness as ch
import circuits
import hints_reference as hr
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_hinted_calls_equal_the_unhinted_mirror(tmp_path):
    from halo2_verifier_amd import hints
    import halo2_verifier_amd as h2v
    exe = ch.build("hinted_calls", tmp_path)
    sv, ssh = circuits.setup_vector_mul(8, 8), circuits.setup_shuffle(8, s_seed=42)
    assert sv.params == ssh.params
    PV, IV = circuits.prove_vector_mul_batch(sv, 8, seed=61, threads=4)
    shuffles = [circuits.prove_shuffle(ssh, data_seed=5 + i, rng_seed=9 + i) for i in range(3)]
    vec = [(sv, p, i) for p, i in zip(PV, IV)]
    shf = [(ssh, p, i) for p, i in shuffles]
    items = [vec[0], shf[0], vec[1], vec[2], shf[1], vec[3], vec[4], shf[2], vec[5], vec[6], vec[7]]     # both keys have proofs with and without a row
    rnd = random.Random(62)
    rand = [rnd.randrange(1, R_MOD) for _ in items]
    offs = []
    for s in (sv, ssh):
        c = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
        offs.append(hints.point_offsets(c))
        c.close()
    assert len(offs[0]) != len(offs[1])

    def counters(sel):
        """rows for every proof but each third one of the call's order; all of them right"""
        pts = [len(offs[0] if s is sv else offs[1]) for s, _, _ in items]
        return sum(pts[j] for j in sel), sum(pts[j] for j in sel if j % 3 != 2), 0

    for case in ("good", "bad"):
        if case == "bad":   # an undecodable point in a proof that has a row: its hint (zeros) is the one miss
            j = 3
            assert items[j][0] is sv and j % 3 != 2
            bad = bytearray(items[j][1]); bad[offs[0][0]:offs[0][0] + 32] = hr.encode(hr.P + 9, 0)
            items[j] = (sv, bytes(bad), items[j][2])
        d = ch.write_dir(tmp_path, sv.params, vks=[sv.vk, ssh.vk], rand=rand, items_txt=ch.keyed_items_text(items, (sv, ssh)))
        out = ch.run(exe, [d]).stdout.splitlines()
        words = {l.split()[0]: l.split()[1:] for l in out if not l.startswith(("stats", "refused", "accepted"))}
        for call in ("keys", "process", "batches"):
            assert words[call + "_hinted"] == words[call], call
        ok, st, left, right = circuits.oracle_accumulate(items, rand)
        assert words["keys"] == [str(int(ok)), left.hex(), right.hex()] + [str(v) for v in st] and ok is (case == "good")
        miss = 0 if case == "good" else 1
        every = range(len(items))
        mine = [j for j in every if items[j][0] is sv]
        stats = {l.split()[1]: tuple(int(x) for x in l.split()[2:]) for l in ch.lines(out, "stats ")}
        want = counters(every)
        assert stats["keys"] == stats["process"] == (want[0], want[1], miss)
        wb = counters(mine)
        assert stats["batches"] == (wb[0], wb[1], miss)
        assert ch.lines(out, "staged_stats ") == ["staged_stats %d %d %d" % (wb[0], wb[1], miss)]
        assert ch.lines(out, ("refused", "accepted")) == ["refused a row one byte too long", "refused a draw too few"]
    sv.free(); ssh.free()
