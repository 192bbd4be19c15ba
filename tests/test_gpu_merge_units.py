"""The fold of a merge, k_accumulator_merge_fold (csrc/util.hip), alone against Python big integers (tests/merge_reference.py).
build/util_units merge_fold (tests/cpp/util_units.hip, built by csrc/Makefile with the library's flags) runs the kernel through the library's
own launcher on raw limbs chosen here, with the outputs between guard bands that the harness checks.

K = 0, 1, 2, 7, 8, 63, 64, 65, 129 and 512 records, each with the team the host rule picks and with the team forced to 1, 8 and 64
lanes (a forced team smaller than K + 1 gives every lane several items; a larger one leaves lanes without any).  Beside random items:
identity items, the previous accumulator (item 0) the identity, equal neighbours and all items equal (the doubling branch of the
complete addition, inside a lane's own loop and at every butterfly level), P beside -P at every butterfly level, and the scatter of
the records into journal slots — without a journal, without a map, and through a map whose slots are out of order.
The accumulator is compared as a pair of group elements; a journal slot is the record's point word for word, and a slot no record owns
keeps its preset.  One child process for all jobs, under a time limit."""
import random
import struct

import numpy as np
import pytest

import merge_reference as mr
import msm_reference as ref
import record_reference as rr
from msm_reference import R
import units_harness as uh

pytestmark = pytest.mark.gpu

KS = [0, 1, 2, 7, 8, 63, 64, 65, 129, 512]
TEAMS = [0, 1, 8, 64]           # 0: the host rule
REPS3 = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
P_MOD = ref.P


def _points(count, seed):
    rnd = random.Random(seed)
    pt, step = ref.mul(rnd.randrange(1, R), ref.G), ref.mul(rnd.randrange(1, R), ref.G)
    out = []
    for _ in range(count):
        out.append(pt)
        pt = ref.add(pt, step)
    return out


POOL = None


def _pool():
    global POOL
    if POOL is None:
        POOL = _points(40, 4242)
    return POOL


def _point_words(pt, rnd):
    """27 words of a stored Jacobian form of pt: a random Z and random representatives; the identity as (0, 1, 0) or as garbage X and Y over Z = 0"""
    reps = rnd.choice(REPS3)
    if pt is None:
        if rnd.random() < 0.5:
            return ref.jac_words(None, reps=reps)
        return ref.fq_words(rnd.randrange(1, P_MOD), reps[0]) + ref.fq_words(rnd.randrange(1, P_MOD), reps[1]) + ref.fq_words(0, reps[2])
    return ref.jac_words(pt, 1 if rnd.random() < 0.2 else rnd.randrange(2, P_MOD), reps)


class Job:
    """one launch: acc and items as affine points (None: the identity)"""

    def __init__(self, name, rnd, team, acc, records, n_slots=0, slots=None, with_sums=None):
        self.name, self.team, self.acc, self.records, self.slots = name, team, tuple(acc), list(records), slots
        self.with_sums = (n_slots > 0) if with_sums is None else with_sums
        self.n_slots = n_slots
        n = len(self.records)
        self.acc_words = [_point_words(p, rnd) for p in self.acc]
        junk = _pool()
        self.rec_words = []
        for k, (left, right) in enumerate(self.records):
            # failed words that a fold must not count, pieces 1 .. 5 that it must not read
            w = [(5 * k) % 3, 1, 0, 0]
            for pt in (left, right):
                w += _point_words(pt, rnd)
                for j in range(rr.PIECES - 1):
                    w += ref.jac_words(junk[(k + j) % len(junk)])
            assert len(w) == rr.RECORD_WORDS
            self.rec_words.append(w)
        assert n <= mr.MERGE_MAX and (not self.with_sums or n_slots >= n)

    def blob(self):
        n = len(self.records)
        out = [struct.pack("<5I", n, self.team, int(self.with_sums), int(self.slots is not None), self.n_slots)]
        if self.slots is not None:
            out.append(np.asarray(self.slots, dtype="<u4").tobytes())
        for w in self.acc_words:
            out.append(np.asarray(w, dtype="<u4").tobytes())
        for w in self.rec_words:
            out.append(np.asarray(w, dtype="<u4").tobytes())
        return b"".join(out)

    def out_words(self):
        return 1 + 2 * 27 + (2 * self.n_slots * 27 if self.with_sums else 0)

    def check(self, got):
        n = len(self.records)
        team = self.team or mr.host_team(n)
        assert int(got[0]) == team, self.name
        want, written = mr.merge_fold(self.acc, self.records, self.slots)
        for side in (0, 1):
            words = [int(v) for v in got[1 + 27 * side: 1 + 27 * side + 27]]
            assert rr.in_range(words), (self.name, side)
            assert ref.jac_point(words) == want[side], (self.name, side)
        if not self.with_sums:
            return
        sums = got[1 + 54:]
        for slot in range(self.n_slots):
            for side in (0, 1):
                words = [int(v) for v in sums[27 * (2 * slot + side): 27 * (2 * slot + side) + 27]]
                if slot in written:
                    k = (self.slots.index(slot) if self.slots is not None else slot)
                    assert words == self.rec_words[k][4 + side * 27 * rr.PIECES: 4 + side * 27 * rr.PIECES + 27], (self.name, slot, side)
                else:
                    assert words == [0xffffffff] * 27, (self.name, slot, side)


def _jobs():
    rnd = random.Random(777)
    pool = _pool()
    jobs = []

    def pick(allow_identity=True):
        return rnd.choice(pool + ([None] * 4 if allow_identity else []))

    # every K with every team: random items, a journal through an out-of-order map on the host-rule launch
    for K in KS:
        for team in TEAMS:
            recs = [(pick(), pick()) for _ in range(K)]
            if team == 0:
                n_slots = K + 3
                slots = rnd.sample(range(n_slots), K)
                jobs.append(Job(f"random K={K} host rule, mapped", rnd, 0, (pick(False), pick(False)), recs, n_slots, slots))
            else:
                jobs.append(Job(f"random K={K} team {team}", rnd, team, (pick(False), pick(False)), recs))
    # the scatter without a map (slot k = k), and a journal array with no records
    for K in (0, 1, 9, 65):
        recs = [(pick(), pick()) for _ in range(K)]
        jobs.append(Job(f"unmapped K={K}", rnd, 0, (pick(), pick()), recs, K + 2, None, with_sums=True))
    a, b = pool[0], pool[1]
    for K in (1, 2, 7, 8, 65):
        for team in sorted({mr.host_team(K), 1, 8, 64}):
            tag = f"K={K} team {team}"
            # identity items only; item 0 the identity; everything the identity
            jobs.append(Job("identity records " + tag, rnd, team, (a, b), [(None, None)] * K))
            jobs.append(Job("identity accumulator " + tag, rnd, team, (None, None), [(pick(False), pick(False)) for _ in range(K)]))
            jobs.append(Job("all identity " + tag, rnd, team, (None, None), [(None, None)] * K))
            # all K items equal, the accumulator too: doublings in the lanes' loops and at every butterfly level
            jobs.append(Job("all equal " + tag, rnd, team, (a, b), [(a, b)] * K))
            # two equal neighbours among distinct points (items j, j + 1 for every j in turn would be K jobs: the first, a middle and the last pair)
            for j in sorted({0, K // 2, K - 1}):
                items = [(pool[2 + (2 * i) % 30], pool[3 + (2 * i) % 30]) for i in range(K + 1)]
                items[j + 1 if j + 1 <= K else j] = items[j]
                jobs.append(Job(f"equal neighbours at {j} " + tag, rnd, team, items[0], items[1:]))
            # P beside -P at every butterfly level d: item 0 is P, item d is -P, the rest identities — and the same with the rest random
            d = team // 2
            while d >= 1:
                if d <= K:
                    items = [(None, None)] * (K + 1)
                    items[0], items[d] = (a, b), (ref.neg(a), ref.neg(b))
                    jobs.append(Job(f"P, -P at level {d} " + tag, rnd, team, items[0], items[1:]))
                    items = [(pick(), pick()) for _ in range(K + 1)]
                    items[d] = (ref.neg(items[0][0]) if items[0][0] else None, ref.neg(items[0][1]) if items[0][1] else None)
                    jobs.append(Job(f"P, -P among others at level {d} " + tag, rnd, team, items[0], items[1:]))
                d //= 2
    # every pair cancels: the sum is the identity at 512 records, on every lane
    recs = []
    for i in range(256):
        p, q = pool[i % 40], pool[(i + 7) % 40]
        recs += [(p, ref.neg(q)), (ref.neg(p), q)]
    jobs.append(Job("cancelling pairs K=512", rnd, 0, (None, None), recs))
    return jobs


def _run(blob, tmp_path, timeout=120):
    return uh.as_words(uh.run("util_units", ["merge_fold"], blob, tmp_path, timeout))


def test_host_rule():
    assert [mr.host_team(k) for k in KS] == [1, 2, 4, 8, 16, 64, 64, 64, 64, 64]
    assert mr.dependent_additions(512, 64) == (9, 6) and mr.dependent_additions(8, mr.host_team(8)) == (1, 4)


def test_merge_fold_against_big_integers(tmp_path):
    jobs = _jobs()
    got = []
    for at in range(0, len(jobs), 200):             # (the harness takes at most 256 jobs per run)
        part = jobs[at:at + 200]
        out = _run(struct.pack("<I", len(part)) + b"".join(j.blob() for j in part), tmp_path)
        assert len(out) == sum(j.out_words() for j in part)
        pos = 0
        for j in part:
            got.append(out[pos:pos + j.out_words()])
            pos += j.out_words()
    for j, g in zip(jobs, got):
        j.check(g)
