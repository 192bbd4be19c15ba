"""The two kernels of h2v_accumulator_process_batch that are its own, alone against Python big integers (tests/legs_reference.py):
k_leg_weights (csrc/verify_kernels.hip) and k_accumulator_legs_fold (csrc/util.hip), through build/legs_units (tests/cpp/legs_units.hip,
built by csrc/Makefile with the library's flags), each through the library's own launcher, the outputs between guard bands.

k_leg_weights: G in 1, 2, 63, 64, 65, 256, 512 (every level of the suffix scan over 512 values in LDS), equal groups and unequal
offsets; M_g programmed to 0, 1, r - 1 and random through the group's first draw and its first proof's multiplier, each placed in the
first, a middle and the last group; the draws and multipliers of the other proofs are random and must not be read.
k_accumulator_legs_fold: G + 1 in 1, 2, 3, 64, 65, 513 records with the host's team and forced teams; records that are identities,
all equal, and each other's negatives at every butterfly level; the accumulator it must REPLACE preset to a point that is not in the
sum; the unscaled pairs into journal slots without a journal, without a map, and through a map out of order.
The accumulator is compared as a pair of group elements; a journal slot is the leg's pair word for word, and a slot no leg owns keeps
its preset.  One child process per kernel, under a time limit."""
import random
import struct

import pytest

import legs_reference as lr
import merge_reference as mr
import msm_reference as ref
import record_reference as rr
from msm_reference import R
import units_harness as uh

pytestmark = pytest.mark.gpu

GS = [1, 2, 63, 64, 65, 256, 512]
NS = [1, 2, 3, 64, 65, 513]
REPS3 = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
P_MOD = ref.P


def _scalar_words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


class WeightsJob:
    def __init__(self, name, rnd, G, ragged, programmed=None):
        self.name, self.G = name, G
        if ragged:
            sizes = [rnd.randrange(1, 6) for _ in range(G)]
            self.off, self.gs = lr.offsets(sizes)[:-1], 0
            n = sum(sizes)
        else:
            self.gs = rnd.randrange(1, 5)
            self.off, n = None, G * self.gs
        self.n = n
        self.draws = [rnd.randrange(R) for _ in range(n)]
        self.mult = [rnd.randrange(R) for _ in range(n)]
        first = self.off if ragged else [g * self.gs for g in range(G)]
        for g, v in (programmed or {}).items():
            f = first[g]
            if rnd.random() < 0.5:
                self.draws[f], self.mult[f] = v, 1
            elif v in (0, 1):
                self.draws[f], self.mult[f] = (rnd.randrange(1, R) if v == 0 else 1), v
            else:
                self.draws[f] = rnd.randrange(1, R)
                self.mult[f] = v * pow(self.draws[f], -1, R) % R
        self.M = lr.leg_products([self.draws[f] for f in first], [self.mult[f] for f in first])
        for g, v in (programmed or {}).items():
            assert self.M[g] == v

    def blob(self):
        out = [struct.pack("<4I", self.G, self.n, int(self.off is not None), self.gs)]
        if self.off is not None:
            out.append(uh.words(self.off))
        out.append(b"".join(d.to_bytes(32, "little") for d in self.draws))
        out.append(b"".join(m.to_bytes(32, "little") for m in self.mult))
        return b"".join(out)

    def out_words(self):
        return 8 * (self.G + 1) + 8 * self.G

    def check(self, got):
        total, W = lr.leg_weights(self.M)
        want = _scalar_words(total)
        for w in W:
            want += _scalar_words(w)
        for m in self.M:
            want += _scalar_words(m)
        assert [int(v) for v in got] == want, self.name


def _weights_jobs():
    rnd = random.Random(991)
    jobs = []
    for G in GS:
        for ragged in (False, True):
            tag = f"G={G} {'unequal' if ragged else 'equal'}"
            jobs.append(WeightsJob("random " + tag, rnd, G, ragged))
            for v in (0, 1, R - 1):
                for g in sorted({0, G // 2, G - 1}):
                    jobs.append(WeightsJob(f"M_{g} = {v if v < 2 else 'r - 1'} " + tag, rnd, G, ragged, {g: v}))
            jobs.append(WeightsJob("all one " + tag, rnd, G, ragged, {g: 1 for g in range(G)}))
            jobs.append(WeightsJob("all r - 1 " + tag, rnd, G, ragged, {g: R - 1 for g in range(G)}))
    return jobs


def _split(jobs, out):
    assert len(out) == sum(j.out_words() for j in jobs)
    pos = 0
    for j in jobs:
        yield j, out[pos:pos + j.out_words()]
        pos += j.out_words()


def _run_all(mode, jobs, tmp_path):
    for at in range(0, len(jobs), 200):             # (the harness takes at most 256 jobs per run)
        part = jobs[at:at + 200]
        out = uh.as_words(uh.run("legs_units", [mode], struct.pack("<I", len(part)) + b"".join(j.blob() for j in part), tmp_path, 120))
        for j, g in _split(part, out):
            j.check(g)


def test_leg_weights_against_big_integers(tmp_path):
    _run_all("weights", _weights_jobs(), tmp_path)


# ---- the fold
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
        POOL = _points(40, 2424)
    return POOL


JUNK_WORDS = {}


def _junk_words(i):
    if i not in JUNK_WORDS:
        JUNK_WORDS[i] = ref.jac_words(_pool()[i])
    return JUNK_WORDS[i]


def _point_words(pt, rnd):
    """27 words of a stored Jacobian form of pt: a random Z and random representatives; the identity as (0, 1, 0) or as garbage X and Y over Z = 0"""
    reps = rnd.choice(REPS3)
    if pt is None:
        if rnd.random() < 0.5:
            return ref.jac_words(None, reps=reps)
        return ref.fq_words(rnd.randrange(1, P_MOD), reps[0]) + ref.fq_words(rnd.randrange(1, P_MOD), reps[1]) + ref.fq_words(0, reps[2])
    return ref.jac_words(pt, 1 if rnd.random() < 0.2 else rnd.randrange(2, P_MOD), reps)


class FoldJob:
    """one launch: records and unscaled pairs as affine points (None: the identity)"""

    def __init__(self, name, rnd, team, records, n_slots=0, slots=None, with_sums=None):
        self.name, self.team, self.records, self.slots, self.n_slots = name, team, list(records), slots, n_slots
        self.with_sums = (n_slots > 0) if with_sums is None else with_sums
        n = len(self.records)
        assert 1 <= n <= lr.MAX_GROUPS + 1 and (not self.with_sums or n_slots >= n - 1)
        junk = _pool()
        # the accumulator as it stands: a point the fold must not add
        self.acc_words = [_point_words(junk[7], rnd), _point_words(junk[8], rnd)]
        self.rec_words = []
        for k, (left, right) in enumerate(self.records):
            w = [(5 * k) % 3, 1, 0, 0]          # failed words that the fold must not count, pieces 1 .. 5 that it must not read
            for pt in (left, right):
                w += _point_words(pt, rnd)
                for j in range(rr.PIECES - 1):
                    w += _junk_words((k + j) % len(junk))
            assert len(w) == rr.RECORD_WORDS
            self.rec_words.append(w)
        self.pairs = [(rnd.choice(junk + [None]), rnd.choice(junk + [None])) for _ in range(n - 1)] if self.with_sums else []
        self.pair_words = [[_point_words(p, rnd) for p in pr] for pr in self.pairs]

    def blob(self):
        n = len(self.records)
        out = [struct.pack("<5I", n, self.team, int(self.with_sums), int(self.slots is not None), self.n_slots)]
        if self.slots is not None:
            out.append(uh.words(self.slots))
        for w in self.acc_words + self.rec_words:
            out.append(uh.words(w))
        for pr in self.pair_words:
            out.append(uh.words(pr[0]) + uh.words(pr[1]))
        return b"".join(out)

    def out_words(self):
        return 1 + 2 * 27 + (2 * self.n_slots * 27 if self.with_sums else 0)

    def check(self, got):
        n = len(self.records)
        assert int(got[0]) == (self.team or mr.host_team(n - 1)), self.name
        want, written = lr.legs_fold(self.records, self.pairs if self.with_sums else None, self.slots)
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
                    g = self.slots.index(slot) if self.slots is not None else slot
                    assert words == self.pair_words[g][side], (self.name, slot, side)
                else:
                    assert words == [0xffffffff] * 27, (self.name, slot, side)


def _fold_jobs():
    rnd = random.Random(778)
    pool = _pool()
    jobs = []

    def pick(allow_identity=True):
        return rnd.choice(pool + ([None] * 4 if allow_identity else []))

    a, b = pool[0], pool[1]
    for n in NS:
        recs = [(pick(), pick()) for _ in range(n)]
        # the host's team with a journal through a map out of order; without a map; without a journal; forced teams
        n_slots = n + 2
        jobs.append(FoldJob(f"random n={n} host rule, mapped", rnd, 0, recs, n_slots, rnd.sample(range(n_slots), n - 1)))
        jobs.append(FoldJob(f"random n={n} host rule, unmapped", rnd, 0, recs, n_slots, None, with_sums=True))
        for team in ((0, 1, 8, 64) if n < 64 else (0, 8)):      # (a forced team smaller than n gives every lane several records)
            tag = f"n={n} team {team}"
            jobs.append(FoldJob("random " + tag, rnd, team, [(pick(), pick()) for _ in range(n)]))
            jobs.append(FoldJob("all identity " + tag, rnd, team, [(None, None)] * n))
            jobs.append(FoldJob("all equal " + tag, rnd, team, [(a, b)] * n))
            # P beside -P at every butterfly level d: record 0 is P, record d is -P, the rest identities, and the same among random records
            d = (team or mr.host_team(n - 1)) // 2
            while d >= 1:
                if d < n:
                    items = [(None, None)] * n
                    items[0], items[d] = (a, b), (ref.neg(a), ref.neg(b))
                    jobs.append(FoldJob(f"P, -P at level {d} " + tag, rnd, team, items))
                    items = [(pick(False), pick(False)) for _ in range(n)]
                    items[d] = (ref.neg(items[0][0]), ref.neg(items[0][1]))
                    jobs.append(FoldJob(f"P, -P among others at level {d} " + tag, rnd, team, items))
                d //= 2
    # every pair cancels: the sum is the identity at 512 records, on every lane
    recs = []
    for i in range(256):
        p, q = pool[i % 40], pool[(i + 7) % 40]
        recs += [(p, ref.neg(q)), (ref.neg(p), q)]
    jobs.append(FoldJob("cancelling pairs n=512", rnd, 0, recs))
    return jobs


def test_legs_fold_against_big_integers(tmp_path):
    _run_all("legs_fold", _fold_jobs(), tmp_path)
