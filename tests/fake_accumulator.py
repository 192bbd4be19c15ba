"""A stand-in for verifier.Accumulator in the non-GPU orchestration tests of distributed.ShardedAccumulator: it computes nothing,
records the calls it gets, and answers with values that depend on everything it was given, so that ranks which were handed different
states, another order or other draws disagree.  (The product has no CPU path: this is test code only.)"""
import hashlib

from halo2_verifier_amd.verifier import Accumulator


class FakeParams:
    def __init__(self, data):
        self.data = data


class FakeContext:
    device = 0

    def __init__(self, params=b"params"):
        self.params = FakeParams(params)


class FakeAccumulator:
    created = []     # every instance, in creation order

    def __init__(self, ctx, journal=0):
        self.ctx, self.journal, self.calls, self.closed = ctx, journal, [], False
        self.tag = 0
        self.merged = None
        FakeAccumulator.created.append(self)

    def process(self, tag):
        self.tag = self.tag * 31 + tag

    def export_state(self):
        left = hashlib.sha256(b"L%d" % self.tag).digest() * 2
        right = hashlib.sha256(b"R%d" % self.tag).digest() * 2
        return Accumulator.pack_state(left, right, self.tag % 1000, 0)

    def merge_states(self, states, draws=None):
        states, draws = [bytes(s) for s in states], [bytes(d) for d in draws]
        if len(states) + 1 > self.journal:
            raise AssertionError("the merged accumulator's journal is too small")
        self.calls.append(("merge_states", states, draws))
        self.merged = (states, draws)
        return draws

    def finalize(self):
        h = hashlib.sha256(b"".join(self.merged[0]) + b"".join(self.merged[1])).digest()
        return True, h * 2, h[::-1] * 2

    def check_legs(self):
        return [(0, 0, True)] + [(Accumulator.unpack_state(s)[2], 0, Accumulator.unpack_state(s)[2] % 2 == 0) for s in self.merged[0]]

    def close(self):
        self.closed = True
