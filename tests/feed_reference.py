"""The host bookkeeping of a resident accumulator with enqueued feeds (include/h2v_feed.h), modelled in Python: what
h2v_accumulator_feed_batch reserves when it is called, and what a settle commits or releases.

The journal holds `capacity` entries, the base included; entry e owns a slot of the device array, and the free slots are handed out
lowest first (accumulator.hip: free_slots, commit_entry).  A feed of G groups
  - is refused (UNSUPPORTED) if the entries, the legs of the feeds not settled yet and its own G do not fit, or if FEED_MAX_PENDING
    feeds wait for their report; a refusal changes nothing;
  - otherwise takes the G lowest free slots at once, in group order, so that nothing enqueued later can be given them.
A settle walks the unsettled feeds in feed order: a feed whose report says 0 appends (slot, size, failed) per group and adds n and
its failed proofs to the counters; a dropped feed (rc != 0: a draw >= r found on the device) gives its slots back, appends nothing
and adds n to BOTH counters.  process_batch is feed + settle with rc = 0.
"""
UNSUPPORTED, BAD_ARGUMENT = -19, -16
FEED_MAX_PENDING = 64


class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


class Model:
    def __init__(self, capacity=0):
        self.capacity = capacity
        self.entries = [(0, 0, 0)] if capacity else []          # (slot, n_proofs, n_failed), the base first
        self.free = list(range(capacity - 1, 0, -1))             # descending: the lowest is taken from the end
        self.n_proofs = self.n_failed = 0
        self.unsettled = []                                       # (sizes, slots)
        self.reports = []                                         # (rc, n, failed) not handed out yet

    @property
    def pending(self):
        return len(self.unsettled), len(self.unsettled) + len(self.reports)

    def feed(self, sizes):
        G = len(sizes)
        if not sum(sizes):
            return
        legs = sum(len(slots) for _, slots in self.unsettled)
        if self.capacity and len(self.entries) + legs + G > self.capacity:
            raise Refused(UNSUPPORTED)
        if len(self.unsettled) + len(self.reports) >= FEED_MAX_PENDING:
            raise Refused(UNSUPPORTED)
        slots = [self.free.pop() for _ in range(G)] if self.capacity else []
        self.unsettled.append((list(sizes), slots))

    def commit(self, outcomes):
        """the implicit settle of every other call: outcomes[i] = (rc, failed per group) of the i-th unsettled feed"""
        assert len(outcomes) == len(self.unsettled)
        for (sizes, slots), (rc, failed) in zip(self.unsettled, outcomes):
            n = sum(sizes)
            if rc == 0:
                for g, slot in enumerate(slots):
                    self.entries.append((slot, sizes[g], failed[g]))
                self.n_proofs += n; self.n_failed += sum(failed)
                self.reports.append((0, n, sum(failed)))
            else:
                self.free = sorted(self.free + slots, reverse=True)
                self.n_proofs += n; self.n_failed += n
                self.reports.append((rc, n, n))
        self.unsettled = []

    def settle(self, outcomes=()):
        self.commit(list(outcomes))
        out, self.reports = self.reports, []
        return out

    def process_batch(self, sizes, failed=None):
        assert not self.unsettled, "commit() the feeds' outcomes first: the model cannot know them"
        self.feed(sizes)
        if self.unsettled:
            self.commit([(0, failed or [0] * len(sizes))])
            self.reports.pop()   # process_batch returns its counts itself and leaves no report

    def drop(self, indices):
        gone = set(indices)
        assert 0 not in gone and all(e < len(self.entries) for e in gone)
        self.free = sorted(self.free + [self.entries[e][0] for e in gone], reverse=True)
        self.entries = [x for e, x in enumerate(self.entries) if e not in gone]
        self.n_proofs = sum(n for _, n, _ in self.entries); self.n_failed = sum(f for _, _, f in self.entries)

    def legs(self):
        """check_legs' first two columns"""
        return [(n, f) for _, n, f in self.entries]
