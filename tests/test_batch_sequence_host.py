"""What the committed sequences of tests/batch_sequence.py cover (no GPU): tests/test_gpu_batch_sequence.py runs exactly
batch_sequence.CASES, so the conditions here are requirements on ITS inputs — it cannot quietly test less than it claims.  Also: the
generator is deterministic, and the model refuses exactly what the stage table of csrc/batch.hip refuses."""
import collections
import os
import re

import pytest

import batch_sequence as bs
from batch_sequence import EMPTY, UPLOADED, LAUNCHED, FINISHED, READERS, ROUTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# readers the stage table admits directly behind a launch; the others need a finished launch and are looked for directly behind the
# finish that follows a launch
AT_LAUNCHED = ("finish", "finish_groups", "finish_into", "export")
AFTER_FINISH = ("recheck", "identify", "process_batch")
FAILING_KINDS = ("upload", "upload_launch", "deferred")
# (the last one: h2v_batch_set_group_sizes sends the offsets to the device itself, and only an upload from device memory relies on that;
# the upload brings its draws and the launch has a pairing, so that multipliers, folded scalars and counts all show the offsets)
GROUP_CHANGES = ["equal->ragged", "ragged->equal", "up", "down", "only the sizes change, then an upload from device memory"]


def _runs(cases=bs.CASES):
    return [bs.run_model(bs.sequence(seed, steps, focus)) for seed, focus, steps in cases]


def coverage(cases=bs.CASES):
    """-> dict of Counters over all cases"""
    cov = collections.defaultdict(collections.Counter)
    for run in _runs(cases):
        prev_route = prev_n = launch_route = None
        prev_reader = None            # the reader of the step directly before
        groups, ragged = 1, False
        after_launch = None           # route, directly behind its launch
        after_finish = None           # route, directly behind the finish / finish_groups that directly followed its launch
        n_chain = []
        pending = {}                  # failing kind -> what it still waits for ("upload", then "read")
        relaunch_ready = False
        last_pairing = None
        second_in_flight = False
        sizes, resized = None, None   # resized: unequal groups whose sizes alone changed -> "armed", then "uploaded" by a device route
        for step, before, out in run:
            op, kw, ok = step.op, step.kw, out.kind == "ok"
            cov["kinds"][out.kind] += 1
            if op == "illegal":
                cov["illegal"][(before, kw["call"])] += 1
            if op == "upload" and kw.get("bad_draw") is not None:
                kind = kw["route"] if kw["route"] in bs.HOST_ROUTES else "deferred"
                cov["failing"][kind] += 1
                pending[kind] = "upload"
            if second_in_flight and op not in ("ctx_call", "second_start", "second_finish"):
                cov["second"]["in flight across a step"] += 1
            if op == "second_start":
                second_in_flight = True
            if op == "second_finish":
                second_in_flight = False
            if op in ("set_groups", "set_group_sizes"):
                now_ragged, g = op == "set_group_sizes", len(kw["sizes"]) if op == "set_group_sizes" else kw["groups"]
                if ragged != now_ragged:
                    cov["groups"]["ragged->equal" if ragged else "equal->ragged"] += 1
                elif not ragged and g != groups:
                    cov["groups"]["up" if g > groups else "down"] += 1
                groups, ragged = g, now_ragged
                resized = "armed" if (op == "set_group_sizes" and sizes is not None and len(sizes) == g and sum(sizes) == sum(kw["sizes"]) and sizes != kw["sizes"]) else None
                sizes = list(kw["sizes"]) if now_ragged else None
            if op == "upload" and ok and kw.get("bad_draw") is None:
                if prev_route is not None:
                    cov["routes"][(prev_route, kw["route"])] += 1
                if prev_n is not None:
                    cov["n_class"][(bs.n_class(prev_n), bs.n_class(kw["n"]))] += 1
                n_chain.append(kw["n"])
                resized = "uploaded" if (resized == "armed" and kw["route"] == "device" and kw["draws"] == "random") else None
                prev_route, prev_n = kw["route"], kw["n"]
                for k, v in pending.items():
                    if v == "upload":
                        pending[k] = "read"
            launched = ok and (op == "launch" or (op == "upload" and kw["route"] == "upload_launch"))
            if ok and op == "launch":
                if before == FINISHED:
                    cov["launch"]["after finish"] += 1
                launch_route = out.view.up["route"]
            if ok and op == "upload" and kw["route"] == "upload_launch":
                launch_route = "upload_launch"
            if launched:
                last_pairing = out.view.pairing
            if op == "ctx_call":
                cov["ctx"][kw["kind"]] += 1
            if ok and op in ("finish", "finish_groups") and out.view.up["route"] != "device_os":
                up = out.view.up
                cov["finished"][("draws", up["draws"])] += 1
                cov["finished"][("content", up["content"])] += 1
                if up["draws"] == "alternating" and up["content"] == "clean" and all(sz % 2 == 0 for sz in bs.group_sizes(up["n"], out.view.groups, out.view.sizes)):
                    cov["finished"]["identity accumulators"] += 1
            if ok and op == "finish_into" and out.view.fault is not None and "summary" in kw["outputs"]:
                cov["finished"]["a draw fault in the summary"] += 1
            if ok and op == "identify" and out.view.up["content"] in ("input", "sign", "two"):
                cov["finished"]["identify names a proof"] += 1
            if ok and op in READERS:
                if after_launch is not None:
                    cov["after_launch"][(after_launch, op)] += 1
                if after_finish is not None:
                    cov["after_finish"][(after_finish, op)] += 1
                if prev_reader is not None:
                    cov["reader_pairs"][(prev_reader, op)] += 1
                if op == "finish_groups" and after_launch is not None and last_pairing is False:
                    cov["launch"]["no pairing, then finish_groups"] += 1
                if op in ("finish", "finish_groups") and resized == "uploaded" and out.view.pairing:
                    cov["groups"]["only the sizes change, then an upload from device memory"] += 1
                if op in ("finish", "finish_groups"):
                    for k, v in list(pending.items()):
                        if v == "read":
                            cov["recovered"][k] += 1
                            del pending[k]
            after_finish = after_launch if (ok and op in ("finish", "finish_groups") and after_launch is not None) else None
            after_launch = launch_route if launched else None
            prev_reader = op if (ok and op in READERS) else None
        for i in range(len(n_chain) - 2):
            if n_chain[i:i + 3] == [300, 255, 257]:
                cov["n_class"]["300 -> 255 -> 257"] += 1
    return cov


@pytest.fixture(scope="module")
def cov():
    return coverage()


def _missing(counter, wanted, least=1):
    return [w for w in wanted if counter[w] < least]


def test_every_route_follows_every_route(cov):
    assert not _missing(cov["routes"], [(a, b) for a in ROUTES for b in ROUTES])


def test_every_size_class_follows_every_size_class(cov):
    assert not _missing(cov["n_class"], [(a, b) for a in range(3) for b in range(3)] + ["300 -> 255 -> 257"])


def test_group_transitions(cov):
    assert not _missing(cov["groups"], GROUP_CHANGES)


def test_every_reader_directly_after_every_routes_launch(cov):
    assert not _missing(cov["after_launch"], [(r, op) for r in ROUTES for op in AT_LAUNCHED])
    assert not _missing(cov["after_finish"], [(r, op) for r in ROUTES for op in AFTER_FINISH])


def test_every_reader_directly_after_every_other_reader(cov):
    assert not _missing(cov["reader_pairs"], [(a, b) for a in READERS for b in READERS if a != b])


def test_every_illegal_call_at_every_stage_twice(cov):
    assert not _missing(cov["illegal"], bs.illegal_table(), least=2)
    assert set(cov["illegal"]) <= set(bs.illegal_table())


def test_every_failing_upload_is_followed_by_a_successful_upload_and_a_full_read(cov):
    assert not _missing(cov["failing"], FAILING_KINDS) and not _missing(cov["recovered"], FAILING_KINDS)


def test_relaunches_and_launches_without_a_pairing(cov):
    assert cov["launch"]["after finish"] >= 3 and cov["launch"]["no pairing, then finish_groups"] >= 3


def test_a_second_batch_in_flight(cov):
    assert cov["second"]["in flight across a step"] >= 6


DESIGNED = [("draws", k) for k in bs.DRAWS] + [("content", k) for k in bs.CONTENT] + ["identity accumulators", "a draw fault in the summary", "identify names a proof"]


def test_every_kind_of_input_is_finished_and_every_context_call_made(cov):
    """what tests/test_gpu_batch_sequence.py asserts it has seen: identity accumulators (alternating draws over duplicated pairs), two
    distinct statuses (an undecodable point, a non-canonical evaluation), a draw fault named by a device finish, a proof named by identify"""
    assert not _missing(cov["finished"], DESIGNED) and not _missing(cov["ctx"], bs.CTX_KINDS)


def test_the_shares_of_failures(cov):
    """about 15 % illegal calls and about 10 % failing uploads"""
    total = sum(cov["kinds"].values())
    assert 0.10 <= sum(cov["illegal"].values()) / total <= 0.20
    assert 0.05 <= sum(cov["failing"].values()) / total <= 0.15


def test_a_failure_is_followed_by_a_success_within_three_steps():
    for run in _runs():
        kinds = [out.kind for _, _, out in run]
        for i, k in enumerate(kinds[:-3]):
            if k != "ok":
                assert "ok" in kinds[i + 1:i + 4], (i, kinds)


@pytest.mark.parametrize("index", range(len(bs.CASES)))
def test_no_case_can_be_removed(index):
    """every committed case carries something a condition depends on"""
    c = coverage(bs.CASES[:index] + bs.CASES[index + 1:])
    lost = (_missing(c["routes"], [(a, b) for a in ROUTES for b in ROUTES]) + _missing(c["n_class"], [(a, b) for a in range(3) for b in range(3)] + ["300 -> 255 -> 257"]) +
            _missing(c["groups"], GROUP_CHANGES) + _missing(c["after_launch"], [(r, op) for r in ROUTES for op in AT_LAUNCHED]) +
            _missing(c["after_finish"], [(r, op) for r in ROUTES for op in AFTER_FINISH]) + _missing(c["reader_pairs"], [(a, b) for a in READERS for b in READERS if a != b]) +
            _missing(c["illegal"], bs.illegal_table(), least=2) + _missing(c["recovered"], FAILING_KINDS) + _missing(c["finished"], DESIGNED) +
            _missing(c["ctx"], bs.CTX_KINDS))
    assert lost or c["launch"]["after finish"] < 3 or c["launch"]["no pairing, then finish_groups"] < 3 or c["second"]["in flight across a step"] < 6


def test_the_large_sequence():
    """the scripted sequence above the overlapped upload's threshold: every route directly behind an h2v_batch_upload_launch that copied
    the points first, that upload behind itself, a relaunch of it, and nothing the model refuses"""
    run = bs.run_model(bs.large_sequence(), bs.LARGE_CAPACITY)
    assert all(out.kind == "ok" for _, _, out in run)
    ups = [s.kw for s, _, _ in run if s.op == "upload"]
    assert all(kw["n"] >= 2048 for kw in ups)
    assert {b["route"] for a, b in zip(ups, ups[1:]) if a["route"] == "upload_launch"} == set(ROUTES)
    ops = [s.op for s, _, _ in run]
    assert any(s.op == "upload" and s.kw["route"] == "upload_launch" and ops[i + 2] == "launch" for i, (s, _, _) in enumerate(run[:-2]))


def test_the_generator_is_deterministic():
    for seed, focus, steps in bs.CASES:
        assert bs.trace(bs.sequence(seed, steps, focus)) == bs.trace(bs.sequence(seed, steps, focus))
    assert bs.trace(bs.sequence(1, 30, "readers")) != bs.trace(bs.sequence(2, 30, "readers"))
    assert len({focus for _, focus, _ in bs.CASES}) == len(bs.FOCUSES)
    assert sorted(bs.SHUFFLED) == list(range(len(bs.CASES)))


def test_a_trace_line_is_python():
    class Recorder:
        def __getattr__(self, op):
            return lambda **kw: calls.append((op, kw))
    for seed, focus, steps in bs.CASES[:2]:
        seq, calls = bs.sequence(seed, steps, focus), []
        exec(bs.trace(seq), {"run": Recorder()})
        assert calls == [(s.op, s.kw) for s in seq]


# ---- the stage table, transcribed from csrc/batch.hip (require_stage: "every call accepts the stages from `least` on") and
# csrc/accumulator.hip (h2v_accumulator_process_batch: stage == Finished), and include/h2v.h's text on each entry point
STAGE_TABLE = {
    "launch": "Uploaded",            # h2v_batch_launch
    "finish": "Launched",            # h2v_batch_finish
    "finish_groups": "Launched",     # h2v_batch_finish_groups
    "finish_into": "Launched",       # h2v_batch_finish_device: "The batch must be launched or finished"
    "export": "Launched",            # h2v_batch_export_accumulators
    "recheck": "Finished",           # h2v_batch_recheck: "the last FINISHED launch"
    "identify": "Finished",          # h2v_batch_identify
    "process_batch": "Finished",     # h2v_accumulator_process_batch
}
WHO = {"h2v_batch_launch": "launch", "h2v_batch_finish": "finish", "h2v_batch_finish_groups": "finish_groups", "h2v_batch_finish_device": "finish_into",
       "h2v_batch_export_accumulators": "export", "h2v_batch_recheck": "recheck", "h2v_batches_recheck": "recheck", "h2v_batch_identify": "identify"}


def test_the_model_refuses_what_the_stage_table_refuses():
    for call, least in STAGE_TABLE.items():
        for stage in (EMPTY, UPLOADED, LAUNCHED, FINISHED):
            m = bs.Model()
            m.stage, m.zero = stage, [0]
            m.up = dict(route="upload", n=4, shape=8, draws="random", content="clean", seed=1)
            assert m.refuses(call, ranges=[(0, 1)]) == (stage < bs.STAGE_NAMES.index(least)), (call, stage)
    assert set(STAGE_TABLE) == set(bs.LEAST)


def test_the_transcribed_table_is_the_sources():
    """every require_stage(...) of csrc/batch.hip, by the name its error message carries"""
    src = open(os.path.join(ROOT, "halo2_verifier_amd", "csrc", "batch.hip")).read()
    found = {}
    for least, who in re.findall(r'require_stage\(\w+(?:\[k\])?, BatchStage::(\w+), (\w+|"[^"]+")\)', src):
        if who == "who":
            continue                 # (finish_impl / h2v_batch_finish_device / recheck_impl / identify: named where they are called)
        found[who.strip('"')] = least
    # the entry points that pass their name on
    assert re.search(r'static const char who\[\] = "h2v_batch_finish_device";\s+int rc;\s+if \(\(rc = require_stage\(b, BatchStage::Launched, who\)\)\)', src)
    assert re.search(r'int finish_impl\(.*\n\s+if \(int rc = require_stage\(b, BatchStage::Launched, who\)\)', src)
    assert re.search(r'require_stage\(batches\[k\], BatchStage::Finished, who\)', src)
    assert re.search(r'static const char who\[\] = "h2v_batch_identify";\s+int rc;\s+if \(\(rc = require_stage\(b, BatchStage::Finished, who\)\)\)', src)
    found.update({"h2v_batch_finish_device": "Launched", "h2v_batch_finish": "Launched", "h2v_batch_finish_groups": "Launched", "h2v_batches_recheck": "Finished",
                  "h2v_batch_identify": "Finished"})
    for who, least in found.items():
        if who in WHO:
            assert STAGE_TABLE[WHO[who]] == least, who
    assert {WHO[w] for w in found if w in WHO} == set(STAGE_TABLE) - {"process_batch"}
    acc = open(os.path.join(ROOT, "halo2_verifier_amd", "csrc", "accumulator.hip")).read()
    assert "if (b->stage != BatchStage::Finished)" in acc
    # include/h2v.h: what the header's text says of the same calls
    hdr = open(os.path.join(ROOT, "include", "h2v.h")).read()
    assert "The batch must be launched or finished" in hdr and "of the last FINISHED launch of b" in hdr
