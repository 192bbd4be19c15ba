"""The threading contract of include/h2v.h: host threads sharing one context.

The scenes of tests/thread_scenes.py — up to eight threads released by a barrier into one-shot calls, staged batches, accumulators
and MSM objects of their own on a shared context (or two) — are played once by tests/thread_driver.py in a fresh child process, and
every call's result is compared bit for bit with its expectation, which comes from the references alone.  Each scene also has a
condition that keeps it from passing by accident: its calls did overlap.  No scene uses one batch, accumulator or MSM object from two
threads at once: that is outside the contract (tests/test_thread_scenes_host.py checks the schedules).

A scene the driver did not reach fails with the threads' progress slots: which call each thread was in when the deadline expired."""
import json
import os
import pickle
import subprocess
import sys

import pytest

import thread_scenes as ts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    """the scenes, and the driver's report of each: one child process for the whole module"""
    work = str(tmp_path_factory.mktemp("threads"))
    data = ts.build()
    with open(os.path.join(work, "scenes.pkl"), "wb") as f:
        pickle.dump(data, f)
    run = subprocess.run([sys.executable, os.path.join(HERE, "thread_driver.py"), work], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    reports = {}
    for scene in data["scenes"]:
        path = os.path.join(work, scene["name"] + ".json")
        if os.path.exists(path):
            reports[scene["name"]] = json.load(open(path))
    stuck = json.load(open(os.path.join(work, "stuck.json"))) if os.path.exists(os.path.join(work, "stuck.json")) else None
    return {"scenes": {s["name"]: s for s in data["scenes"]}, "reports": reports, "stuck": stuck, "returncode": run.returncode, "output": run.stdout[-4000:]}


def _report(played, name):
    if name not in played["reports"]:
        pytest.fail(f"the driver did not finish scene {name!r} (exit status {played['returncode']}); progress slots: {played['stuck']}\n{played['output']}", pytrace=False)
    return played["scenes"][name], played["reports"][name]


def _short(v):
    text = repr(v)
    return text if len(text) < 400 else text[:200] + " ... " + text[-200:]


def _check_results(scene, report):
    """every call equals its expectation bit for bit"""
    bad = []
    for k, (rep, got) in enumerate(zip(scene["reps"], report["reps"])):
        rows = [(t, i, c, got["threads"][t][i]) for t, th in enumerate(rep["threads"]) for i, c in enumerate(th)]
        rows += [("main", i, c, got["main"][i]) for i, c in enumerate(rep["main_after"])]
        for t, i, c, r in rows:
            if r is None:
                bad.append(f"rep {k} thread {t} call {i} ({c['op']}): not made")
            elif c["error"] is not None:
                if r["error"] is None or r["error"][0] != c["error"][0] or not r["error"][1].endswith(c["error"][1]):
                    bad.append(f"rep {k} thread {t} call {i} ({c['op']}): expected the refusal {c['error']}, got {_short(r['error'] or r['result'])}")
            elif r["error"] is not None or not ts.matches(r["result"], c["expect"]):
                bad.append(f"rep {k} thread {t} call {i} ({c['op']}): got {_short(r['error'] or r['result'])}, the reference says {_short(c['expect'])}")
        for r in got["replays"]:
            bad.insert(0, f"rep {k} thread {r['thread']} call {r['index']} ({r['op']}) replayed alone on fresh objects: " +
                       ("AGREES with the reference: the failure depends on the concurrency" if r["alone_ok"] else "disagrees as well: not a matter of threads"))
    assert not bad, "%d mismatches\n%s" % (len(bad), "\n".join(bad[:12]))


def _intervals(got):
    return [(r["t0"], r["t1"], t) for t, th in enumerate(got["threads"]) for r in th if r is not None]


def overlap_share(report):
    """the share of calls that began while another thread's call was in progress"""
    began, total = 0, 0
    for got in report["reps"]:
        iv = _intervals(got)
        for t0, _, t in iv:
            total += 1
            began += any(u != t and a <= t0 < b for a, b, u in iv)
    return began / max(total, 1)


def _check_overlap(report):
    share = overlap_share(report)
    print(f"{report['name']}: {sum(len(_intervals(g)) for g in report['reps'])} calls, {share:.0%} began inside another thread's call, "
          f"peak threads in one symbol {max(v['peak'] for v in report['symbols'].values())}, {report['seconds']:.2f} s")
    assert share >= 0.5, share


def test_first_use(played):
    scene, report = _report(played, "first_use")
    _check_results(scene, report)
    _check_overlap(report)
    for k, got in enumerate(report["reps"]):      # on every fresh context at least two threads' FIRST calls overlapped
        first = [(th[0]["t0"], th[0]["t1"]) for th in got["threads"]]
        assert any(a[0] <= b[0] < a[1] for x, a in enumerate(first) for y, b in enumerate(first) if x != y), (k, first)


def test_staged(played):
    scene, report = _report(played, "staged")
    _check_results(scene, report)
    _check_overlap(report)


def test_plan_churn(played):
    scene, report = _report(played, "plan_churn")
    _check_results(scene, report)
    _check_overlap(report)
    assert ts.churn_shapes_under_pins(scene) > ts.MAX_CACHED_PLANS      # from the schedule, not measured


def test_oneshot_mix(played):
    scene, report = _report(played, "oneshot_mix")
    _check_results(scene, report)
    _check_overlap(report)


def test_two_contexts(played):
    scene, report = _report(played, "two_contexts")
    _check_results(scene, report)
    _check_overlap(report)
    # each ordered pair of contexts was called from both sides during the same round: the calls of a round lie between two barriers,
    # so both sides' calls of round r began before either side's call of round r + 1
    rep, got = scene["reps"][0], report["reps"][0]
    for a, b in ((0, 1), (2, 3), (4, 5), (6, 7)):
        rounds = {}
        for t in (a, b):
            for c, r in zip(rep["threads"][t], got["threads"][t]):
                if c["round"] is not None:
                    rounds.setdefault(c["round"], {})[t] = (c["args"]["order"], r)
        assert len(rounds) >= 30
        for k in sorted(rounds):
            (on_a, ra), (on_b, rb) = rounds[k][a], rounds[k][b]
            assert on_a == list(reversed(on_b)) and on_a[0] != on_a[1], (k, on_a, on_b)      # (A, B) against (B, A)
            if k + 1 in rounds:
                assert max(ra["t0"], rb["t0"]) <= min(v[1]["t0"] for v in rounds[k + 1].values()), k


def test_feeders(played):
    scene, report = _report(played, "feeders")
    _check_results(scene, report)
    _check_overlap(report)


def test_errors(played):
    scene, report = _report(played, "errors")
    _check_results(scene, report)
    _check_overlap(report)
    refusals = sum(1 for th in scene["reps"][0]["threads"] for c in th if c["error"])
    assert refusals >= 100 and report["symbols"]["h2v_last_error"]["calls"] >= refusals


def test_hand_over(played):
    scene, report = _report(played, "hand_over")
    _check_results(scene, report)
    # the batch's calls never overlapped: an upload on one thread, the launch on the next, the finish on a third
    got = report["reps"][0]
    uses = sorted((r["t0"], r["t1"]) for th in got["threads"][:3] for r in th)
    assert all(a[1] <= b[0] for a, b in zip(uses, uses[1:]))


def test_same_call(played):
    scene, report = _report(played, "same_call")
    _check_results(scene, report)
    _check_overlap(report)


def test_every_entry_point_was_entered_by_two_threads_at_once(played):
    """every symbol of _lib.SIGNATURES that the scenes call from two threads: in some scene two threads were inside it at once"""
    from halo2_verifier_amd import _lib
    for name in ts.SCENES:
        _report(played, name)
    peak, wanted = {}, set()
    for name, report in played["reports"].items():
        for sym, v in report["symbols"].items():
            peak[sym] = max(peak.get(sym, 0), v["peak"])
        wanted |= {sym for sym, threads in ts.symbols_reached(played["scenes"][name]).items() if threads >= 2}
    wanted -= set(ts.EXCLUDED)
    assert wanted == set(_lib.SIGNATURES) - set(ts.EXCLUDED)
    print({sym: peak.get(sym, 0) for sym in sorted(wanted)})
    alone = sorted(sym for sym in wanted if peak.get(sym, 0) < 2)
    assert not alone, alone
