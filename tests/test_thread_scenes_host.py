"""What the scenes of tests/thread_scenes.py promise (no GPU): tests/test_gpu_threads.py plays exactly thread_scenes.build(), so the
conditions here are requirements on ITS inputs.  The scenes are deterministic; no schedule gives one batch, accumulator or MSM object
to two threads at once; every call has an expectation of the shape the driver compares; every entry point of the C ABI is reached by
two threads of a scene or excluded with a reason; and the threading paragraph of include/h2v.h names exactly the entry points that
take a context's lock, which a scan of csrc/*.hip derives."""
import glob
import os
import pickle
import re

import pytest

import thread_scenes as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return ts.build()


def _reps(built):
    return [(s["name"], k, rep) for s in built["scenes"] for k, rep in enumerate(s["reps"])]


def test_the_same_seed_gives_the_same_bytes(built):
    """the two cheapest scenes built again from a fresh world: the same bytes, proofs included"""
    w = ts.World(ts.SEED)
    try:
        again = {"hand_over": ts.scene_hand_over(w, ts.SEED), "feeders": ts.scene_feeders(w, ts.SEED)}
        other = ts.scene_hand_over(w, ts.SEED + 1)
    finally:
        w.free()
    first = {s["name"]: s for s in built["scenes"]}
    for name, scene in again.items():
        assert pickle.dumps(scene) == pickle.dumps(first[name]), name
    assert pickle.dumps(other) != pickle.dumps(first["hand_over"])
    assert built["keys"] == w.keys


def test_the_scenes_are_the_ones_the_gpu_test_names(built):
    assert tuple(s["name"] for s in built["scenes"]) == ts.SCENES
    for name, k, rep in _reps(built):
        assert 1 <= len(rep["threads"]) <= ts.MAX_THREADS, (name, k)
        assert all(rep["threads"]), (name, k)
    reps = {s["name"]: s["reps"] for s in built["scenes"]}
    assert len([r for r in reps["first_use"] if r["tag"] == "a"]) >= 5 and len([r for r in reps["first_use"] if r["tag"] == "b"]) >= 5
    assert all(len(r["threads"]) == 8 for r in reps["first_use"] + reps["staged"])
    # first use (b): eight different first calls
    for r in reps["first_use"]:
        if r["tag"] == "b":
            assert len({th[0]["op"] for th in r["threads"]}) == 8
    # staged: about 20 uses of its batch per thread, by every route, with every reader and both kinds of regrouping
    for th in reps["staged"][0]["threads"]:
        ops = [c["op"] for c in th]
        assert ops.count("b_finish_groups") >= 20
        assert {"b_upload", "b_upload_launch", "b_upload_tensors", "b_finish_into", "b_recheck", "b_identify", "b_set_group_sizes", "b_set_groups"} <= set(ops)
    assert ts.churn_shapes_under_pins({"reps": reps["plan_churn"]}) == 40 > ts.MAX_CACHED_PLANS
    assert sum(1 for th in reps["plan_churn"][0]["threads"] if th[0]["op"] == "verify_batch_shapes") == 2
    assert all(len(c["args"]["shapes"]) == 12 for th in reps["plan_churn"][0]["threads"] for c in th if c["op"] == "verify_batch_shapes")
    mix = {c["op"] for th in reps["oneshot_mix"][0]["threads"] for c in th}
    assert {"verify_batch", "verify_batch_identify", "verify_batch_seeded", "verify_batches", "verify_each", "guard_msm", "guards_check_each", "msm_g1",
            "pairing_check", "msm_append", "msm_scale", "msm_scalars", "msm_eval_many", "dual_check_many", "b_finish_groups", "a_process",
            "a_process_guards", "a_add_msm", "a_finalize"} <= mix
    two = reps["two_contexts"][0]
    assert max(c["round"] for c in two["threads"][0] if c["round"] is not None) + 1 >= 30
    for a, b in ((0, 1), (2, 3), (4, 5), (6, 7)):       # the same call, the contexts the other way round, in every round
        ra = [(c["op"], c["args"]["order"]) for c in two["threads"][a] if c["round"] is not None]
        rb = [(c["op"], list(reversed(c["args"]["order"]))) for c in two["threads"][b] if c["round"] is not None]
        assert ra == rb and len(ra) >= 30 and ra[0][1] in (["A", "B"], ["B", "A"])
    assert len(reps["feeders"][0]["threads"]) == 4 and [c["op"] for c in reps["feeders"][0]["main_after"]] == ["a_merge", "a_read", "a_finalize", "merge_local"]
    for th in reps["feeders"][0]["threads"]:
        assert {"a_process", "a_process_guards", "a_process_batch"} <= {c["op"] for c in th}
    hand = reps["hand_over"][0]
    assert [len(th) for th in hand["threads"][:3]] == [10, 10, 10]
    assert [th[0]["op"] for th in hand["threads"]] == ["b_upload", "b_launch", "b_finish_groups", "a_process"] and hand["main_after"][0]["op"] == "a_finalize"


def test_no_object_is_given_to_two_threads_at_once(built):
    """over the schedule itself: two calls that use one object from two threads are ordered by `after` edges or the final join"""
    shared = 0
    for name, k, rep in _reps(built):
        assert ts.shared_object_conflicts(rep) == [], (name, k)
        for t, i, c in ts.all_calls(rep):
            if c["after"] is not None:
                shared += 1
                assert name == "hand_over"
            on = c["on"] if isinstance(c["on"], list) else [c["on"]]
            kinds = {spec[0] for spec in rep["objects"]}
            assert all(x in c["uses"] for x in on if x in kinds), (name, k, t, i, c["op"])     # what a call is made on, it uses
    assert shared >= 29
    # and the check can fail: thread 1's launch of round 3 without its wait for thread 0's upload
    hand = pickle.loads(pickle.dumps([s for s in built["scenes"] if s["name"] == "hand_over"][0]["reps"][0]))
    hand["threads"][1][3]["after"] = None
    assert ts.shared_object_conflicts(hand)


def test_every_thread_has_inputs_of_its_own(built):
    """no two threads of a repetition share a proof's bytes with the same draw, so a result delivered to the wrong thread is a mismatch"""
    for name, k, rep in _reps(built):
        expects = {}
        for t, i, c in ts.all_calls(rep):
            if c["expect"] is not None and c["op"] in ("verify_batch", "msm_g1", "b_finish_groups", "a_finalize", "verify_batch_keys", "b_finish"):
                if c["op"] == "b_finish_groups" and set(c["expect"][2]) == {ts.canon(ts.ZERO)}:
                    continue                # (every proof of the launch refused by its status: no point of anybody's)
                key = pickle.dumps(c["expect"])
                assert expects.setdefault(key, t) == t, (name, k, t, i, c["op"])


def test_every_expectation_is_there_and_has_the_shape_the_driver_compares(built):
    returns_nothing = {"msm_append", "msm_scale", "msm_add_msm", "b_set_groups", "b_set_group_sizes", "b_upload", "b_upload_launch", "b_upload_tensors",
                       "b_launch", "a_process_guards", "a_add_msm", "a_add_msms", "b_export", "b_fold_enqueue", "b_set_stream", "a_journal_begin", "a_drop_legs"}
    seen, defects = set(), set()
    for name, k, rep in _reps(built):
        for t, i, c in ts.all_calls(rep):
            seen.add(c["op"])
            assert c["op"] in ts.OP_SYMBOLS
            if c["error"] is not None:
                assert c["expect"] is None and c["error"][0] in (ts.BAD_ARGUMENT, ts.UNSUPPORTED) and c["error"][1]
            elif c["op"] in returns_nothing:
                assert c["expect"] is None, (name, c["op"])
            else:
                assert c["expect"] is not None, (name, k, t, i, c["op"])
                assert ts.canon(c["expect"]) == c["expect"] and ts.matches(c["expect"], c["expect"])      # plain data, as JSON holds it
                if c["op"] in ("verify_batch", "verify_batch_seeded", "verify_batch_identify", "verify_batch_keys", "b_finish"):
                    ok, st, left, right = c["expect"]
                    assert isinstance(ok, bool) and all(isinstance(v, int) for v in st)
                    assert left == ts.ANY or len(left) == 128
                    defects |= {v for v in st if v}
                if c["op"] == "b_finish_groups":
                    oks, st, lefts, rights = c["expect"]
                    assert len(oks) == len(lefts) == len(rights) and all(len(p) == 128 for p in lefts + rights)
                    if not all(oks) and not any(st):
                        defects.add("pairing")
    assert seen == set(ts.OP_SYMBOLS)
    assert "pairing" in defects and -5 in defects          # a tampered evaluation or a wrong input; a scalar that is not canonical
    assert not ts.matches([1, "ab"], [1, "ac"]) and ts.matches([1, "ab"], [1, ts.ANY]) and not ts.matches(True, 1)
    # OS draws: only statuses and verdicts are expected
    os_calls = [c for _, _, rep in _reps(built) for _, _, c in ts.all_calls(rep) if c["op"] == "verify_batch" and c["args"]["rand"] is None]
    assert os_calls and all(c["expect"][2:] == [ts.ANY, ts.ANY] for c in os_calls)
    # a zero draw among the uploads
    assert any(bytes(32) in [c["args"]["rand"][j:j + 32] for j in range(0, len(c["args"]["rand"]), 32)]
               for _, _, rep in _reps(built) for _, _, c in ts.all_calls(rep) if c["op"] == "b_upload")


def test_every_entry_point_is_in_a_scene_or_excluded_with_a_reason(built):
    from halo2_verifier_amd import _lib
    reach = {}
    for scene in built["scenes"]:
        for sym, threads in ts.symbols_reached(scene).items():
            reach[sym] = max(reach.get(sym, 0), threads)
    assert set(reach) <= set(_lib.SIGNATURES)
    assert set(ts.EXCLUDED) <= set(_lib.SIGNATURES) and all(isinstance(r, str) and len(r) > 10 for r in ts.EXCLUDED.values())
    missing = sorted(sym for sym in _lib.SIGNATURES if sym not in ts.EXCLUDED and reach.get(sym, 0) < 2)
    assert not missing, f"entry points that no scene calls from two threads and that are not excluded: {missing}"
    # the refusals of the errors scene: five kinds in every thread, each with a text of that thread's own
    errors = [s for s in built["scenes"] if s["name"] == "errors"][0]["reps"][0]
    texts = []
    for th in errors["threads"]:
        mine = {tuple(c["error"]) for c in th if c["error"]}
        assert len(mine) == 5 and sum(1 for c in th if c["error"]) * 2 == len(th)      # a successful call between two refusals
        texts.append(mine)
    assert all(a != b for x, a in enumerate(texts) for b in texts[x + 1:])


# ------------------------------------------------------------------ the header's threading paragraph against the sources
def _strip(src):
    src = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)


def _closing(src, at, opening, closing):
    depth = 0
    for k in range(at, len(src)):
        if src[k] == opening:
            depth += 1
        elif src[k] == closing:
            depth -= 1
            if depth == 0:
                return k
    raise ValueError(at)


def _definitions(src):
    """name -> body, of the functions and structs defined at the left margin"""
    out = {}
    for m in re.finditer(r"^struct (\w+)[^;{()]*\{", src, re.M):
        out[m.group(1)] = out.get(m.group(1), "") + src[m.end():_closing(src, m.end() - 1, "{", "}")]
    for m in re.finditer(r"^(?!namespace|extern|struct|typedef|using|#|return)[A-Za-z_][\w:<>\*&, ]*?[ \*&](\w+)\(", src, re.M):
        close = _closing(src, m.end() - 1, "(", ")")
        rest = re.match(r"\s*(?:const\s*)?\{", src[close + 1:])
        if rest:
            start = close + rest.end()
            out[m.group(1)] = out.get(m.group(1), "") + src[start:_closing(src, start, "{", "}")]
    return out


def lock_takers():
    """the entry points from which a context's lock is reached: a body that names `->mu` of a context (lock_guard<std::mutex>
    lock(ctx->mu), ScratchBatch's member, CtxLocks' loop; VkDevice::mu and split_mu are other locks), and every body that names one
    of those, to the fixed point"""
    defs = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "halo2_verifier_amd", "csrc", "*.hip"))):
        for name, body in _definitions(_strip(open(path).read())).items():
            defs[name] = defs.get(name, "") + body
    reach = {n for n, b in defs.items() if re.search(r"(?<!vk)->mu\b", b)}
    seeds = set(reach)
    grew = True
    while grew:
        grew = False
        for n, b in defs.items():
            if n not in reach and any(re.search(r"\b%s\b" % r, b) for r in reach):
                reach.add(n)
                grew = True
    return seeds, reach, defs


def test_the_header_names_exactly_the_entry_points_that_take_a_contexts_lock():
    from halo2_verifier_amd import _lib
    seeds, reach, defs = lock_takers()
    assert set(_lib.SIGNATURES) <= set(defs)                      # the scan saw every entry point's body
    assert {"ScratchBatch", "CtxLocks", "h2v_msm_g1", "h2v_pairing_check"} <= seeds and "run_group_batches" in reach
    assert "h2v_batch_launch" not in reach and "h2v_accumulator_finalize" not in reach
    derived = {n for n in reach if n in _lib.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "h2v.h")).read()
    para = header[header.index(" *   - Threading:"):header.index(" */\n#ifndef H2V_H")]
    lines = para.split("They are:\n")[1].split("\n")
    named = set()
    for line in lines:
        if not re.fullmatch(r" \*\s+(h2v_\w+[,.]\s*)+", line):
            break
        named |= set(re.findall(r"h2v_\w+", line))
    assert named == derived, (sorted(named - derived), sorted(derived - named))
    # what the paragraph says beside the list: several locks in a row, the tuning, one thread at a time, the error text
    for phrase in ("address order", "several times in a row", "one thread at a time", "per thread", "while the context is\n *     idle"):
        assert phrase in para, phrase
    # the calls that take the lock several times in a row do so by calling locking entry points one after another, not nested
    assert len(re.findall(r"\bh2v_msm_g1\(", defs["verify_seeded"])) == 2 and "h2v_pairing_check(" in defs["verify_seeded"]
    assert len(re.findall(r"\bh2v_msm_g1\(", defs["h2v_accumulator_add_msm"])) == 2
