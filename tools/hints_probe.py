"""What point hints (include/h2v_hints.h) do to the headline launch, 20 groups of 1024 proofs of the k = 14 pool, inputs resident:
   python tools/hints_probe.py [--k 14] [--groups 20] [--reps 15] [--out FILE] [--partial [--parent LIB]] [--oneshot]
One MI355X, one process, at least 50 ms of warm-up per variant; medians and min .. max of --reps repetitions of launch + finish_groups,
the variants alternating inside each repetition:
   none        no hints: the path of a build without hints, the baseline of every other row
   hits        right hints for every point
   one_miss    right hints except the first point of every wave of 64: the worst case of the in-kernel fallback
   misses      all-zero hints: every point pays the check and then the root
Hints are per upload and a launch leaves the canonical y where the hints lay, so every hinted repetition uploads again (untimed) and
sets its hints (untimed) before the timed launch; `none` uploads again too, so that all rows do the same outside the timed region.
Then, from separate profiled runs (Batch.set_profiling), the `decompress` entry of Batch.timings_ms() for the same four variants, and
the upload from device memory with and without set_hints_tensor (upload_tensors [+ set_hints_tensor] + launch + finish_groups): what
the 32 bytes per point cost on the way in.  Untimed: every variant returns the results of `none`, and hint_stats() is what the
variant is named for.

--partial (after the rows above, which stay as they are): hints from SOME senders (include/h2v_hint_rows.h).  Six rows — none, all
right, one wrong per wave, all wrong, every second proof without hints, one proof in eight without hints — on this build, and with
--parent LIB (a libh2v_amd.so built from the parent commit, loaded beside the in-tree one, as tools/accumulator_probe.py loads it) on
the parent's library too, where a proof without hints gets a zero row through h2v_batch_set_hints.  All variants of both libraries
alternate inside each repetition; medians and min .. max of --reps launches + finish_groups, then the `decompress` entry of
Batch.timings_ms() from profiled launches.  The session's spread is the `none` row's max - min.
--oneshot: a 1024-proof h2v_verify_batch_keys_hinted and a one-proof call, from host bytes with right rows, against the same calls
without hints on this build."""
import argparse, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import torch
import halo2_verifier_amd as h2v
from halo2_verifier_amd import hints

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--partial", action="store_true")
ap.add_argument("--parent", default=None)
ap.add_argument("--oneshot", action="store_true")
args = ap.parse_args()
assert args.reps >= 15, "at least 15 repetitions of each variant"

B, NPUB, G = 1024, bench.N_PUBLIC, args.groups
n = B * G
d = bench.load_or_make_proofs(B, args.k, print)
proofs, inst = d["proofs"] * G, d["inst"] * G
rand = b"".join(((i * 0x9e3779b97f4a7c15 + 0x1234567) % (1 << 250)).to_bytes(32, "little") for i in range(1, n + 1))
raw = h2v.SerdeFormat.RawBytes
ctx = h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw))
off = hints.point_offsets(ctx)
NP, ROW = len(off), 32 * len(off)
total = n * NP
right = hints.for_proofs(off, d["proofs"], 1024) * G
one_miss = bytearray(right)
for t in range(0, total, 64):
    one_miss[32 * t + 1] ^= 1          # (byte 1: the parity stays, only the curve check can tell)
HINTS = {"none": None, "hits": right, "one_miss": bytes(one_miss), "misses": bytes(len(right))}
MISSES = {"none": 0, "hits": 0, "one_miss": (total + 63) // 64, "misses": total}

batches = {v: h2v.Batch(ctx, n, NPUB, groups=G) for v in HINTS}


def prepare(v):
    b = batches[v]
    b.upload(proofs, 1024, inst, [NPUB], rand)
    if HINTS[v] is not None:
        b.set_hints(HINTS[v])


def timed(v):
    b = batches[v]
    t0 = time.perf_counter()
    b.launch()
    out = b.finish_groups(raw_statuses=True)
    return (time.perf_counter() - t0) * 1e3, out


prepare("none")
want = timed("none")[1]
assert all(want[0]) and want[1].count(0) == len(want[1])
for v in HINTS:
    prepare(v)
    assert timed(v)[1] == want, v
    assert batches[v].hint_stats() == (total, total if HINTS[v] is not None else 0, MISSES[v]), (v, batches[v].hint_stats())
t0 = time.perf_counter()
while time.perf_counter() - t0 < bench.WARM_S * 4 * 4:   # (launches are most of the loop: each variant for well over 50 ms)
    for v in HINTS:
        prepare(v); timed(v)
ts = {v: [] for v in HINTS}
for _ in range(args.reps):
    for v in HINTS:
        prepare(v)
        ts[v].append(timed(v)[0])

# the decompression stage alone: profiled launches (an event between the stages), apart from the timings above
stage = {v: [] for v in HINTS}
for v in HINTS:
    batches[v].set_profiling(True)
for _ in range(args.reps):
    for v in HINTS:
        prepare(v); timed(v)
        stage[v].append(batches[v].timings_ms()["decompress"])
for v in HINTS:
    batches[v].set_profiling(False)

# the way in from device memory, with and without the hints' 32 bytes per point
dev = "cuda:0"
t_proofs = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).reshape(n, 1024).to(dev)
t_inst = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, 32 * NPUB).to(dev)
t_rand = torch.frombuffer(bytearray(rand), dtype=torch.uint8).reshape(n, 32).to(dev)
t_hints = torch.frombuffer(bytearray(right), dtype=torch.uint8).reshape(n, ROW).to(dev)
torch.cuda.synchronize()


def from_device(with_hints):
    b = batches["hits" if with_hints else "none"]
    t0 = time.perf_counter()
    b.upload_tensors(t_proofs, t_inst, [NPUB], t_rand)
    if with_hints:
        b.set_hints_tensor(t_hints)
    b.launch()
    out = b.finish_groups(raw_statuses=True)
    return (time.perf_counter() - t0) * 1e3, out


DEVICE = {"device_upload": False, "device_upload_hinted": True}
for v, w in DEVICE.items():
    assert from_device(w)[1] == want, v
    for _ in range(12):
        from_device(w)
    ts[v] = []
for _ in range(args.reps):
    for v, w in DEVICE.items():
        ts[v].append(from_device(w)[0])


def row(t):
    s = sorted(t)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3)}


res = {"n": n, "groups": G, "k": args.k, "reps": args.reps, "n_points_per_proof": NP, "launch_finish": {v: row(t) for v, t in ts.items()},
       "decompress_stage_profiled": {v: row(t) for v, t in stage.items()}}
base = res["launch_finish"]["none"]
res["none_spread_ms"] = round(base["max_ms"] - base["min_ms"], 3)
res["hits_minus_none_ms"] = round(res["launch_finish"]["hits"]["median_ms"] - base["median_ms"], 3)
res["hits_faster_than_none_by_more_than_the_spread"] = -res["hits_minus_none_ms"] > res["none_spread_ms"]
lines = [f"{n} proofs in {G} groups, k = {args.k}, {NP} points per proof, {args.reps} repetitions, variants alternating", "launch + finish_groups:"]
lines += [f"  {v:21s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}  {n / r['median_ms'] / 1e3:6.2f} M proofs/s" for v, r in res["launch_finish"].items()]
lines += ["the decompress entry of Batch.timings_ms(), profiled launches:"]
lines += [f"  {v:21s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}" for v, r in res["decompress_stage_profiled"].items()]
lines += [f"hits - none: {res['hits_minus_none_ms']:+.3f} ms; the spread of none: {res['none_spread_ms']:.3f} ms; "
          f"faster by more than the spread: {res['hits_faster_than_none_by_more_than_the_spread']}"]


def partial_probe():
    """the six rows of --partial on this build and, with --parent, on the parent's library"""
    import ctypes
    from halo2_verifier_amd import _lib
    rows1 = [right[i * ROW:(i + 1) * ROW] for i in range(B)]
    skip = {"half": lambda i: i % 2 == 1, "eighth": lambda i: i % 8 == 7}
    KINDS = {"none": None, "all_right": right, "one_wrong_per_wave": bytes(one_miss), "all_wrong": bytes(len(right))}
    for name, without in skip.items():
        KINDS[name] = [None if without(i) else rows1[i % B] for i in range(n)]
    libs = {"this": (ctx, None)}
    if args.parent:
        plib = ctypes.CDLL(os.path.abspath(args.parent))
        for table in (_lib.SIGNATURES, hints.SIGNATURES):
            for name, (restype, argtypes) in table.items():
                if hasattr(plib, name):
                    fn = getattr(plib, name)
                    fn.restype, fn.argtypes = restype, argtypes
        mine = _lib.load_library()
        _lib._LIB = plib
        try:
            libs["parent"] = (h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw)), plib)
        finally:
            _lib._LIB = mine
    var = {}
    for lname, (c, plib) in libs.items():
        for kind, rows in KINDS.items():
            flat = rows if not isinstance(rows, list) else b"".join(r if r is not None else bytes(ROW) for r in rows)
            var[f"{lname}:{kind}"] = (h2v.Batch(c, n, NPUB, groups=G), plib, rows, flat)

    def prep(v):
        b, plib, rows, flat = var[v]
        b.upload(proofs, 1024, inst, [NPUB], rand)
        if rows is None:
            return
        if plib is not None:      # the parent: its own entry point, zero rows for the proofs without hints
            rc = plib.h2v_batch_set_hints(b._h, n, flat)
            assert rc == 0, (v, rc)
        elif isinstance(rows, list):
            b.set_hint_rows(rows)
        else:
            b.set_hints(rows)

    def run(v):
        b = var[v][0]
        t0 = time.perf_counter()
        b.launch()
        out = b.finish_groups(raw_statuses=True)
        return (time.perf_counter() - t0) * 1e3, out

    for v in var:
        prep(v)
        assert run(v)[1] == want, v
    null_points = {k: NP * sum(1 for i in range(n) if f(i)) for k, f in skip.items()}
    for kind, f in skip.items():
        assert var[f"this:{kind}"][0].hint_stats() == (total, total - null_points[kind], 0), (kind, var[f"this:{kind}"][0].hint_stats())
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < bench.WARM_S * 4 * len(var):
        for v in var:
            prep(v); run(v)
    tl = {v: [] for v in var}
    for _ in range(args.reps):
        for v in var:
            prep(v)
            tl[v].append(run(v)[0])
    st = {v: [] for v in var}
    for v in var:
        var[v][0].set_profiling(True)
    for _ in range(args.reps):
        for v in var:
            prep(v); run(v)
            st[v].append(var[v][0].timings_ms()["decompress"])
    out = {"launch_finish": {v: row(t) for v, t in tl.items()}, "decompress_stage_profiled": {v: row(t) for v, t in st.items()}}
    for lname in libs:
        r = out["launch_finish"][f"{lname}:none"]
        out[f"{lname}_none_spread_ms"] = round(r["max_ms"] - r["min_ms"], 3)
    text = [f"--partial: hints from some senders, {n} proofs in {G} groups, {args.reps} repetitions, all variants alternating", "launch + finish_groups:"]
    text += [f"  {v:28s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}" for v, r in out["launch_finish"].items()]
    text += ["the decompress entry of Batch.timings_ms(), profiled launches:"]
    text += [f"  {v:28s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}" for v, r in out["decompress_stage_profiled"].items()]
    text += [f"the spread of {l}:none (max - min): {out[l + '_none_spread_ms']:.3f} ms" for l in libs]
    for b, _, _, _ in var.values():
        b.close()
    if "parent" in libs:
        libs["parent"][0].close()
    return out, text


def oneshot_probe():
    """h2v_verify_batch_keys_hinted from host bytes with right rows against h2v_verify_batch_keys over the same arguments: 1024 proofs,
    and one.  The arguments are marshalled once, outside the timed region: the C calls alone are timed."""
    import ctypes
    from halo2_verifier_amd import verifier
    P = [d["proofs"][i * 1024:(i + 1) * 1024] for i in range(B)]
    I = [[[d["inst"][(i * NPUB + j) * 32:(i * NPUB + j + 1) * 32] for j in range(NPUB)]] for i in range(B)]
    draws = [rand[32 * i:32 * i + 32] for i in range(B)]
    rows1 = [right[i * ROW:(i + 1) * ROW] for i in range(B)]
    lib = hints._library()
    out, text = {}, ["--oneshot: h2v_verify_batch_keys_hinted from host bytes with right rows against h2v_verify_batch_keys, alternating (the C calls alone):"]
    for m in (B, 1):
        a, _, _ = verifier._keyed_args([ctx], [0] * m, P[:m], I[:m], draws[:m])
        rows = hints.call_rows([ctx], [0] * m, rows1[:m])
        res_of = {v: verifier._Results(m) for v in ("plain", "hinted")}
        stats = hints.stats_out()

        def plain():
            r = res_of["plain"]
            h2v._lib.check(lib.h2v_verify_batch_keys(*a, r.st, ctypes.byref(r.ok), r.left, r.right))

        def hinted():
            r = res_of["hinted"]
            h2v._lib.check(lib.h2v_verify_batch_keys_hinted(*a[:6], rows, *a[6:], r.st, ctypes.byref(r.ok), r.left, r.right, stats))
        calls = {"plain": plain, "hinted": hinted}
        plain(); hinted()
        assert res_of["plain"].result() == res_of["hinted"].result() and res_of["plain"].ok.value and tuple(stats) == (m * NP, m * NP, 0)
        for _ in range(10):
            for c in calls.values():
                c()
        t = {v: [] for v in calls}
        for _ in range(args.reps):
            for v, c in calls.items():
                t0 = time.perf_counter()
                c()
                t[v].append((time.perf_counter() - t0) * 1e3)
        out[str(m)] = {v: row(x) for v, x in t.items()}
        text += [f"  {m:5d} proofs  {v:7s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}" for v, r in out[str(m)].items()]
    return out, text


if args.partial:
    res["partial"], more = partial_probe()
    lines += more
if args.oneshot:
    res["oneshot"], more = oneshot_probe()
    lines += more
print("\n".join(lines), flush=True)
for b in batches.values():
    b.close()
ctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")
