"""What every proof's Guard out of a launch (include/h2v_guards.h) costs at the headline launch, 20 groups of 1024 proofs of the k = 14
pool, resident on the device, against the launch alone on this build and on the parent commit's, and against the parent's only route
to a Guard, h2v_guard_msm per proof:
   python tools/guards_out_probe.py --parent PATH [--k 14] [--groups 20] [--reps 7] [--out FILE]
   python tools/guards_out_probe.py --trace [--k 14] [--groups 20]
PATH is a build of libh2v_amd.so made from the parent commit, loaded beside the in-tree one.  One MI355X, one process, at least 50 ms
of warm-up per variant; medians of --reps repetitions with the variants alternating inside each repetition:
   parent   parent build:  launch + finish_groups                                                                          (a)
   host     this build:    launch + finish_groups                                                                          (a)
   device   this build:    (a) + guards_device with all six outputs + one hipStreamSynchronize of the batch's stream       (b)
   append   this build:    (a) + guards_append of every group's range into a pair of fresh MSMKZG objects per group (the
                           objects are made outside the timed region; their first allocation is the call's own)            (c)
   single   parent build:  h2v_guard_msm for each of 64 proofs; the figure reported is SCALED to the launch's proofs        (d)
and, untimed, that the device arrays equal Batch.guards of the same launch.  Prints each variant's median and min .. max, the
parent's spread, (b) - (a) next to the bytes the call writes, and whether `host` is within 1.08 x `parent`.
--trace: no timing; 20 guards_device calls alone on a finished batch, for a run of its own under
   rocprofv3 --kernel-trace --stats -- python tools/guards_out_probe.py --trace
whose k_guards_* rows are the call's per-kernel durations (e)."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import torch
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib, guards

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a build of libh2v_amd.so from the parent commit")
ap.add_argument("--trace", action="store_true", help="guards_device alone on a finished batch, for a kernel trace")
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not args.trace and not args.parent:
    ap.error("--parent PATH, or --trace")

B, N, G = 1024, bench.N_PUBLIC, args.groups
n = B * G
SINGLE = 64
d = bench.load_or_make_proofs(B, args.k, print)
proofs, inst = d["proofs"] * G, d["inst"] * G
rand = b"".join(((i * 0x9e3779b97f4a7c15 + 0x1234567) % (1 << 250)).to_bytes(32, "little") for i in range(1, n + 1))
raw = h2v.SerdeFormat.RawBytes
BOUND = 1.08


def context():
    return h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw))


def outputs(shape):
    sizes = guards.output_sizes(n, shape)
    t = {what: torch.empty(size // 4, dtype=torch.int32, device="cuda:0") if what == "status" else torch.empty(size, dtype=torch.uint8, device="cuda:0")
         for what, size in zip(guards.OUTPUTS, sizes)}
    torch.cuda.synchronize()
    return t, sum(sizes)


mine = _lib.load_library()
ctx = context()


def synchronise(batch):
    """-> a function that is one hipStreamSynchronize of the batch's stream"""
    return torch.cuda.ExternalStream(batch.stream, device="cuda:0").synchronize


if args.trace:
    b = h2v.Batch(ctx, n, N, groups=G)
    b.upload(proofs, 1024, inst, [N], rand)
    b.launch()
    want = b.finish_groups(raw_statuses=True)
    t, _ = outputs(b.guard_shape())
    addr = [t[k].data_ptr() for k in guards.OUTPUTS]
    for _ in range(20):
        guards.guards_device(b, 0, n, *addr)
    synchronise(b)()
    assert t["status"].count_nonzero().item() == 0 and all(want[0])
    b.close(); ctx.close()
    sys.exit(0)

parent = ctypes.CDLL(os.path.abspath(args.parent))   # (a parent build lacks the newer symbols)
for name, (restype, argtypes) in _lib.SIGNATURES.items():
    if hasattr(parent, name):
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = restype, argtypes
assert not hasattr(parent, "h2v_batch_guards_device"), "--parent is not a build of the parent commit"
_lib._LIB = parent
try:
    pctx = context()
    batches = {"parent": h2v.Batch(pctx, n, N, groups=G)}
    batches["parent"].upload(proofs, 1024, inst, [N], rand)
finally:
    _lib._LIB = mine
for v in ("host", "device", "append"):
    batches[v] = h2v.Batch(ctx, n, N, groups=G)
    batches[v].upload(proofs, 1024, inst, [N], rand)
batches["device"].launch(); batches["device"].finish_groups(raw_statuses=True)
shape = batches["device"].guard_shape()
t, written = outputs(shape)
addr = [t[k].data_ptr() for k in guards.OUTPUTS]
dev_sync = synchronise(batches["device"])
one_proof = [d["proofs"][i * 1024:(i + 1) * 1024] for i in range(SINGLE)]
one_inst = [[[d["inst"][(i * N + j) * 32:(i * N + j + 1) * 32] for j in range(N)]] for i in range(SINGLE)]


def host_finish(v):
    def run():
        b = batches[v]
        b.launch()
        return b.finish_groups(raw_statuses=True)
    return run


def device():
    b = batches["device"]
    b.launch()
    b.finish_groups(raw_statuses=True)
    guards.guards_device(b, 0, n, *addr)
    dev_sync()


def fresh_pairs():
    return [h2v.DualMSM(ctx) for _ in range(G)]


def append(pairs):
    b = batches["append"]
    b.launch()
    b.finish_groups(raw_statuses=True)
    for g, p in enumerate(pairs):
        guards.guards_append(b, p.left, p.right, g * B, B)


def single():
    for p, i in zip(one_proof, one_inst):
        rc, _ = pctx.guard_msm(p, i)
        assert rc == 0


want = host_finish("host")()
assert all(want[0]) and want[1].count(0) == len(want[1])
assert host_finish("parent")() == want
device()
rows = batches["device"].guards(B - 2, 4)               # across the first group boundary
tl, tr = shape
for what, T, size in (("left_scalars", tl, 32), ("left_bases", tl, 64), ("right_scalars", tr, 32), ("right_bases", tr, 64)):
    got = bytes(t[what][(B - 2) * T * size:(B + 2) * T * size].cpu().numpy().tobytes())
    assert got == b"".join(x for r in rows for x in r[what]), what
assert t["status"].count_nonzero().item() == 0
pairs = fresh_pairs()
append(pairs)
assert len(pairs[0].left) == B * tl and len(pairs[G - 1].right) == B * tr
ok, lefts, rights = h2v.dual_check_many(pairs)
assert (ok, lefts, rights) == (want[0], want[2], want[3])
for p in pairs:
    p.close()
_lib._LIB = parent
try:
    single()
finally:
    _lib._LIB = mine

timed = {"parent": host_finish("parent"), "host": host_finish("host"), "device": device}
t0 = time.perf_counter()
while time.perf_counter() - t0 < bench.WARM_S * 4:   # (each variant for at least 50 ms)
    for fn in timed.values():
        fn()
    pairs = fresh_pairs(); append(pairs)
    for p in pairs:
        p.close()
ts = {v: [] for v in list(timed) + ["append", "single"]}
for _ in range(args.reps):
    for v, fn in timed.items():
        t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
    pairs = fresh_pairs()
    t0 = time.perf_counter(); append(pairs); ts["append"].append((time.perf_counter() - t0) * 1e3)
    for p in pairs:
        p.close()
    _lib._LIB = parent
    try:
        t0 = time.perf_counter(); single(); ts["single"].append((time.perf_counter() - t0) * 1e3 * n / SINGLE)
    finally:
        _lib._LIB = mine

res = {"n": n, "groups": G, "k": args.k, "reps": args.reps, "parent": args.parent, "bound": BOUND, "shape": list(shape), "bytes_written": written,
       "single_proofs_timed": SINGLE, "rows": {}}
for v, tv in ts.items():
    res["rows"][v] = {"median_ms": round(sorted(tv)[len(tv) // 2], 3), "min_ms": round(min(tv), 3), "max_ms": round(max(tv), 3)}
    r = res["rows"][v]
    note = f"  (SCALED from {SINGLE} proofs to {n})" if v == "single" else ""
    print(f"{v:7s} {r['median_ms']:10.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]{note}", flush=True)
base = res["rows"]["parent"]["median_ms"]
res["parent_spread_ms"] = round(res["rows"]["parent"]["max_ms"] - res["rows"]["parent"]["min_ms"], 3)
res["host_over_parent"] = round(res["rows"]["host"]["median_ms"] / base, 4)
res["host_within_bound"] = res["rows"]["host"]["median_ms"] <= BOUND * base
res["device_minus_host_ms"] = round(res["rows"]["device"]["median_ms"] - res["rows"]["host"]["median_ms"], 3)
res["append_minus_host_ms"] = round(res["rows"]["append"]["median_ms"] - res["rows"]["host"]["median_ms"], 3)
gbps = written / max(res["device_minus_host_ms"], 1e-6) / 1e6   # (meaningless where the difference is below the spread: see --trace)
res["device_minus_host_resolved"] = res["device_minus_host_ms"] > res["parent_spread_ms"]
print(f"host / parent: {res['host_over_parent']:.4f} (bound {BOUND}, within: {res['host_within_bound']}); the parent's spread over its {args.reps} timings: "
      f"{res['parent_spread_ms']:.3f} ms")
print(f"(b) - (a) = {res['device_minus_host_ms']:.3f} ms for {written} bytes written ({n} proofs x ({tl} + {tr}) terms x 96 B + 36 B per proof): "
      + (f"{gbps:.0f} GB/s" if res["device_minus_host_resolved"] else "below the parent's spread, NOT RESOLVED (the kernels' own times: --trace)") + "; "
      f"(c) - (a) = {res['append_minus_host_ms']:.3f} ms for {G} calls", flush=True)
for b in batches.values():
    b.close()
ctx.close(); pctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(f"{v:7s} median {r['median_ms']:10.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}" for v, r in res["rows"].items()) + "\n"
                + json.dumps(res, indent=1) + "\n")
