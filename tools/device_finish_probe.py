"""What a finish into device memory (h2v_batch_finish_device) costs at the headline launch, 20 groups of 1024 proofs of the k = 14 pool,
resident on the device, against the host finish of this build and of the parent commit's:
   python tools/device_finish_probe.py --parent PATH [--k 14] [--groups 20] [--reps 7] [--out FILE]
   python tools/device_finish_probe.py --trace [--k 14] [--groups 20]
PATH is a build of libh2v_amd.so made from the parent commit, loaded beside the in-tree one.  One MI355X, one process, at least 50 ms
of warm-up per variant; medians of --reps repetitions with the variants alternating inside each repetition:
   parent   parent build:  launch + finish_groups
   host     this build:    launch + finish_groups
   device   this build:    launch + finish_device with all seven outputs + one hipStreamSynchronize of the batch's stream
and, untimed, that the device arrays equal finish_groups of the same launch.  Prints each variant's median and min .. max, the
parent's spread, and whether `host` and `device` are within 1.08 x `parent`.
--trace: no timing; 20 finish_device calls alone on a finished batch, for a run of its own under
   rocprofv3 --kernel-trace --stats -- python tools/device_finish_probe.py --trace
whose k_results_* rows are the call's per-kernel durations."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import torch
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a build of libh2v_amd.so from the parent commit")
ap.add_argument("--trace", action="store_true", help="finish_device alone on a finished batch, for a kernel trace")
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not args.trace and not args.parent:
    ap.error("--parent PATH, or --trace")

B, N, G = 1024, bench.N_PUBLIC, args.groups
n = B * G
d = bench.load_or_make_proofs(B, args.k, print)
proofs, inst = d["proofs"] * G, d["inst"] * G
rand = b"".join(((i * 0x9e3779b97f4a7c15 + 0x1234567) % (1 << 250)).to_bytes(32, "little") for i in range(1, n + 1))
raw = h2v.SerdeFormat.RawBytes
BOUND = 1.08


def context():
    return h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw))


def outputs():
    dev = "cuda:0"
    t = {"status": torch.empty(n, dtype=torch.int32, device=dev), "group_ok": torch.empty(G, dtype=torch.int32, device=dev),
         "left_xy": torch.empty((G, 64), dtype=torch.uint8, device=dev), "right_xy": torch.empty((G, 64), dtype=torch.uint8, device=dev),
         "group_failed": torch.empty(G, dtype=torch.int32, device=dev), "failed_index": torch.empty(n, dtype=torch.int32, device=dev),
         "summary": torch.empty(8, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    return t


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
    t = outputs()
    addr = [t[k].data_ptr() for k in ("status", "group_ok", "left_xy", "right_xy", "group_failed", "failed_index")]
    for _ in range(20):
        b.finish_device(*addr, n, t["summary"].data_ptr())
    synchronise(b)()
    assert t["summary"].tolist()[1:5] == [0, G, n, G] and all(want[0])
    b.close(); ctx.close()
    sys.exit(0)

parent = ctypes.CDLL(os.path.abspath(args.parent))   # (a parent build lacks the newer symbols)
for name, (restype, argtypes) in _lib.SIGNATURES.items():
    if hasattr(parent, name):
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = restype, argtypes
assert not hasattr(parent, "h2v_batch_finish_device"), "--parent is not a build of the parent commit"
_lib._LIB = parent
try:
    pctx = context()
    batches = {"parent": h2v.Batch(pctx, n, N, groups=G)}
    batches["parent"].upload(proofs, 1024, inst, [N], rand)
finally:
    _lib._LIB = mine
for v in ("host", "device"):
    batches[v] = h2v.Batch(ctx, n, N, groups=G)
    batches[v].upload(proofs, 1024, inst, [N], rand)
t = outputs()
addr = [t[k].data_ptr() for k in ("status", "group_ok", "left_xy", "right_xy", "group_failed", "failed_index")]
summary_addr = t["summary"].data_ptr()
dev_sync = synchronise(batches["device"])


def host_finish(v):
    def run():
        b = batches[v]
        b.launch()
        return b.finish_groups(raw_statuses=True)
    return run


def device():
    b = batches["device"]
    b.launch()
    b.finish_device(*addr, n, summary_addr)
    dev_sync()


variants = {"parent": host_finish("parent"), "host": host_finish("host"), "device": device}
want = variants["host"]()
assert all(want[0]) and want[1].count(0) == len(want[1])
assert variants["parent"]() == want
device()
assert t["group_ok"].tolist() == [1] * G and bytes(t["status"].cpu().numpy().tobytes()) == want[1]
assert [bytes(r) for r in t["left_xy"].cpu().numpy()] == want[2] and [bytes(r) for r in t["right_xy"].cpu().numpy()] == want[3]
assert t["summary"].tolist() == [-1, 0, G, n, G, 1, 0, 0] and t["group_failed"].tolist() == [0] * G
t0 = time.perf_counter()
while time.perf_counter() - t0 < bench.WARM_S * 3:   # (each variant for at least 50 ms)
    for fn in variants.values():
        fn()
ts = {v: [] for v in variants}
for _ in range(args.reps):
    for v, fn in variants.items():
        t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)

res = {"n": n, "groups": G, "k": args.k, "reps": args.reps, "parent": args.parent, "bound": BOUND, "rows": {}}
for v, tv in ts.items():
    res["rows"][v] = {"median_ms": round(sorted(tv)[len(tv) // 2], 3), "min_ms": round(min(tv), 3), "max_ms": round(max(tv), 3),
                      "mproofs_per_s": round(n / sorted(tv)[len(tv) // 2] / 1e3, 2)}
    r = res["rows"][v]
    print(f"{v:7s} {r['median_ms']:7.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  {r['mproofs_per_s']:6.2f} M proofs/s", flush=True)
base = res["rows"]["parent"]["median_ms"]
res["parent_spread_ms"] = round(res["rows"]["parent"]["max_ms"] - res["rows"]["parent"]["min_ms"], 3)
for v in ("host", "device"):
    res[v + "_over_parent"] = round(res["rows"][v]["median_ms"] / base, 4)
    res[v + "_within_bound"] = res["rows"][v]["median_ms"] <= BOUND * base
print(f"host / parent: {res['host_over_parent']:.4f}; device / parent: {res['device_over_parent']:.4f}; bound {BOUND}; "
      f"the parent's spread over its {args.reps} timings: {res['parent_spread_ms']:.3f} ms")
print("host and device within the bound:", res["host_within_bound"], res["device_within_bound"], flush=True)
for b in batches.values():
    b.close()
ctx.close(); pctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(f"{v:7s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}  {r['mproofs_per_s']:6.2f} M proofs/s"
                          for v, r in res["rows"].items()) + "\n" + json.dumps(res, indent=1) + "\n")
