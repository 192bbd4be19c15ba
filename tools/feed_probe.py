#!/usr/bin/env python3
"""What an enqueued feed of a resident accumulator costs (include/h2v_feed.h), on one MI355X, one process:

   python tools/feed_probe.py --parent <the parent commit's libh2v_amd.so> [--parent-tree <a checkout of the parent, built>] [--out F]

k = 14 (the benchmark's 1024 proofs, cycled), 20 x 1024 resident proofs per launch, no pairing in the launch.  At least 50 ms of
warm-up, medians of 7 repetitions with their range, the variants alternating inside every repetition; the parent commit's library
is loaded beside the in-tree one.  Wall times, ms:
   a. the parent's   launch + finish_groups + process_batch
   b. this tree's    launch + finish_groups + process_batch          gate: b / a <= 1.08 (what DESIGN.md holds additive changes to)
   c. this tree's    launch + feed on two alternating batches, 8 rounds, ONE settle at the end; reported per round, against a with
                     a's own spread beside it
   d. with --parent-tree: `python bench.py --gpus 1 --steps 20 --warmup 5` three times in each tree, alternating; gate: the medians
      within 1.08.
With --trace: a process of 8 proofs, then one feed + settle at G = 20 and at G = 512, for a `rocprofv3 --kernel-trace --stats` run of
its own."""
import argparse
import ctypes
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
bench.hw_queue_env()
from halo2_verifier_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--out", default=None)
ap.add_argument("--parent", default=None)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
import halo2_verifier_amd as h2v

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
RAW = h2v.SerdeFormat.RawBytes
LEGS, GATE = 20, 1.08

n, N = 1024, bench.N_PUBLIC
d = bench.load_or_make_proofs(n, args.k, print)
ctx = h2v.Context(h2v.ParamsKZG(d["params"], RAW), h2v.VerifyingKey(d["vk"], RAW))
P = [d["proofs"][1024 * i:1024 * (i + 1)] for i in range(n)]
I = [[[d["inst"][32 * (N * i + j):32 * (N * i + j + 1)] for j in range(N)]] for i in range(n)]
rnd = random.Random(2026)
flat_p, flat_i = d["proofs"][:1024 * n], d["inst"][:32 * N * n]


def median(ts):
    return sorted(ts)[len(ts) // 2]


def parent_context(path):
    """a Context on another build of the library, loaded beside the in-tree one"""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    mine = _lib.load_library()
    _lib._LIB = lib
    try:
        return h2v.Context(h2v.ParamsKZG(d["params"], RAW), h2v.VerifyingKey(d["vk"], RAW))
    finally:
        _lib._LIB = mine


def staged(c, groups, per_group):
    """a resident batch of groups x per_group proofs (the pool, cycled), uploaded once, launched and finished once"""
    total = groups * per_group
    reps_, rest = divmod(total, n)
    b = h2v.Batch(c, total, N, groups=groups)
    tail = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(total))
    b.upload(flat_p * reps_ + flat_p[:1024 * rest], 1024, flat_i * reps_ + flat_i[:32 * N * rest], [N], tail)
    b.launch(with_pairing=False)
    ok, st, _, _ = b.finish_groups(raw_statuses=True)
    assert all(ok) and not any(st)
    return b


def lead(c):
    acc = h2v.Accumulator(c)
    acc.process(c, None, P[:8], I[:8], [rnd.randrange(1, R_MOD) for _ in range(8)])   # (a non-empty accumulator: the scale step has points to scale)
    return acc


if args.trace:
    for G, per in ((LEGS, n), (512, 2)):
        b, acc = staged(ctx, G, per), lead(ctx)
        b.launch(with_pairing=False)
        acc.feed(b)
        assert acc.settle() == [(0, b.n, 0)] and acc.finalize()[0]
        acc.close(); b.close()
    ctx.close()
    sys.exit(0)

res = {"k": args.k, "reps": args.reps, "rounds": args.rounds, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}
pctx = parent_context(args.parent) if args.parent else None

big = [staged(ctx, LEGS, n), staged(ctx, LEGS, n)]
acc_b, acc_c = lead(ctx), lead(ctx)


def three_calls(b, acc):
    b.launch(with_pairing=False)
    b.finish_groups(raw_statuses=True)
    return acc.process_batch(b)


def fed_rounds():
    for r in range(args.rounds):
        b = big[r % 2]
        b.launch(with_pairing=False)
        acc_c.feed(b)
    reports = acc_c.settle()
    assert reports == [(0, LEGS * n, 0)] * args.rounds, reports


variants = {}
if pctx:
    pbig, pacc = staged(pctx, LEGS, n), lead(pctx)
    variants["a_parent_launch_finish_process_batch"] = lambda: three_calls(pbig, pacc)
variants["b_launch_finish_process_batch"] = lambda: three_calls(big[0], acc_b)
variants["c_launch_feed_x%d_settle" % args.rounds] = fed_rounds

t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.05:   # warm-up
    for fn in variants.values():
        fn()
ts = {v: [] for v in variants}
for _ in range(args.reps):
    for v, fn in variants.items():
        t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
c_name = [v for v in variants if v.startswith("c_")][0]
ts[c_name + "_per_round"] = [t / args.rounds for t in ts[c_name]]
row = {v: round(median(t), 3) for v, t in ts.items()}
row.update({v + "_min_max": [round(min(t), 3), round(max(t), 3)] for v, t in ts.items()})
for v in ts:
    lo, hi = row[v + "_min_max"]
    print(f"{v:44s} {row[v]:8.3f} ms   ({lo:.3f} - {hi:.3f})", flush=True)
assert acc_b.finalize()[0] and acc_c.finalize()[0]
if pctx:
    a, b_, c = row["a_parent_launch_finish_process_batch"], row["b_launch_finish_process_batch"], row[c_name + "_per_round"]
    lo, hi = row["a_parent_launch_finish_process_batch_min_max"]
    row["b_over_a"] = round(b_ / a, 4)
    row["c_per_round_over_a"] = round(c / a, 4)
    row["c_below_a_by_more_than_a_spread"] = bool(a - c > hi - lo)
    print(f"b / a = {row['b_over_a']:.3f} ({'within' if row['b_over_a'] <= GATE else 'OUTSIDE'} {GATE}x)", flush=True)
    print(f"c per round / a = {row['c_per_round_over_a']:.3f}; a's spread {hi - lo:.3f} ms; c is "
          f"{'below a by more than that spread' if row['c_below_a_by_more_than_a_spread'] else 'NOT below a by more than that spread'}", flush=True)
    pacc.close(); pbig.close()
res["feed_ms"] = row
acc_b.close(); acc_c.close()
for b in big:
    b.close()
ctx.close()

def dump():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


dump()
if args.parent_tree:
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = {"this": [], "parent": []}
    for _ in range(3):
        for name, cwd in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            runs[name].append(json.loads(line)["value"])
    res["headline_proofs_per_s"] = runs
    ratio = median(runs["parent"]) / median(runs["this"])
    res["headline_parent_over_this"] = round(ratio, 4)
    print(f"headline, proofs/s: this {runs['this']}   parent {runs['parent']}   parent / this = {ratio:.3f} "
          f"({'within' if ratio <= GATE else 'OUTSIDE'} {GATE}x)", flush=True)

print(json.dumps(res))
dump()
