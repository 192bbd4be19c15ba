#!/usr/bin/env python3
"""Which hardware queue every stream of a run landed on, and what a launch waits for: from a rocprofv3 --kernel-trace CSV,
   python tools/queue_gaps.py <k_kernel_trace.csv> [label]
For every stream: its queue and kernel count.  For every kernel name: the gap in front of it inside its own stream (start - end of the
stream's previous kernel), and for the gaps above 20 us the kernel of ANOTHER stream that filled most of the gap on the SAME queue —
a stream's kernels are in order, and so are the kernels of all streams that share a hardware queue.  Last: how long each queue
was busy and how long two queues were busy at once (the overlap the pipeline lives on).  Only the last 60 % of the trace is
read (the timed region and its neighbourhood; uploads and warm-up are left out)."""
import collections
import csv
import statistics
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if r["Kind"] == "KERNEL_DISPATCH"]
label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
K = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Stream_Id"], r["Kernel_Name"].split("(")[0].replace("void ", "").replace("h2v::", "")) for r in rows]
K.sort()
K = K[int(len(K) * 0.4):]
print(f"== {label}: {len(K)} dispatches, {(K[-1][1] - K[0][0]) / 1e6:.2f} ms")
by_stream = collections.defaultdict(list)
for k in K:
    by_stream[k[3]].append(k)
print("stream -> queue (kernels):", "  ".join(f"s{s}->q{v[0][2]} ({len(v)})" for s, v in sorted(by_stream.items(), key=lambda x: int(x[0]))))
by_queue = collections.defaultdict(list)
for k in K:
    by_queue[k[2]].append(k)
gaps = collections.defaultdict(list)
blockers = collections.defaultdict(collections.Counter)
for s, v in by_stream.items():
    for prev, cur in zip(v, v[1:]):
        g = cur[0] - prev[1]
        if prev[4].startswith("k_pairing") or prev[4] in ("k_copy_words", "k_point_to_bytes"):
            continue   # the first kernel of the stream's next launch: the host decides when it comes
        gaps[cur[4]].append(g / 1e3)
        if g > 20000:
            best, best_t = "(nothing on this queue)", 0
            for o in by_queue[cur[2]]:
                if o[3] == s:
                    continue
                t = min(o[1], cur[0]) - max(o[0], prev[1])
                if t > best_t:
                    best, best_t = o[4], t
            blockers[cur[4]][best] += 1
print(f"{'kernel':28s} {'n':>5s} {'median gap':>11s} {'p90':>9s} {'max':>9s}   gaps > 20 us were behind (same queue, other stream)")
for name, g in sorted(gaps.items(), key=lambda x: -sum(x[1])):
    g.sort()
    print(f"{name[:28]:28s} {len(g):5d} {statistics.median(g):9.1f} us {g[int(0.9 * (len(g) - 1))]:7.1f} us {g[-1]:7.1f} us   " +
          ", ".join(f"{b} x{c}" for b, c in blockers[name].most_common(3)))
t0, t1 = K[0][0], K[-1][1]
ev = []
for q, v in by_queue.items():
    cur_s, cur_e, busy = None, None, 0
    for s, e, *_ in v:   # union of the queue's kernel intervals
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                ev.append((cur_s, 1)); ev.append((cur_e, -1)); busy += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    ev.append((cur_s, 1)); ev.append((cur_e, -1)); busy += cur_e - cur_s
    print(f"queue {q}: a kernel running {100 * busy / (t1 - t0):.0f} % of the time")
ev.sort()
depth, last, both = 0, t0, 0
for t, d in ev:
    if depth >= 2:
        both += t - last
    depth += d
    last = t
print(f"two queues busy at once: {100 * both / (t1 - t0):.0f} % of the time")
