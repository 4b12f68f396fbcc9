"""The list set-up's chain in one timed bench step, from a rocprofv3 kernel-trace CSV: every launch
(any duration, every queue) from the step's start to the start of the first k_nb_tile, and every
launch from the end of the last list kernel to the start of k_normals_chain; then, over all timed
steps of the trace, the marks (tile0: start of the first k_nb_tile; chain: the same, counted from
the start of the estimation stream's first kernel of the step) and the in-step duration of each
kernel of the two windows on that stream.

usage: setup_timeline.py run_kernel_trace.csv [step index from the end, default 5]"""
import collections
import csv
import sys


def short(name):
    return name.replace("pfx::(anonymous namespace)::", "").replace("void ", "").split("(")[0][:64]


rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
for r in rows:
    r.setdefault("Queue_Id", "?")
    r["s"], r["e"], r["k"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])
ends = [i for i, r in enumerate(rows) if "k_fpfh_weight<true" in r["Kernel_Name"]]
back = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def step_parts(t0, t1):
    """(rows before the first tile kernel, rows between the last list kernel and the chain, marks)"""
    step = [r for r in rows if r["s"] >= t0 and r["e"] <= t1]
    tiles = [r for r in step if r["k"].startswith("k_nb_tile")]
    chain = [r for r in step if r["k"].startswith("k_normals_chain<") or r["k"] == "k_normals_chain"]
    if not tiles or not chain:
        return None
    q = tiles[0]["Queue_Id"]
    lists = [r for r in step if r["Queue_Id"] == q and r["k"].startswith(("k_nb_tile", "k_nb_wide", "k_nb_query"))
             and r["s"] < chain[0]["s"]]
    last_end = max(r["e"] for r in lists)
    head = [r for r in step if r["s"] < tiles[0]["s"]]
    gap = [r for r in step if r["Queue_Id"] == q and r["s"] >= last_end and r["s"] < chain[0]["s"]]
    first = min(r["s"] for r in head if r["Queue_Id"] == q)  # (the host's launch of the stream's first kernel varies)
    return head, gap, dict(queue=q, tile0=tiles[0]["s"] - t0, chain=tiles[0]["s"] - first, lists_end=last_end - t0, chain0=chain[0]["s"] - t0,
                           step=t1 - t0)


def show(part, t0, q):
    for r in part:
        print("q%-3s%s %9.1f %8.1f  %s" % (r["Queue_Id"], "*" if r["Queue_Id"] == q else " ", (r["s"] - t0) / 1e3,
                                          (r["e"] - r["s"]) / 1e3, r["k"]))


t0, t1 = rows[ends[-back - 1]]["e"], rows[ends[-back]]["e"]
head, gap, m = step_parts(t0, t1)
print("step %.1f us; normal-estimation queue q%s (*); columns: queue, start us, duration us, kernel" %
      (m["step"] / 1e3, m["queue"]))
print("-- step start to the first k_nb_tile (starts at %.1f us)" % (m["tile0"] / 1e3))
show(head, t0, m["queue"])
print("-- end of the last list kernel (%.1f us) to k_normals_chain (starts at %.1f us)" %
      (m["lists_end"] / 1e3, m["chain0"] / 1e3))
show(gap, t0, m["queue"])

# the same two windows over the other steps (the first two warm up, the last three run with per-kernel
# timers: left out)
dur = collections.defaultdict(list)
marks = collections.defaultdict(list)
for a, b in zip(ends[2:-4], ends[3:-3]):
    parts = step_parts(rows[a]["e"], rows[b]["e"])
    if not parts:
        continue
    h, g, mm = parts
    per = collections.defaultdict(int)
    for r in h + g:
        if r["Queue_Id"] == mm["queue"]:
            per[r["k"]] += r["e"] - r["s"]
    for k, v in per.items():
        dur[k].append(v)
    for k in ("tile0", "chain", "lists_end", "chain0", "step"):
        marks[k].append(mm[k])
print("-- over %d steps: mean (min-max) us, marks with their median" % len(marks["step"]))
for k in ("step", "tile0", "chain", "lists_end", "chain0"):
    v = sorted(marks[k])
    print("%-40s %8.1f (%.1f-%.1f) median %.1f" % (k, sum(v) / len(v) / 1e3, v[0] / 1e3, v[-1] / 1e3, v[len(v) // 2] / 1e3))
print("%-40s %8.1f" % ("chain0 - lists_end", (sum(marks["chain0"]) - sum(marks["lists_end"])) / len(marks["step"]) / 1e3))
for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
    print("%-64s %8.1f (%.1f-%.1f) x%d" % (k, sum(v) / len(v) / 1e3, min(v) / 1e3, max(v) / 1e3, len(v)))
