"""Measurement: the k-NN search and the k-NN normals (pfx_knn.hip) from the context's HIP-event timers
and the wall clock, in one process.  Inputs: synth_room and synth_seabed at 100,000 and 1,000,000
points (PFX_KNN_SIZES overrides the sizes), k = 10, 30, 100, the surface as the queries.  One warm-up
call, then PFX_KNN_REPEATS (default 5) calls of each device form; the median wall clock (host waits
included: the search reads a counter back per grid) and the median per stage are reported with the
path statistics.  Beside them: the CPU restatement (tests/cpp/knn_ref.cpp, OpenMP) on the same host on
256 sampled queries against the whole surface, as microseconds per query, and whether the GPU rows of
those queries equal it; and, once per cloud, pfx_normals at r = 0.05 against normals_knn at the k
nearest that cloud's mean radius-neighbour count (capped at KNN_MAX_K).  One JSON line per
measurement.  Needs a GPU."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import knn_ref as R  # noqa: E402
from pcl_feature_extraction_amd import Context  # noqa: E402
from pcl_feature_extraction_amd._native import KNN_MAX_K  # noqa: E402
from pcl_feature_extraction_amd.synth import synth_room, synth_seabed  # noqa: E402

REPEATS = int(os.environ.get("PFX_KNN_REPEATS", "5"))
SIZES = [int(v) for v in os.environ.get("PFX_KNN_SIZES", "100000,1000000").split(",")]
STAGES = ("knn", "grid_build", "knn_order", "knn_search", "knn_exhaustive", "knn_normals")
STATS = ("knn_queries", "knn_rounds", "knn_first", "knn_requeued", "knn_exhaustive", "knn_skipped")


def timed(ctx, call):
    """Median wall clock and per-stage device time of REPEATS calls after one warm-up."""
    call()
    ctx.synchronize()
    wall = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    ctx.set_timing(True)
    ms = {s: [] for s in STAGES}
    for _ in range(REPEATS):
        ctx.reset_timing()
        call()
        ctx.synchronize()
        for s in STAGES:
            ms[s].append(ctx.kernel_time(s)[0])
    ctx.set_timing(False)
    out = {"wall_ms": round(float(np.median(wall)), 3)}
    out.update({s + "_ms": round(float(np.median(v)), 4) for s, v in ms.items()})
    return out


def measure(ctx, ref, name, cloud, k):
    x, y, z = cloud
    n = len(x)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in cloud]
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    idx = torch.empty((n, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
    out4 = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    base = {"input": name, "points": n, "k": k, "repeats": REPEATS}
    s = dict(base, call="knn_search", **timed(ctx, lambda: ctx.knn_search_dev(*d, *d, k, counts, idx, d2)))
    s.update({st: ctx.stat(st) for st in STATS})
    q = np.random.default_rng(1).choice(n, 256, replace=False)
    t0 = time.perf_counter()
    want = R.search(ref, x, y, z, x[q], y[q], z[q], k)
    s["restatement_cpu_us_per_query"] = round((time.perf_counter() - t0) * 1e6 / len(q), 1)
    s["restatement_threads"] = os.cpu_count()
    s["gpu_us_per_query"] = round(s["wall_ms"] * 1e3 / n, 4)
    qi = torch.from_numpy(q).to(dev)
    s["equals_restatement"] = bool(np.array_equal(idx[qi].cpu().numpy(), want[1]) and
                                   np.array_equal(d2[qi].cpu().numpy().view(np.uint32), want[2].view(np.uint32)))
    print(json.dumps(s), flush=True)
    m = dict(base, call="normals_knn", **timed(ctx, lambda: ctx.normals_knn_dev(*d, k, *out4)))
    m.update({st: ctx.stat(st) for st in STATS})
    print(json.dumps(m), flush=True)


def radius_against_knn(ctx, name, cloud, r=0.05):
    n = len(cloud[0])
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in cloud]
    out4 = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    rad = timed(ctx, lambda: ctx.normals_dev(*d, r, *out4))
    mean = ctx.stat("normals_neighbors") / n
    k = int(min(KNN_MAX_K, max(3, round(mean))))
    knn = timed(ctx, lambda: ctx.normals_knn_dev(*d, k, *out4))
    print(json.dumps({"input": name, "points": n, "call": "normals r=0.05 against normals_knn", "radius": r,
                      "mean_radius_neighbors": round(mean, 1), "k": k, "normals_wall_ms": rad["wall_ms"],
                      "normals_knn_wall_ms": knn["wall_ms"],
                      "normals_knn_stages": {s: v for s, v in knn.items() if s != "wall_ms"}}), flush=True)


def main():
    if not torch.cuda.is_available():
        sys.exit("knn_time: no GPU")
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        ref = R.build(tmp)
        for n in SIZES:
            for name, gen, seed in (("synth_room", synth_room, 1), ("synth_seabed", synth_seabed, 3)):
                cloud = gen(n, seed)[:3]
                label = f"{name}({n}, {seed})"
                for k in (10, 30, 100):
                    measure(ctx, ref, label, cloud, k)
                radius_against_knn(ctx, label, cloud)
                ctx.trim()


if __name__ == "__main__":
    main()
