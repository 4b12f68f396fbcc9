"""Measurement: uniform-sampling keypoints (pfx_uniform.hip) from the context's HIP-event timers, in
one process.  Inputs: synth_room at 100,000 and 1,000,000 points, leaf 0.05 and 0.01.  One warm-up
call, then PFX_UNIFORM_REPEATS (default 5) calls of the device form; the median per stage is reported,
with the host form's wall clock (median of the same number of calls, staging included) and, beside
them, the CPU restatement (tests/cpp/uniform_ref.cpp) on the same host, one thread.  One JSON line per
input.  Needs a GPU."""
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

import uniform_ref as R  # noqa: E402
from pcl_feature_extraction_amd import Context  # noqa: E402
from pcl_feature_extraction_amd.synth import synth_room  # noqa: E402

REPEATS = int(os.environ.get("PFX_UNIFORM_REPEATS", "5"))
STAGES = ("uniform", "uniform_bbox", "uniform_keys", "uniform_sort", "uniform_heads", "uniform_compact",
          "uniform_gather")


def measure(ctx, ref, n, leaf):
    x, y, z, _ = synth_room(n, 1)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(v).to(dev) for v in (x, y, z)]
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    lf = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    k = ctx.uniform_sampling_dev(*d, leaf, idx, lf)  # warm-up: code objects, scratch buffers
    ctx.synchronize()
    ctx.set_timing(True)
    ms = {s: [] for s in STAGES}
    for _ in range(REPEATS):
        ctx.reset_timing()
        ctx.uniform_sampling_dev(*d, leaf, idx, lf)
        ctx.synchronize()
        for s in STAGES:
            ms[s].append(ctx.kernel_time(s)[0])
    ctx.set_timing(False)
    ctx.uniform_sampling(x, y, z, leaf)
    wall = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ctx.uniform_sampling(x, y, z, leaf, return_leaf=True)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    want = R.sample(ref, x, y, z, leaf)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    got = idx[:k].cpu().numpy()
    out = {"input": f"synth_room({n}, 1)", "leaf": leaf, "repeats": REPEATS, "keypoints": k,
           "points": ctx.stat("uniform_points"), "cells": ctx.stat("uniform_cells"),
           "equals_restatement": bool(np.array_equal(got, want.idx))}
    for s in STAGES:
        out[s + "_ms"] = round(float(np.median(ms[s])), 4)
    out["sort_share"] = round(out["uniform_sort_ms"] / out["uniform_ms"], 3)
    out["host_form_wall_ms"] = round(float(np.median(wall)), 3)
    out["restatement_cpu_ms"] = round(cpu_ms, 2)
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("uniform_time: no GPU")
    with tempfile.TemporaryDirectory() as tmp, Context(0) as ctx:
        ref = R.build(tmp)
        for n in (100_000, 1_000_000):
            for leaf in (0.05, 0.01):
                print(json.dumps(measure(ctx, ref, n, leaf)), flush=True)


if __name__ == "__main__":
    main()
