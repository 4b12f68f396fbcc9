"""Measurement: ICP (pfx_icp_dev) on the reference's indoor pair with the reference's parameters
(0.07, 100 iterations, 1e-6, 1e-4), the two calls of the evaluation loop:
  direct    : the two full clouds (evaluation.cpp:246-253)
  keypoints : their ISS keypoints (salient 6 x, non-max 4 x the cloud resolution; :289-293)
One warm-up call, then PFX_ICP_REPEATS (default 5) calls: the median wall time per call (the call is
synchronous: one host synchronisation per iteration), time per iteration, and the split by stage
from the context's timers (HIP events around each stage's launches: search, compaction, means,
sigma, the exact sum, the fitness score; "host" is the wall time the events do not cover: launch
gaps, the readback, the 3x3 SVD).  The single-threaded CPU restatement (tests/cpp/icp_ref.cpp) is
timed once on the same inputs with its own stage clocks.  One JSON line per input.  Needs a GPU."""
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

import icp_ref as R  # noqa: E402
from pcl_feature_extraction_amd import Context, icp_params  # noqa: E402

REPEATS = int(os.environ.get("PFX_ICP_REPEATS", "5"))
STAGES = ("icp_nn", "icp_compact", "icp_means", "icp_sigma", "icp_mse", "icp_fitness")


def clouds(ctx):
    import shot_color_ref as S
    full = [S.read_cloud("indoor_" + w)[:3] for w in ("source", "target")]
    kp = []
    for x, y, z in full:
        res = ctx.cloud_resolution(x, y, z)
        k = ctx.iss_keypoints(x, y, z, 6 * res, 4 * res)
        kp.append(tuple(np.ascontiguousarray(v[k]) for v in (x, y, z)))
    return {"direct": full, "keypoints": kp}


def measure(ctx, name, src, tgt, lib):
    dev = torch.device("cuda", 0)
    ds = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for v in src]
    dt = [torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev) for v in tgt]
    prm = icp_params(**R.REFERENCE)
    got = ctx.icp_dev(*ds, *dt, prm)  # warm-up: code objects, scratch buffers
    wall, stage = [], {k: [] for k in STAGES}
    ctx.set_timing(True)
    for _ in range(REPEATS):
        ctx.reset_timing()
        ctx.synchronize()
        t0 = time.perf_counter()
        got = ctx.icp_dev(*ds, *dt, prm)
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in STAGES:
            stage[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    it = max(got.iterations, 1)
    out = {"input": name, "source_points": len(src[0]), "target_points": len(tgt[0]), "iterations": got.iterations,
           "state": got.state, "correspondences_last": ctx.stat("icp_correspondences"),
           "nn_rounds": ctx.stat("icp_nn_rounds"), "brute": ctx.stat("icp_brute"),
           "exact_sum": ctx.stat("icp_exact_sum"), "repeats": REPEATS}
    med = float(np.median(wall))
    out["total_ms"] = round(med, 3)
    out["total_ms_min_max"] = [round(min(wall), 3), round(max(wall), 3)]
    out["ms_per_iteration"] = round(med / it, 4)
    covered = 0.0
    for k in STAGES:
        m = float(np.median(stage[k]))
        covered += m
        out[k[4:] + "_ms"] = round(m, 3)
    out["host_ms"] = round(med - covered, 3)
    t0 = time.perf_counter()
    want = R.icp(lib, src, tgt, R.REFERENCE)
    sec = time.perf_counter() - t0
    out["restatement_1thread_s"] = round(sec, 3)
    out["restatement_ms_per_iteration"] = round(sec * 1e3 / max(want.iterations, 1), 3)
    out["restatement_stage_s"] = {k: round(v, 3) for k, v in R.stage_seconds(lib).items()}
    out["equal_to_restatement"] = bool(
        np.array_equal(got.transformation.view(np.uint32), want.transformation.view(np.uint32)) and
        got.fitness == want.fitness and (got.iterations, got.state) == (want.iterations, want.state))
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("icp_time: no GPU")
    lib = R.build(tempfile.mkdtemp(prefix="icp_ref"))
    with Context(0) as ctx:
        for name, (src, tgt) in clouds(ctx).items():
            print(json.dumps(measure(ctx, name, src, tgt, lib)), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
