"""Measurement: SHOT-1344 (pfx_shot_color_dev) against SHOT-352 (pfx_shot_dev) on the same inputs in
one run, from the context's stage timers ("shot", "shot_color": HIP events around each call's
kernels).  One warm-up call of each, then PFX_SC_REPEATS (default 9) alternating calls; the
median per call is reported with the spread, and neighbours per second from the calls' own
neighbour counts.  Inputs:
  indoor : tests/golden/clouds/indoor_source.pcd with its own colours, normals at 0.05, queries =
           its ISS keypoints (salient 6 x, non-max 4 x the cloud resolution), r = 0.08
  seabed : configs[3]'s synth_seabed(1M, seed 3), seeded random colours, queries = the fixed
           10,000-index sample of the benchmark, r = 0.08
The single-threaded CPU restatement (tests/cpp/shot_color_ref.cpp, frames given) is timed on the
indoor case with a host clock.  One JSON line per input.  Needs a GPU."""
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

from pcl_feature_extraction_amd import Context  # noqa: E402
from pcl_feature_extraction_amd.synth import synth_seabed  # noqa: E402

R = 0.08
REPEATS = int(os.environ.get("PFX_SC_REPEATS", "9"))


def indoor(ctx):
    import shot_color_ref as S
    x, y, z, rgb = S.read_cloud("indoor_source")
    res = ctx.cloud_resolution(x, y, z)
    kp = ctx.iss_keypoints(x, y, z, 6 * res, 4 * res)
    return (x, y, z), rgb, kp.astype(np.int64)


def seabed(ctx):
    x, y, z, _ = synth_seabed(1_000_000, 3)
    rgb = np.random.default_rng(7).integers(0, 1 << 24, len(x), dtype=np.uint32)
    return (x, y, z), rgb, np.sort(np.random.default_rng(10).choice(len(x), 10_000, replace=False))


def measure(ctx, name, xyz, rgb, rows):
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)
    s = [f(a) for a in xyz]
    nrm = [torch.empty_like(s[0]) for _ in range(4)]
    ctx.normals_dev(*s, 0.05, *nrm)
    ctx.synchronize()
    q = [f(a[rows]) for a in xyz]
    srgb, qrgb = u(rgb), u(rgb[rows])
    nq = len(rows)
    d352 = torch.empty((nq, 352), dtype=torch.float32, device=dev)
    d1344 = torch.empty((nq, 1344), dtype=torch.float32, device=dev)
    rf = torch.empty((nq, 9), dtype=torch.float32, device=dev)
    calls = {
        "shot": lambda: ctx.shot_dev(*s, *nrm[:3], *q, R, d352, rf),
        "shot_color": lambda: ctx.shot_color_dev(*s, *nrm[:3], srgb, *q, qrgb, R, d1344, rf),
    }
    for c in calls.values():  # warm-up: code objects, scratch buffers
        c()
    ctx.synchronize()
    ctx.set_timing(True, stages_only=True)
    ms = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, c in calls.items():
            ctx.reset_timing()
            c()
            ctx.synchronize()
            ms[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    nb = {"shot": ctx.stat("shot_neighbors"), "shot_color": ctx.stat("shot_color_neighbors")}
    out = {"input": name, "points": len(xyz[0]), "queries": nq, "neighbors": nb["shot_color"], "repeats": REPEATS}
    for k in calls:
        med = float(np.median(ms[k]))
        out[k + "_ms"] = round(med, 4)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[k + "_neighbors_per_s"] = round(nb[k] / (med * 1e-3), 0)
    out["color_over_shape"] = round(out["shot_color_ms"] / out["shot_ms"], 3)
    out["lut_clamped"] = ctx.stat("shot_color_lut_clamped")
    return out, [a.cpu().numpy() for a in nrm[:3]], rf.cpu().numpy()


def restatement_seconds(xyz, nrm, rgb, rows, rf):
    import shot_color_ref as S
    lib = S.build(tempfile.mkdtemp(prefix="shot_color_ref"))
    q = [np.ascontiguousarray(a[rows]) for a in xyz]
    t0 = time.perf_counter()
    S.shot_color(lib, *xyz, *nrm, rgb, *q, rgb[rows], R, rf)
    return time.perf_counter() - t0


def main():
    if not torch.cuda.is_available():
        sys.exit("shot_color_time: no GPU")
    with Context(0) as ctx:
        for name, make in (("indoor", indoor), ("seabed", seabed)):
            xyz, rgb, rows = make(ctx)
            out, nrm, rf = measure(ctx, name, xyz, rgb, rows)
            if name == "indoor":
                out["restatement_1thread_s"] = round(restatement_seconds(xyz, nrm, rgb, rows, rf), 3)
            print(json.dumps(out), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
