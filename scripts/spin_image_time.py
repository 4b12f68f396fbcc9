"""Measurement: spin images (pfx_spin_image_dev, W = 8) against SHOT-352 (pfx_shot_dev) on the same
inputs in one run, from the context's stage timers ("shot", "spin_image": HIP events around each
call's kernels).  One warm-up call of each, then PFX_SI_REPEATS (default 9) alternating calls; the
median per call is reported with the spread, and neighbours per second from the calls' own
neighbour counts.  The rotation axis of a query is the surface normal at that point.  Inputs:
  indoor : tests/golden/clouds/indoor_source.pcd, normals at 0.05, queries = its ISS keypoints
           (salient 6 x, non-max 4 x the cloud resolution), r = 0.08
  seabed : configs[3]'s synth_seabed(1M, seed 3), queries = the fixed 10,000-index sample of the
           benchmark, r = 0.08
The single-threaded CPU restatement (tests/cpp/spin_ref.cpp) is timed on both with a host clock.
One JSON line per input.  Needs a GPU."""
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
from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402
from pcl_feature_extraction_amd.synth import synth_seabed  # noqa: E402

R = 0.08
REPEATS = int(os.environ.get("PFX_SI_REPEATS", "9"))


def indoor(ctx):
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd"))
    res = ctx.cloud_resolution(c.x, c.y, c.z)
    kp = ctx.iss_keypoints(c.x, c.y, c.z, 6 * res, 4 * res)
    return (c.x, c.y, c.z), kp.astype(np.int64)


def seabed(ctx):
    x, y, z, _ = synth_seabed(1_000_000, 3)
    return (x, y, z), np.sort(np.random.default_rng(10).choice(len(x), 10_000, replace=False))


def measure(ctx, name, xyz, rows):
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    s = [f(a) for a in xyz]
    nrm = [torch.empty_like(s[0]) for _ in range(4)]
    ctx.normals_dev(*s, 0.05, *nrm)
    ctx.synchronize()
    q = [f(a[rows]) for a in xyz]
    idx = torch.from_numpy(rows).to(dev)
    axes = [n[idx].contiguous() for n in nrm[:3]]
    nq = len(rows)
    d352 = torch.empty((nq, 352), dtype=torch.float32, device=dev)
    rf = torch.empty((nq, 9), dtype=torch.float32, device=dev)
    d153 = torch.empty((nq, 153), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    calls = {
        "shot": lambda: ctx.shot_dev(*s, *nrm[:3], *q, R, d352, rf),
        "spin_image": lambda: ctx.spin_image_dev(*s, *q, *axes, R, d153),
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
    nb = {"shot": ctx.stat("shot_neighbors"), "spin_image": ctx.stat("spin_neighbors")}
    out = {"input": name, "points": len(xyz[0]), "queries": nq, "neighbors": nb["spin_image"], "repeats": REPEATS,
           "kmax": ctx.stat("spin_kmax"), "queued": ctx.stat("spin_queued")}
    for k in calls:
        med = float(np.median(ms[k]))
        out[k + "_ms"] = round(med, 4)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        out[k + "_neighbors_per_s"] = round(nb[k] / (med * 1e-3), 0)
    out["spin_over_shot"] = round(out["spin_image_ms"] / out["shot_ms"], 3)
    return out, [a.cpu().numpy() for a in axes], d153.cpu().numpy()


def restatement_seconds(xyz, rows, axes, got):
    import spin_ref as P
    lib = P.build(tempfile.mkdtemp(prefix="spin_ref"))
    q = [np.ascontiguousarray(a[rows]) for a in xyz]
    t0 = time.perf_counter()
    want = P.spin(lib, *xyz, *q, *axes, R)
    dt = time.perf_counter() - t0
    same = np.array_equal(np.ascontiguousarray(got).view(np.uint32), want.out.view(np.uint32))
    return dt, bool(same)


def main():
    if not torch.cuda.is_available():
        sys.exit("spin_image_time: no GPU")
    with Context(0) as ctx:
        for name, make in (("indoor", indoor), ("seabed", seabed)):
            xyz, rows = make(ctx)
            out, axes, got = measure(ctx, name, xyz, rows)
            dt, same = restatement_seconds(xyz, rows, axes, got)
            out["restatement_1thread_s"] = round(dt, 3)
            out["rows_equal_restatement"] = same
            print(json.dumps(out), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
