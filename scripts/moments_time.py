"""Measurement: moment invariants and principal curvatures (pfx_moments.hip) from the context's
HIP-event timers, in one process.  One warm-up call of each, then PFX_MT_REPEATS (default 9)
alternating calls; the median per call is reported with its minimum and maximum.  Per cloud
(tests/golden/clouds/indoor_source.pcd and underwater_source.pcd), at the cloud's ISS keypoints
(salient 6 x, non-max 4 x the cloud resolution), r = 0.08, normals at 0.05:
  * "moment_invariants" and "principal_curvatures";
  * as the yardstick, the intensity gradient's query path ("intensity_gradient") on the same queries:
    the same sort and the same two passes with more arithmetic, whose own minimum-to-maximum spread
    says what a difference means.
One JSON line per cloud.  Needs a GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pcl_feature_extraction_amd import Context, rgb_to_intensity  # noqa: E402
from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402

REPEATS = int(os.environ.get("PFX_MT_REPEATS", "9"))


def measure(ctx, name):
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", name + ".pcd"))
    rgb = np.ascontiguousarray(c.fields["rgb"]).view(np.uint32)
    res = ctx.cloud_resolution(c.x, c.y, c.z)
    rows = ctx.iss_keypoints(c.x, c.y, c.z, 6 * res, 4 * res).astype(np.int64)
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    s = [f(a) for a in (c.x, c.y, c.z)]
    si = f(rgb_to_intensity(rgb))
    n, nq = len(c.x), len(rows)
    nrm = [torch.empty_like(s[0]) for _ in range(4)]
    ctx.normals_dev(*s, 0.05, *nrm)
    ctx.synchronize()
    idx = torch.from_numpy(rows).to(dev)
    q = [a[idx].contiguous() for a in s]
    qn = [a[idx].contiguous() for a in nrm[:3]]
    d3 = torch.empty((nq, 3), dtype=torch.float32, device=dev)
    d5 = torch.empty((nq, 5), dtype=torch.float32, device=dev)
    g3 = torch.empty((nq, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    calls = {
        "moment_invariants": lambda: ctx.moment_invariants_dev(*s, *q, 0.08, d3),
        "principal_curvatures": lambda: ctx.principal_curvatures_dev(*s, *nrm[:3], *q, *qn, 0.08, d5),
        "intensity_gradient": lambda: ctx.intensity_gradient_dev(*s, si, *q, *qn, 0.08, g3),
    }
    for call in calls.values():  # warm-up: code objects, scratch buffers
        call()
    ctx.synchronize()
    ctx.set_timing(True)
    ms = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, call in calls.items():
            ctx.reset_timing()
            call()
            ctx.synchronize()
            ms[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    out = {"input": name, "points": n, "queries": nq, "repeats": REPEATS,
           "neighbors": ctx.stat("moments_neighbors"), "kmax": ctx.stat("moments_kmax"),
           "queued": ctx.stat("moments_queued")}
    for k in calls:
        out[k + "_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    out["moments_over_gradient"] = round(out["moment_invariants_ms"] / out["intensity_gradient_ms"], 3)
    out["curvatures_over_gradient"] = round(out["principal_curvatures_ms"] / out["intensity_gradient_ms"], 3)
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("moments_time: no GPU")
    with Context(0) as ctx:
        for name in ("indoor_source", "underwater_source"):
            print(json.dumps(measure(ctx, name)), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
