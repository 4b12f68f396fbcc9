"""Measurement: the 3D shape context and USC (pfx_shape_context.hip) from the context's HIP-event
timers, in one process.  One warm-up call of each, then PFX_SCT_REPEATS (default 9) alternating calls;
the median per call is reported with its minimum and maximum.  Per cloud
(tests/golden/clouds/indoor_source.pcd and underwater_source.pcd), normals at 0.05, at the cloud's ISS
keypoints (salient 6 x, non-max 4 x the cloud resolution), R = 0.08, rmin = R / 10, rho = R / 5:
  * "sc_density": the support marks, the draw ranks and the density counts of a 3DSC call;
  * "shape_context": the descriptor kernel of the same call, and of a USC call on pfx_shot_lrf's frames
    ("usc");
  * "shot_lrf": the frames alone;
  * "shot": SHOT-352 on the same queries in the same run, the yardstick.
One JSON line per cloud.  Needs a GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pcl_feature_extraction_amd import Context  # noqa: E402
from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402

REPEATS = int(os.environ.get("PFX_SCT_REPEATS", "9"))
R = 0.08


def measure(ctx, name):
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", name + ".pcd"))
    res = ctx.cloud_resolution(c.x, c.y, c.z)
    rows = ctx.iss_keypoints(c.x, c.y, c.z, 6 * res, 4 * res).astype(np.int64)
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    s = [f(a) for a in (c.x, c.y, c.z)]
    n, nq = len(c.x), len(rows)
    nrm = [torch.empty_like(s[0]) for _ in range(4)]
    ctx.normals_dev(*s, 0.05, *nrm)
    ctx.synchronize()
    idx = torch.from_numpy(rows).to(dev)
    q = [a[idx].contiguous() for a in s]
    new = lambda w: torch.empty((nq, w), dtype=torch.float32, device=dev)  # noqa: E731
    d1980, rf, frames, d352, rf352 = new(1980), new(9), new(9), new(352), new(9)
    ctx.shot_lrf_dev(*s, *q, R, frames)
    ctx.synchronize()
    torch.cuda.synchronize()
    # call -> the timers read after it
    calls = {
        "3dsc": (lambda: ctx.shape_context_dev(*s, *nrm[:3], *q, R, d1980, rf), ("sc_density", "shape_context")),
        "usc": (lambda: ctx.usc_dev(*s, *q, frames, R, d1980, rf), ("sc_density", "shape_context")),
        "lrf": (lambda: ctx.shot_lrf_dev(*s, *q, R, frames), ("shot_lrf",)),
        "shot": (lambda: ctx.shot_dev(*s, *nrm[:3], *q, R, d352, rf352), ("shot",)),
    }
    for call, _ in calls.values():  # warm-up: code objects, scratch buffers, the default stream's upload
        call()
    ctx.synchronize()
    stats = {}
    ctx.set_timing(True)
    ms = {}
    for _ in range(REPEATS):
        for k, (call, timers) in calls.items():
            ctx.reset_timing()
            call()
            ctx.synchronize()
            for t in timers:
                ms.setdefault(k + ":" + t, []).append(ctx.kernel_time(t)[0])
            if k == "3dsc":
                stats = {w: ctx.stat("sc_" + w) for w in ("support", "neighbors", "kmax", "queued", "draws")}
    ctx.set_timing(False)
    out = {"input": name, "points": n, "queries": nq, "repeats": REPEATS}
    out.update({"sc_" + k: v for k, v in stats.items()})
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    out["3dsc_over_shot"] = round((out["3dsc:sc_density_ms"] + out["3dsc:shape_context_ms"]) / out["shot:shot_ms"], 3)
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("shape_context_time: no GPU")
    with Context(0) as ctx:
        for name in ("indoor_source", "underwater_source"):
            print(json.dumps(measure(ctx, name)), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
