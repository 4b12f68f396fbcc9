"""Measurement: the boundary points (pfx_boundary.hip) from the context's HIP-event timers, in one
process.  One warm-up call of each, then PFX_BOUNDARY_REPEATS (default 9) alternating calls; the median
per call is reported with its minimum and maximum.  On tests/golden/clouds/indoor_source.pcd, r = 0.08,
normals at 0.05, PCL's default angle threshold, at two sets of queries (each with its own normal):
  * the cloud rows at its ISS keypoints (6 and 4 cloud resolutions);
  * 10,000 seeded rows of the cloud.
For scale, the two kernels that gather the same neighbourhoods and also sort them, BOARD's frames
("board_lrf") and SHOT's frames alone ("shot_lrf"), run on the same rows in the same run.  One JSON line
per set.  Needs a GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pcl_feature_extraction_amd import Context  # noqa: E402
from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402

REPEATS = int(os.environ.get("PFX_BOUNDARY_REPEATS", "9"))


def measure(ctx, what, s, sn, rows):
    dev = s[0].device
    idx = torch.from_numpy(np.asarray(rows, np.int64)).to(dev)
    q = [a[idx].contiguous() for a in s]
    qn = [a[idx].contiguous() for a in sn]
    nq = len(rows)
    flags = torch.empty(nq, dtype=torch.uint8, device=dev)
    rf = [torch.empty((nq, 9), dtype=torch.float32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    calls = {
        "boundary": lambda: ctx.boundary_dev(*s, *q, *qn, 0.08, flags),
        "board_lrf": lambda: ctx.board_lrf_dev(*s, *sn, *q, 0.08, rf[0]),
        "shot_lrf": lambda: ctx.shot_lrf_dev(*s, *q, 0.08, rf[1]),
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
    out = {"input": "indoor_source", "keypoints": what, "points": int(s[0].numel()), "queries": nq, "repeats": REPEATS,
           "boundary_neighbors": ctx.stat("boundary_neighbors"), "boundary_kmax": ctx.stat("boundary_kmax"),
           "boundary_flagged": ctx.stat("boundary_flagged"),
           "no_neighbor_rows": int((flags == 255).sum().item())}
    for k in calls:
        out[k + "_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    out["boundary_over_board_lrf"] = round(out["boundary_ms"] / out["board_lrf_ms"], 3)
    out["boundary_over_shot_lrf"] = round(out["boundary_ms"] / out["shot_lrf_ms"], 3)
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("boundary_time: no GPU")
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd"))
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    with Context(0) as ctx:
        res = ctx.cloud_resolution(c.x, c.y, c.z)
        iss = np.asarray(ctx.iss_keypoints(c.x, c.y, c.z, 6 * res, 4 * res), np.int64)
        s = [f(a) for a in (c.x, c.y, c.z)]
        nrm = [torch.empty_like(s[0]) for _ in range(4)]
        ctx.normals_dev(*s, 0.05, *nrm)
        ctx.synchronize()
        fin = np.flatnonzero(np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z))
        sample = np.sort(np.random.default_rng(31).choice(fin, 10000, replace=False))
        for what, rows in (("iss_keypoints", iss), ("10000_seeded_rows", sample)):
            print(json.dumps(measure(ctx, what, s, nrm[:3], rows)), flush=True)


if __name__ == "__main__":
    main()
