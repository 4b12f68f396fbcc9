"""Measurement: the intensity gradient and RIFT (pfx_rift.hip) from the context's HIP-event timers, in
one process.  One warm-up call of each, then PFX_RT_REPEATS (default 9) alternating calls; the
median per call is reported with its minimum and maximum.  Per cloud
(tests/golden/clouds/indoor_source.pcd and underwater_source.pcd), intensities from the colours and
normals at 0.05:
  * the whole-cloud gradient at r = 0.05 ("intensity_gradient_cloud": k_igrad_lists alone, the lists
    already built) next to Harris6D's gradient stage on the same cloud and radius ("harris6d_gradient":
    k_intensity_gradient alone, pfx_harris6d_keypoints_dev at radius 0.05) -- the same loop over the
    same lists; the Harris stage's own minimum-to-maximum spread is the yardstick;
  * at the cloud's ISS keypoints (salient 6 x, non-max 4 x the cloud resolution), r = 0.08: the
    gradient ("intensity_gradient"), RIFT with 4 x 8 bins ("rift") and, for scale, spin images
    ("spin_image", W = 8) on the same queries.
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

REPEATS = int(os.environ.get("PFX_RT_REPEATS", "9"))


def measure(ctx, name):
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", name + ".pcd"))
    rgb = np.ascontiguousarray(c.fields["rgb"]).view(np.uint32)
    res = ctx.cloud_resolution(c.x, c.y, c.z)
    rows = ctx.iss_keypoints(c.x, c.y, c.z, 6 * res, 4 * res).astype(np.int64)
    dev = torch.device("cuda", 0)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    s = [f(a) for a in (c.x, c.y, c.z)]
    si = f(rgb_to_intensity(rgb))
    d_rgb = torch.from_numpy(rgb.view(np.int32)).to(dev)
    n, nq = len(c.x), len(rows)
    nrm = [torch.empty_like(s[0]) for _ in range(4)]
    ctx.normals_dev(*s, 0.05, *nrm)
    ctx.synchronize()
    idx = torch.from_numpy(rows).to(dev)
    q = [a[idx].contiguous() for a in s]
    qn = [a[idx].contiguous() for a in nrm[:3]]
    grad = torch.empty((n, 3), dtype=torch.float32, device=dev)
    g_q = torch.empty((nq, 3), dtype=torch.float32, device=dev)
    d32 = torch.empty((nq, 32), dtype=torch.float32, device=dev)
    d153 = torch.empty((nq, 153), dtype=torch.float32, device=dev)
    h_idx = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.intensity_gradient_dev(*s, si, *s, *nrm[:3], 0.05, grad, same_as_surface=True)
    ctx.synchronize()
    sg = [grad[:, i].contiguous() for i in range(3)]
    torch.cuda.synchronize()
    calls = {
        "intensity_gradient_cloud": lambda: ctx.intensity_gradient_dev(*s, si, *s, *nrm[:3], 0.05, grad,
                                                                       same_as_surface=True),
        "harris6d_gradient": lambda: ctx.harris6d_keypoints_dev(*s, d_rgb, h_idx, radius=0.05),
        "intensity_gradient": lambda: ctx.intensity_gradient_dev(*s, si, *q, *qn, 0.08, g_q),
        "rift": lambda: ctx.rift_dev(*s, *sg, *q, 0.08, d32),
        "spin_image": lambda: ctx.spin_image_dev(*s, *q, *qn, 0.08, d153),
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
           "rift_neighbors": ctx.stat("rift_neighbors"), "rift_kmax": ctx.stat("rift_kmax"),
           "rift_queued": ctx.stat("rift_queued")}
    for k in calls:
        out[k + "_ms"] = round(float(np.median(ms[k])), 4)
        out[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    out["cloud_gradient_over_harris_stage"] = round(out["intensity_gradient_cloud_ms"] / out["harris6d_gradient_ms"], 3)
    out["rift_over_spin"] = round(out["rift_ms"] / out["spin_image_ms"], 3)
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("rift_time: no GPU")
    with Context(0) as ctx:
        for name in ("indoor_source", "underwater_source"):
            print(json.dumps(measure(ctx, name)), flush=True)
            ctx.trim()


if __name__ == "__main__":
    main()
