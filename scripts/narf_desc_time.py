"""Measurement: the NARF descriptors (pfx_narf_desc.hip) and the point indices from the context's
HIP-event timers, in one process.  One warm-up call of each, then PFX_NARF_DESC_REPEATS (default 9)
calls; the median per call is reported with its minimum and maximum.  On
tests/golden/clouds/indoor_source.pcd with the reference's 640 x 480 camera:
  * "narf_desc" (k_narf_desc, the scan and the compaction; the range image is outside it) at every
    valid pixel of a lattice of every 67th pixel, support 0.2 and 0.5, with rotation invariance;
  * "point_indices" (both passes and the scan) for the cloud's points at those pixels as keypoints.
One JSON line per setting.  Needs a GPU."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pcl_feature_extraction_amd import Context, camera, narf_desc_params  # noqa: E402
from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402

REPEATS = int(os.environ.get("PFX_NARF_DESC_REPEATS", "9"))


def timed(ctx, name, call):
    call()
    ctx.synchronize()
    ctx.set_timing(True)
    ms = []
    for _ in range(REPEATS):
        ctx.reset_timing()
        call()
        ctx.synchronize()
        ms.append(ctx.kernel_time(name)[0])
    ctx.set_timing(False)
    return round(float(np.median(ms)), 4), [round(min(ms), 4), round(max(ms), 4)]


def main():
    c = read_pcd(os.path.join(ROOT, "tests", "golden", "clouds", "indoor_source.pcd"))
    dev = torch.device("cuda", 0)
    with Context(0) as ctx:
        cam = camera()
        ri = ctx.range_image_planar(c.x, c.y, c.z, cam)
        valid = np.flatnonzero(np.isfinite(ri[..., 3].ravel()))
        pix = valid[valid % 67 == 0].astype(np.int32)
        s = [torch.tensor(np.asarray(v), device=dev) for v in (c.x, c.y, c.z)]
        dpix = torch.tensor(pix, device=dev)
        cap = 5 * len(pix)
        desc = torch.empty((cap, 36), device=dev)
        pose = torch.empty((cap, 12), device=dev)
        key = torch.empty(cap, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for support in (0.2, 0.5):
            prm = narf_desc_params(support, True)
            ms, rng = timed(ctx, "narf_desc", lambda: ctx.narf_descriptors_dev(*s, dpix, desc, pose, key, prm, cam))
            print(json.dumps({"input": "indoor_source", "points": len(c.x), "entries": len(pix), "support": support,
                              "repeats": REPEATS, "narf_desc_ms": ms, "narf_desc_ms_min_max": rng,
                              **{k: ctx.stat("narf_desc_" + k) for k in
                                 ("rows", "fallback_normals", "pose_failed", "ring_max", "background_cells")}}))
        pts = ri.reshape(-1, 4)[pix]
        k = [torch.tensor(np.ascontiguousarray(pts[:, i]), device=dev) for i in range(3)]
        out = torch.empty(4 * len(pix) + 64, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        count = [None]

        def call():
            count[0] = ctx.point_indices_dev(*s, *k, out)
        ms, rng = timed(ctx, "point_indices", call)
        print(json.dumps({"input": "indoor_source", "points": len(c.x), "keypoints": len(pix), "repeats": REPEATS,
                          "point_indices_ms": ms, "point_indices_ms_min_max": rng, "indices": int(count[0].item())}))


if __name__ == "__main__":
    main()
