"""How often the k-NN contract's one departure from PCL can show (DESIGN.md "k-NN: the contract"): on
each of the four reference clouds (tests/golden/clouds), with the cloud as its own queries and
k = 10, 30, 100, the share of rows that hold two neighbours of exactly equal float32 d2 (their order
inside the row is the index's here, the tree's visiting order in FLANN) and the share whose k-th and
(k+1)-th d2 are equal (there the tie decides who is in the row).  CPU only; needs scipy.

A row's candidates are the k + 32 nearest points of a float64 kd-tree; their d2 is then formed by the
contract's float32 statement and the row ordered by (d2, index), so a tie is counted exactly where the
library and the restatement see one (a float32 tie that reaches across more than 32 places of the
float64 order would be missed; none is plausible at these densities).  One JSON line per cloud and k."""
import glob
import json
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pcl_feature_extraction_amd.pcd import read_pcd  # noqa: E402

f32 = np.float32


def report(path, ks=(10, 30, 100), margin=32):
    c = read_pcd(path)
    fin = np.isfinite(c.x) & np.isfinite(c.y) & np.isfinite(c.z)
    x, y, z = c.x[fin], c.y[fin], c.z[fin]
    n = len(x)
    tree = cKDTree(np.stack([x, y, z], 1).astype(np.float64))
    _, nb = tree.query(tree.data, k=max(ks) + margin, workers=-1)
    dx, dy, dz = x[:, None] - x[nb], y[:, None] - y[nb], z[:, None] - z[nb]
    d2 = ((f32(0) + dx * dx) + dy * dy) + dz * dz
    key = np.sort((d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | nb.astype(np.uint64), axis=1)
    d = (key >> np.uint64(32)).astype(np.uint32)
    for k in ks:
        inside = (d[:, 1:k] == d[:, : k - 1]).any(axis=1)
        edge = d[:, k] == d[:, k - 1]
        print(json.dumps({"cloud": os.path.basename(path), "points": n, "k": k,
                          "rows_with_a_tie_inside": int(inside.sum()), "share_inside": round(float(inside.mean()), 5),
                          "rows_with_a_tie_at_k": int(edge.sum()), "share_at_k": round(float(edge.mean()), 5)}),
              flush=True)


if __name__ == "__main__":
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "clouds", "*.pcd"))):
        report(p)
