"""Measurement: CVFH (pfx_cvfh.hip) from the context's HIP-event timers, in one process.  One warm-up
call, then PFX_CVFH_REPEATS (default 5) calls; the median per stage is reported.  Inputs:
  * the roof of tests/cvfh_cases.py at 20,000 and at 200,000 points (spacing 0.0025, so the larger one
    is the wider one), input normals and curvatures from Context.normals at 0.02, PCL's defaults;
  * 1,000,000 points none of which passes the curvature filter: the fallback, whose centroid is one
    sequential float sum over the whole surface.
With PFX_CVFH_CPU=1 the CPU restatement (tests/cpp/cvfh_ref.cpp) runs on the same inputs on this
host: the time of the oracle's normal estimation on the filtered cloud, and of the restatement given
those normals.  One JSON line per input.  Needs a GPU."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cvfh_cases as K  # noqa: E402
from pcl_feature_extraction_amd import Context  # noqa: E402

REPEATS = int(os.environ.get("PFX_CVFH_REPEATS", "5"))
STAGES = ("cvfh_filter", "normals", "cvfh_components", "cvfh_rank", "cvfh_means", "cvfh_fallback", "cvfh_signature")
STATS = ("cvfh_filtered", "cvfh_clusters", "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows")


def measure(ctx, what, s):
    ctx.cvfh(*s)  # warm-up: code objects, scratch buffers
    ctx.set_timing(True)
    ms = {k: [] for k in STAGES}
    wall = []
    for _ in range(REPEATS):
        ctx.reset_timing()
        t = time.perf_counter()
        ctx.cvfh(*s)
        wall.append((time.perf_counter() - t) * 1e3)
        for k in STAGES:
            ms[k].append(ctx.kernel_time(k)[0])
    ctx.set_timing(False)
    out = {"input": what, "points": len(s[0]), "repeats": REPEATS}
    out.update({k: ctx.stat(k) for k in STATS})
    out.update({k + "_ms": round(float(np.median(v)), 4) for k, v in ms.items()})
    out["host_call_ms"] = round(float(np.median(wall)), 3)
    return out


def cpu(s):
    import cvfh_ref as R
    import oracle_lib as O
    lib = R.build(tempfile.mkdtemp())
    spent = {}

    def normals(x, y, z, r):
        t = time.perf_counter()
        n = O.normals(x, y, z, r)
        spent["cpu_normals_s"] = round(time.perf_counter() - t, 3)
        return n

    t = time.perf_counter()
    R.cvfh(lib, normals, *s)
    spent["cpu_restatement_s"] = round(time.perf_counter() - t - spent.get("cpu_normals_s", 0.0), 3)
    return spent


def main():
    with Context(0) as ctx:
        for m in (100, 316):
            xyz = K.roof(m, 0.0025, 0.00025)
            s = xyz + tuple(ctx.normals(*xyz, 0.02))
            out = measure(ctx, "roof", s)
            if os.environ.get("PFX_CVFH_CPU") == "1":
                out.update(cpu(s))
            print(json.dumps(out), flush=True)
        n = 1000000
        rng = np.random.default_rng(1)
        xyz = K.f32(*(rng.random((3, n)) + 1.0))
        nx, ny, nz, curv = K.flat_normals(n)
        print(json.dumps(measure(ctx, "fallback", xyz + (nx, ny, nz, curv + np.float32(1.0)))), flush=True)


if __name__ == "__main__":
    main()
