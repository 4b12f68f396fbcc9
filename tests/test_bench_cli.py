"""bench.py's command line: the plain run (timed steps only), --full, --dump-outputs.

The dump helper and the option parsing need no device; one -m gpu test runs the plain headline
once (2 timed steps over one scan) and checks its line and the dumped arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _load(directory):
    return {f[:-4]: np.load(os.path.join(directory, f)) for f in sorted(os.listdir(directory))}


def test_dump_keeps_small_outputs_whole(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    desc = rng.random((89, 33), dtype=np.float32)
    desc[3] = np.nan  # a descriptor row without a frame (PCL's quiet_NaN): written as 0, flagged in _valid
    desc[7, 5] = np.inf
    arrays = {"descriptors": desc, "keypoints": np.arange(89, dtype=np.int32) * 3457,
              "resolution": np.asarray([0.1 + 1e-12])}
    bench.dump_outputs(str(tmp_path / "d"), arrays)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == sorted(list(arrays) + ["descriptors_valid"])
    assert all(np.isfinite(a).all() for a in got.values())
    assert got["descriptors"].dtype == np.float32 and got["descriptors_valid"].dtype == np.float32
    bad = np.zeros(89, bool)
    bad[[3, 7]] = True
    assert np.array_equal(got["descriptors_valid"], (~bad).astype(np.float32))
    assert got["descriptors"][~bad].tobytes() == desc[~bad].tobytes()
    assert np.all(got["descriptors"][3] == 0) and got["descriptors"][7, 5] == 0
    assert np.array_equal(np.delete(got["descriptors"][7], 5), np.delete(desc[7], 5))
    assert got["keypoints"].dtype == np.float64 and np.array_equal(got["keypoints"], arrays["keypoints"])
    assert got["resolution"].dtype == np.float64 and got["resolution"][0] == arrays["resolution"][0]


def test_dump_samples_large_outputs_to_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 5 << 20)
    big = np.arange(600_000 * 4, dtype=np.float32).reshape(-1, 4)  # 9.6 MB: over the budget
    big[::1000, 1] = np.nan
    idx = np.arange(300_000, dtype=np.int32)                       # 2.4 MB as float64
    small = np.arange(33, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"normals": big, "indices": idx, "row": small})
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    files = [os.path.join(str(tmp_path / "a"), f) for f in os.listdir(str(tmp_path / "a"))]
    assert sum(os.path.getsize(f) for f in files) <= 5 << 20
    for nm in a:  # the same seeded rows in both runs
        assert a[nm].tobytes() == b[nm].tobytes()
    assert np.array_equal(a["row"], small)
    rows = a["normals"][:, 0].astype(np.int64) // 4  # every kept row is a whole row of the output, in order
    assert 0 < len(rows) < len(big) and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["normals"], np.nan_to_num(big[rows], nan=0.0))
    assert np.array_equal(a["normals_valid"], (rows % 1000 != 0).astype(np.float32))  # the same rows in both files
    assert all(np.isfinite(v).all() for v in a.values())
    assert a["indices"].dtype == np.float64 and np.all(np.diff(a["indices"]) > 0)


def test_options():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in p.stdout
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--cycle", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["unit"] == "Mpoints/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e6 / (line["ms_per_step"] * 1e-3) / 1e6) < 1e-2 * line["value"]
    for moved in ("roofline", "cpu_baseline", "end_to_end_h2d_d2h", "parity_all_scans"):
        assert moved not in line  # --full only
    got = _load(out)
    assert sorted(got) == ["descriptor_indices", "descriptors", "descriptors_valid", "keypoints", "normals",
                           "normals_valid"]
    assert all(np.isfinite(a).all() for a in got.values())
    k = line["config"]["descriptor_rows"]
    assert got["descriptors"].shape == (k, 33) and got["descriptors"].dtype == np.float32
    assert got["descriptor_indices"].shape == (k,) and got["descriptor_indices"].dtype == np.float64
    assert got["normals"].shape == (1_000_000, 4) and got["normals"].dtype == np.float32
    assert got["descriptors_valid"].shape == (k,) and got["descriptors_valid"].all() and k > 0
    # unit normals wherever the estimation found a neighbourhood, zeros elsewhere
    n = got["normals"][:, :3].astype(np.float64)
    ok = got["normals_valid"] == 1
    assert got["normals_valid"].shape == (1_000_000,) and not got["normals"][~ok].any()
    assert ok.mean() > 0.99 and np.allclose(np.linalg.norm(n[ok], axis=1), 1.0, atol=1e-5)
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= 64_000_000
