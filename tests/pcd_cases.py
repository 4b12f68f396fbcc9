"""PCD files for the loader tests (pcl::io::loadPCDFile<PointXYZRGB>, evaluation.cpp:226-235):
ascii as pcl::io::savePCDFile writes it (evaluation.cpp:258), and binary with other field
orders, extra and 1-byte fields (unaligned x y z), comments and NaN points; and the binary
x y z rgb layout of the reference's clouds with a VIEWPOINT of choice (the sensor pose of the NARF
branch, keypoints.h:207-216)."""
import numpy as np


def cloud(n, seed):
    r = np.random.default_rng(seed)
    x, y, z = (r.normal(0, 2, n).astype(np.float32) for _ in range(3))
    x[::17] = np.nan  # non-dense cloud
    return x, y, z


def write_ascii(path, x, y, z):
    n = len(x)
    rgb = np.arange(n, dtype=np.uint32) * 2654435761 % (1 << 24)
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\n"
                "TYPE F F F U\nCOUNT 1 1 1 1\n" f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 1 2 3 1 0 0 0\nPOINTS {n}\n"
                "DATA ascii\n")
        for i in range(n):
            f.write(f"{x[i]:.9g} {y[i]:.9g} {z[i]:.9g} {rgb[i]}\n")


def write_binary_mixed(path, x, y, z):
    """FIELDS intensity(u8) label(u16) z y curvature x : x y z at unaligned byte offsets."""
    n = len(x)
    dt = np.dtype([("intensity", "u1"), ("label", "<u2"), ("z", "<f4"), ("y", "<f4"), ("curvature", "<f4"),
                   ("x", "<f4")])
    rec = np.zeros(n, dt)
    rec["x"], rec["y"], rec["z"] = x, y, z
    rec["intensity"] = np.arange(n) % 251
    rec["label"] = np.arange(n) % 60000
    with open(path, "wb") as f:
        f.write(("# comment line\nVERSION 0.7\nFIELDS intensity label z y curvature x\nSIZE 1 2 4 4 4 4\n"
                 "TYPE U U F F F F\nCOUNT 1 1 1 1 1 1\n" f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
                 f"POINTS {n}\nDATA binary\n").encode())
        f.write(rec.tobytes())


def quaternion_of(r):
    """Unit quaternion (w, x, y, z), float32, of a 3x3 rotation matrix with w well away from 0."""
    r = np.asarray(r, np.float64)
    w = 0.5 * np.sqrt(1.0 + r[0, 0] + r[1, 1] + r[2, 2])
    q = np.array([w, (r[2, 1] - r[1, 2]) / (4 * w), (r[0, 2] - r[2, 0]) / (4 * w), (r[1, 0] - r[0, 1]) / (4 * w)])
    return (q / np.linalg.norm(q)).astype(np.float32)


def viewpoint_pose(t, q):
    """Affine3f(Translation3f(t)) * Affine3f(Quaternionf(q)) in include/pfx_pcl.hpp's own float32
    operation order (Eigen's toRotationMatrix, then the 4x4 product summed k = 0..3 from 0):
    the 16 row-major floats the facade hands to pfx_camera.sensor_pose, bit for bit."""
    f = np.float32
    qw, qx, qy, qz = (f(v) for v in q)
    tx, ty, tz = f(2) * qx, f(2) * qy, f(2) * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    rot = np.eye(4, dtype=f)
    rot[0, :3] = f(1) - (tyy + tzz), txy - twz, txz + twy
    rot[1, :3] = txy + twz, f(1) - (txx + tzz), tyz - twx
    rot[2, :3] = txz - twy, tyz + twx, f(1) - (txx + tyy)
    tr = np.eye(4, dtype=f)
    tr[:3, 3] = [f(v) for v in t]
    out = np.zeros((4, 4), f)
    for i in range(4):
        for j in range(4):
            s = f(0)
            for k in range(4):
                s = f(s + f(tr[i, k] * rot[k, j]))
            out[i, j] = s
    return out


def write_binary_xyzrgb(path, x, y, z, viewpoint=(0, 0, 0, 1, 0, 0, 0)):
    """PCL's binary PointXYZRGB layout (16 B per point); viewpoint = tx ty tz qw qx qy qz, written
    with 9 significant digits so that a float32 reads back exactly."""
    n = len(x)
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = x, y, z
    vp = " ".join("%.9g" % float(np.float32(v)) for v in viewpoint)
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\n"
                 "TYPE F F F F\nCOUNT 1 1 1 1\n" f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT {vp}\nPOINTS {n}\n"
                 "DATA binary\n").encode())
        f.write(rec.tobytes())
