"""Python front-end of libpfx (host numpy arrays or torch device tensors).

Every call goes through the HIP C-ABI (include/pfx.h); nothing here computes features on the
CPU.  ``Context`` owns one ``pfx_ctx`` (one HIP stream) on one device.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

import collections

from . import _native as N


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u32(a):
    """Packed 0x00RRGGBB colour words; int32 input keeps its bits."""
    a = np.asarray(a)
    if a.dtype == np.int32:
        a = a.view(np.uint32)
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.c_void_p(a.data_ptr())  # torch tensor (device pointer)


def narf_params(support_size=0.2, **kw) -> N.NarfParams:
    p = N.NarfParams()
    N.lib().pfx_narf_params_default(ctypes.byref(p))
    p.support_size = support_size
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def narf_desc_params(support_size=0.2, rotation_invariant=True) -> N.NarfDescParams:
    """pfx_narf_desc_params; rotation_invariant is PCL's default (pfx_narf_desc_params_default), the
    support size the reference's."""
    p = N.NarfDescParams()
    N.lib().pfx_narf_desc_params_default(ctypes.byref(p))
    p.support_size, p.rotation_invariant = float(support_size), int(bool(rotation_invariant))
    return p


def icp_params(**kw) -> N.IcpParams:
    """pfx_icp_params with PCL's defaults (sqrt(DBL_MAX), 10, 0, -DBL_MAX); the reference's icpAlign
    sets max_correspondence_distance=0.07, max_iterations=100, transformation_epsilon=1e-6,
    euclidean_fitness_epsilon=1e-4."""
    p = N.IcpParams()
    N.lib().pfx_icp_params_default(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"icp_params: unknown field {k}")
        setattr(p, k, v)
    return p


def uniform01_stream(seed, n, skip=0) -> np.ndarray:
    """n float32 of the shape context's random stream (boost::mt19937 seeded `seed`, read through
    uniform_01<float>) after skipping `skip` floats (pfx_rng_uniform01; host only)."""
    out = np.empty(int(n), dtype=np.float32)
    code = N.lib().pfx_rng_uniform01(int(seed) & 0xffffffff, int(skip), int(n), _ptr(out))
    if code != 0:
        raise N.PfxError(code, "uniform01_stream: skip and n must be >= 0")
    return out


def spin_params(image_width=8, support_angle_cos=0.0, min_pts_neighb=0, radial=0, angular=0) -> N.SpinParams:
    """pfx_spin_params; the defaults are PCL's (pfx_spin_params_default)."""
    p = N.SpinParams()
    N.lib().pfx_spin_params_default(ctypes.byref(p))
    p.image_width, p.support_angle_cos, p.min_pts_neighb = int(image_width), float(support_angle_cos), int(min_pts_neighb)
    p.radial, p.angular = int(radial), int(angular)
    return p


def board_params(tangent_radius=0.0, margin_thresh=0.85, find_holes=False) -> N.BoardParams:
    """pfx_board_params; the defaults are PCL's (pfx_board_params_default).  The three hole parameters
    keep their defaults: they matter only with find_holes, which is not supported."""
    p = N.BoardParams()
    N.lib().pfx_board_params_default(ctypes.byref(p))
    p.tangent_radius, p.margin_thresh, p.find_holes = float(tangent_radius), float(margin_thresh), int(bool(find_holes))
    return p


def cvfh_params(viewpoint=(0.0, 0.0, 0.0), radius_normals=None, cluster_tolerance=None, eps_angle_threshold=None,
                curvature_threshold=None, min_points=None, normalize_bins=False) -> N.CvfhParams:
    """pfx_cvfh_params; what is left None keeps PCL's default (pfx_cvfh_params_default: 0.015f, 0.015f,
    0.125f, 0.03f, 50)."""
    p = N.CvfhParams()
    N.lib().pfx_cvfh_params_default(ctypes.byref(p))
    p.viewpoint[0], p.viewpoint[1], p.viewpoint[2] = map(float, viewpoint)
    for k, v in (("radius_normals", radius_normals), ("cluster_tolerance", cluster_tolerance),
                 ("eps_angle_threshold", eps_angle_threshold), ("curvature_threshold", curvature_threshold)):
        if v is not None:
            setattr(p, k, float(v))
    if min_points is not None:
        p.min_points = int(min_points)
    p.normalize_bins = int(bool(normalize_bins))
    return p


def rgb_to_intensity(rgb) -> np.ndarray:
    """pcl::PointXYZRGBtoXYZI on packed 0x00RRGGBB words: (0.299f * r + 0.587f * g) + 0.114f * b,
    every step in float32.  Input preparation for Context.intensity_gradient, not a feature."""
    c = _u32(rgb)
    r = ((c >> 16) & 255).astype(np.float32)
    g = ((c >> 8) & 255).astype(np.float32)
    b = (c & 255).astype(np.float32)
    return (np.float32(0.299) * r + np.float32(0.587) * g) + np.float32(0.114) * b


#: result of Context.narf_descriptors: desc (m, 36), pose (m, 12) the row-major 3 x 4 world -> patch
#: transforms, keypoint (m,) the entry of pixel_idx each row came from
NarfDescriptors = collections.namedtuple("NarfDescriptors", "desc pose keypoint")

#: result of Context.cvfh: rows (m, 308), centroids (m, 3) and dominant_normals (m, 3) what each row is
#: about, labels (n_indices,) the indexed point's cluster or -1
Cvfh = collections.namedtuple("Cvfh", "rows centroids dominant_normals labels")

#: result of Context.icp / icp_dev; state: 0 not converged, 1 iterations, 2 transform, 3 absolute
#: MSE, 4 relative MSE, 5 no correspondences (pfx.h PFX_ICP_*); aligned: (x, y, z) or None
IcpResult = collections.namedtuple("IcpResult",
                                   "transformation fitness converged iterations state aligned")


def pcd_header(path) -> N.PcdHeader:
    """PCD header through the C-ABI (host only: no device needed)."""
    h = N.PcdHeader()
    st = N.lib().pfx_pcd_read_header(str(path).encode(), ctypes.byref(h))
    if st != 0:
        raise N.PfxError(st, f"pfx_pcd_read_header({path})")
    return h


def camera(**kw) -> N.Camera:
    c = N.Camera()
    N.lib().pfx_camera_default(ctypes.byref(c))
    for k, v in kw.items():
        if k == "sensor_pose":
            for i, e in enumerate(np.asarray(v, dtype=np.float32).reshape(16)):
                c.sensor_pose[i] = float(e)
        else:
            setattr(c, k, v)
    return c


class Context:
    def __init__(self, device: int = 0):
        self._lib = N.lib()
        h = ctypes.c_void_p()
        code = self._lib.pfx_ctx_create(device, ctypes.byref(h))
        if code != 0:
            raise N.PfxError(code, f"pfx_ctx_create(device={device}) failed")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self._lib.pfx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, code):
        if code != 0:
            raise N.PfxError(code, self._lib.pfx_last_error(self.h).decode())

    # ---- plumbing ------------------------------------------------------------------
    def set_stream(self, stream_handle):
        """Run on an external HIP stream (torch's `stream.cuda_stream`; 0 = the null stream)."""
        self._check(self._lib.pfx_ctx_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def use_own_stream(self):
        self._check(self._lib.pfx_ctx_use_own_stream(self.h))

    def synchronize(self):
        """Waits for this context's stream; raises deferred errors of the stream-ordered calls
        (an FPFH neighbourhood beyond capacity -> PfxError, its rows NaN)."""
        self._check(self._lib.pfx_ctx_synchronize(self.h))

    def trim(self):
        """Frees every device scratch buffer of this context (pfx_ctx_trim)."""
        self._check(self._lib.pfx_ctx_trim(self.h))

    def set_shared(self, shared=True):
        """Launch-shape hint: another stream runs latency-critical work on this device
        concurrently (pfx_ctx_set_shared); results are unchanged."""
        self._check(self._lib.pfx_ctx_set_shared(self.h, 1 if shared else 0))

    def set_timing(self, enable=True, stages_only=False):
        """HIP-event timers on this context's stream: every kernel group, or (stages_only) one event
        pair per stage call (normals, normals_fast, shot, iss, ...: the live roofline's timer)."""
        self._check(self._lib.pfx_ctx_set_timing(self.h, (2 if stages_only else 1) if enable else 0))

    def reset_timing(self):
        self._check(self._lib.pfx_ctx_reset_timing(self.h))

    def kernel_time(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self._lib.pfx_ctx_kernel_time(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def stat(self, name):
        v = ctypes.c_int64()
        self._check(self._lib.pfx_ctx_last_stats(self.h, name.encode(), ctypes.byref(v)))
        return v.value

    # ---- host-array entry points ---------------------------------------------------
    def radius_search(self, x, y, z, qx, qy, qz, r, cap=0):
        x, y, z, qx, qy, qz = map(_f32, (x, y, z, qx, qy, qz))
        nq = len(qx)
        counts = np.zeros(nq, dtype=np.int64)
        idx = d2 = None
        if cap:
            idx = np.full((nq, cap), -1, dtype=np.int32)
            d2 = np.full((nq, cap), np.nan, dtype=np.float32)
        self._check(self._lib.pfx_radius_search(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), _ptr(qx), _ptr(qy),
                                                _ptr(qz), nq, float(r), _ptr(counts), _ptr(idx), _ptr(d2),
                                                int(cap)))
        return counts, idx, d2

    def knn_search(self, x, y, z, qx, qy, qz, k):
        """KdTreeFLANN::nearestKSearch (pfx_knn_search), host arrays: (counts (nq,) int64, idx (nq, k)
        int32, d2 (nq, k) float32); each row the min(k, finite points) smallest (d2, index) ascending,
        then -1 / NaN."""
        x, y, z, qx, qy, qz = map(_f32, (x, y, z, qx, qy, qz))
        nq, k = len(qx), int(k)
        counts = np.zeros(nq, dtype=np.int64)
        idx = np.full((nq, max(k, 1)), -1, dtype=np.int32)
        d2 = np.full((nq, max(k, 1)), np.nan, dtype=np.float32)
        self._check(self._lib.pfx_knn_search(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), _ptr(qx), _ptr(qy), _ptr(qz),
                                             nq, k, _ptr(counts), _ptr(idx), _ptr(d2)))
        return counts, idx, d2

    def normals_knn(self, x, y, z, k, viewpoint=(0.0, 0.0, 0.0)):
        """NormalEstimationOMP with setKSearch(k) (pfx_normals_knn), host arrays."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        out = np.empty((4, n), dtype=np.float32)
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals_knn(self.h, _ptr(x), _ptr(y), _ptr(z), n, int(k), _ptr(vp), _ptr(out[0]),
                                              _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
        return out[0], out[1], out[2], out[3]

    def normals(self, x, y, z, r, viewpoint=(0.0, 0.0, 0.0)):
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        out = np.empty((4, n), dtype=np.float32)
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals(self.h, _ptr(x), _ptr(y), _ptr(z), n, float(r), _ptr(vp), _ptr(out[0]),
                                          _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
        return out[0], out[1], out[2], out[3]

    def normals_fast(self, x, y, z, r, viewpoint=(0.0, 0.0, 0.0)):
        """Opt-in MFMA-covariance normals (pfx_normals_fast): not parity-exact, see include/pfx.h."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        out = np.empty((4, n), dtype=np.float32)
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals_fast(self.h, _ptr(x), _ptr(y), _ptr(z), n, float(r), _ptr(vp),
                                               _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
        return out[0], out[1], out[2], out[3]

    def fpfh(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, same_as_surface=False):
        sx, sy, sz, nx, ny, nz = map(_f32, (sx, sy, sz, nx, ny, nz))
        if same_as_surface:
            qx, qy, qz = sx, sy, sz
        qx, qy, qz = map(_f32, (qx, qy, qz))
        nq = len(qx)
        out = np.empty((nq, 33), dtype=np.float32)
        self._check(self._lib.pfx_fpfh(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz), len(sx),
                                       _ptr(qx), _ptr(qy), _ptr(qz), nq, 1 if same_as_surface else 0, float(r),
                                       _ptr(out)))
        return out

    def shot(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r):
        sx, sy, sz, nx, ny, nz, qx, qy, qz = map(_f32, (sx, sy, sz, nx, ny, nz, qx, qy, qz))
        nq = len(qx)
        desc = np.empty((nq, 352), dtype=np.float32)
        rf = np.empty((nq, 9), dtype=np.float32)
        self._check(self._lib.pfx_shot(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz), len(sx),
                                       _ptr(qx), _ptr(qy), _ptr(qz), nq, float(r), _ptr(desc), _ptr(rf)))
        return desc, rf

    def shot_color(self, sx, sy, sz, nx, ny, nz, srgb, qx, qy, qz, qrgb, r):
        """SHOTColorEstimationOMP (pfx_shot_color): srgb / qrgb are packed 0x00RRGGBB words (the low
        24 bits are read); returns desc (nq, 1344) and rf (nq, 9) float32."""
        sx, sy, sz, nx, ny, nz, qx, qy, qz = map(_f32, (sx, sy, sz, nx, ny, nz, qx, qy, qz))
        srgb, qrgb = _u32(srgb), _u32(qrgb)
        if len(srgb) != len(sx) or len(qrgb) != len(qx):
            raise ValueError("shot_color: one packed colour per surface point and per query")
        nq = len(qx)
        desc = np.empty((nq, 1344), dtype=np.float32)
        rf = np.empty((nq, 9), dtype=np.float32)
        self._check(self._lib.pfx_shot_color(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz),
                                             _ptr(srgb), len(sx), _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qrgb), nq,
                                             float(r), _ptr(desc), _ptr(rf)))
        return desc, rf

    def pfh(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r):
        """PFHEstimation (pfx_pfh): (nq, 125) float32, NaN rows for queries without neighbours."""
        sx, sy, sz, nx, ny, nz, qx, qy, qz = map(_f32, (sx, sy, sz, nx, ny, nz, qx, qy, qz))
        nq = len(qx)
        out = np.empty((nq, 125), dtype=np.float32)
        self._check(self._lib.pfx_pfh(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz), len(sx),
                                      _ptr(qx), _ptr(qy), _ptr(qz), nq, float(r), _ptr(out)))
        return out

    def spin_image(self, sx, sy, sz, qx, qy, qz, qnx, qny, qnz, r, image_width=8, support_angle_cos=0.0,
                   min_pts_neighb=0, surface_normals=None, debug=False, radial=0, angular=0):
        """SpinImageEstimation (pfx_spin_image): (nq, (W + 1)(2W + 1)) float32; (qnx, qny, qnz) is the
        rotation axis of each query (the input cloud's normal there).  surface_normals: (nx, ny, nz) of
        the surface, needed when support_angle_cos > 0.  debug=True also returns raw (nq, S) float64,
        the matrix before normalisation, and sums (nq,) float64."""
        sx, sy, sz, qx, qy, qz, qnx, qny, qnz = map(_f32, (sx, sy, sz, qx, qy, qz, qnx, qny, qnz))
        sn = (None, None, None) if surface_normals is None else tuple(map(_f32, surface_normals))
        if len(qnx) != len(qx) or any(v is not None and len(v) != len(sx) for v in sn):
            raise ValueError("spin_image: one axis per query and one normal per surface point")
        nq = len(qx)
        S = (int(image_width) + 1) * (2 * int(image_width) + 1) if 1 <= int(image_width) <= 16 else 1
        out = np.empty((nq, S), dtype=np.float32)
        raw = np.empty((nq, S), dtype=np.float64) if debug else None
        sums = np.empty(nq, dtype=np.float64) if debug else None
        p = spin_params(image_width, support_angle_cos, min_pts_neighb, radial, angular)
        self._check(self._lib.pfx_spin_image(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(sn[0]), _ptr(sn[1]),
                                             _ptr(sn[2]), len(sx), _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qnx), _ptr(qny),
                                             _ptr(qnz), nq, float(r), ctypes.byref(p), _ptr(out), _ptr(raw),
                                             _ptr(sums)))
        return (out, raw, sums) if debug else out

    def intensity_gradient(self, sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz, r, same_as_surface=False):
        """IntensityGradientEstimation with the float intensity accessor (pfx_intensity_gradient):
        (nq, 3) float32, NaN rows for queries with fewer than three neighbours.  si is the surface's
        intensity (rgb_to_intensity), (qnx, qny, qnz) the normal at each query.  same_as_surface=True:
        the queries are the surface (the whole-cloud path); the same bits either way."""
        sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz = map(_f32, (sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz))
        if len(si) != len(sx) or len(qnx) != len(qx):
            raise ValueError("intensity_gradient: one intensity per surface point and one normal per query")
        nq = len(qx)
        out = np.empty((nq, 3), dtype=np.float32)
        self._check(self._lib.pfx_intensity_gradient(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(si), len(sx),
                                                     _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qnx), _ptr(qny), _ptr(qnz),
                                                     nq, 1 if same_as_surface else 0, float(r), _ptr(out)))
        return out

    def rift(self, sx, sy, sz, sgx, sgy, sgz, cx, cy, cz, r, nr_distance_bins=4, nr_gradient_bins=8):
        """RIFTEstimation (pfx_rift): (nq, D G) float32, row[gradient_bin * D + distance_bin];
        (sgx, sgy, sgz) are the surface's intensity gradients, (cx, cy, cz) the centres."""
        sx, sy, sz, sgx, sgy, sgz, cx, cy, cz = map(_f32, (sx, sy, sz, sgx, sgy, sgz, cx, cy, cz))
        if len(sgx) != len(sx):
            raise ValueError("rift: one gradient per surface point")
        nq, D, G = len(cx), int(nr_distance_bins), int(nr_gradient_bins)
        out = np.empty((nq, D * G if 1 <= D <= 16 and 1 <= G <= 16 else 1), dtype=np.float32)
        self._check(self._lib.pfx_rift(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(sgx), _ptr(sgy), _ptr(sgz), len(sx),
                                       _ptr(cx), _ptr(cy), _ptr(cz), nq, float(r), D, G, _ptr(out)))
        return out

    def intensity_spin(self, sx, sy, sz, si, cx, cy, cz, r, nr_distance_bins=4, nr_intensity_bins=5, sigma=1.0):
        """IntensitySpinEstimation (pfx_intensity_spin): (nq, D I) float32, row[distance_bin * I +
        intensity_bin]; si is the surface's intensity (rgb_to_intensity), (cx, cy, cz) the centres; a
        NaN row for a centre without neighbours.  No normals are read."""
        sx, sy, sz, si, cx, cy, cz = map(_f32, (sx, sy, sz, si, cx, cy, cz))
        if len(si) != len(sx):
            raise ValueError("intensity_spin: one intensity per surface point")
        nq, D, I = len(cx), int(nr_distance_bins), int(nr_intensity_bins)  # noqa: E741
        out = np.empty((nq, D * I if 1 <= D <= 16 and 1 <= I <= 16 else 1), dtype=np.float32)
        self._check(self._lib.pfx_intensity_spin(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(si), len(sx), _ptr(cx),
                                                 _ptr(cy), _ptr(cz), nq, float(r), D, I, float(sigma), _ptr(out)))
        return out

    def moment_invariants(self, sx, sy, sz, qx, qy, qz, r):
        """MomentInvariantsEstimation (pfx_moment_invariants): (nq, 3) float32, j1 j2 j3 of the radius
        neighbours of each query; a NaN row for a query without neighbours."""
        sx, sy, sz, qx, qy, qz = map(_f32, (sx, sy, sz, qx, qy, qz))
        nq = len(qx)
        out = np.empty((nq, 3), dtype=np.float32)
        self._check(self._lib.pfx_moment_invariants(self.h, _ptr(sx), _ptr(sy), _ptr(sz), len(sx), _ptr(qx), _ptr(qy),
                                                    _ptr(qz), nq, float(r), _ptr(out)))
        return out

    def principal_curvatures(self, sx, sy, sz, snx, sny, snz, qx, qy, qz, qnx, qny, qnz, r):
        """PrincipalCurvaturesEstimation (pfx_principal_curvatures): (nq, 5) float32, the principal
        direction x y z, then pc1 and pc2.  (snx, sny, snz) are the surface normals, (qnx, qny, qnz)
        the normal at each query; a NaN row for a query without neighbours."""
        sx, sy, sz, snx, sny, snz, qx, qy, qz, qnx, qny, qnz = map(
            _f32, (sx, sy, sz, snx, sny, snz, qx, qy, qz, qnx, qny, qnz))
        if len(snx) != len(sx) or len(qnx) != len(qx):
            raise ValueError("principal_curvatures: one normal per surface point and one per query")
        nq = len(qx)
        out = np.empty((nq, 5), dtype=np.float32)
        self._check(self._lib.pfx_principal_curvatures(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny),
                                                       _ptr(snz), len(sx), _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qnx),
                                                       _ptr(qny), _ptr(qnz), nq, float(r), _ptr(out)))
        return out

    def shape_context(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, min_radius=None, point_density_radius=None,
                      rnd=None):
        """ShapeContext3DEstimation (pfx_shape_context): desc (nq, 1980) and rf (nq, 9) float32.  The
        minimal and point-density radii default to r / 10 and r / 5.  rnd: (3 nq) float32, three per
        drawing row (uniform01_stream); None starts the stream of seed 12345 afresh."""
        sx, sy, sz, nx, ny, nz, qx, qy, qz = map(_f32, (sx, sy, sz, nx, ny, nz, qx, qy, qz))
        nq = len(qx)
        if len(nx) != len(sx):
            raise ValueError("shape_context: one normal per surface point")
        if rnd is not None:
            rnd = _f32(rnd).ravel()
            if len(rnd) != 3 * nq:
                raise ValueError("shape_context: rnd holds three floats per query")
        rmin = float(r) / 10 if min_radius is None else float(min_radius)
        rho = float(r) / 5 if point_density_radius is None else float(point_density_radius)
        desc = np.empty((nq, 1980), dtype=np.float32)
        rf = np.empty((nq, 9), dtype=np.float32)
        self._check(self._lib.pfx_shape_context(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz),
                                                len(sx), _ptr(qx), _ptr(qy), _ptr(qz), nq, float(r), rmin, rho,
                                                _ptr(rnd), _ptr(desc), _ptr(rf)))
        return desc, rf

    def usc(self, sx, sy, sz, qx, qy, qz, frames, r, min_radius=None, point_density_radius=None):
        """UniqueShapeContext (pfx_usc) with the caller's frames, (nq, 9) float32 (x, y, z axis: shot_lrf's
        layout): desc (nq, 1980) and rf (nq, 9) float32."""
        sx, sy, sz, qx, qy, qz = map(_f32, (sx, sy, sz, qx, qy, qz))
        nq = len(qx)
        frames = _f32(frames).ravel()
        if len(frames) != 9 * nq:
            raise ValueError("usc: one frame of nine floats per query")
        rmin = float(r) / 10 if min_radius is None else float(min_radius)
        rho = float(r) / 5 if point_density_radius is None else float(point_density_radius)
        desc = np.empty((nq, 1980), dtype=np.float32)
        rf = np.empty((nq, 9), dtype=np.float32)
        self._check(self._lib.pfx_usc(self.h, _ptr(sx), _ptr(sy), _ptr(sz), len(sx), _ptr(qx), _ptr(qy), _ptr(qz),
                                      _ptr(frames), nq, float(r), rmin, rho, _ptr(desc), _ptr(rf)))
        return desc, rf

    def shot_lrf(self, sx, sy, sz, qx, qy, qz, r):
        """SHOTLocalReferenceFrameEstimation (pfx_shot_lrf): (nq, 9) float32, shot()'s rf bit for bit."""
        sx, sy, sz, qx, qy, qz = map(_f32, (sx, sy, sz, qx, qy, qz))
        rf = np.empty((len(qx), 9), dtype=np.float32)
        self._check(self._lib.pfx_shot_lrf(self.h, _ptr(sx), _ptr(sy), _ptr(sz), len(sx), _ptr(qx), _ptr(qy),
                                           _ptr(qz), len(qx), float(r), _ptr(rf)))
        return rf

    def board_lrf(self, sx, sy, sz, snx, sny, snz, qx, qy, qz, r, tangent_radius=0.0, margin_thresh=0.85,
                  find_holes=False):
        """BOARDLocalReferenceFrameEstimation (pfx_board_lrf): (nq, 9) float32, the x, y and z axis of
        every row (shot_lrf's layout); (snx, sny, snz) are the surface normals.  A NaN row for a query
        with fewer than six neighbours or without a usable normal around it.  find_holes=True is
        PFX_ERR_UNSUPPORTED."""
        sx, sy, sz, snx, sny, snz, qx, qy, qz = map(_f32, (sx, sy, sz, snx, sny, snz, qx, qy, qz))
        if len(snx) != len(sx):
            raise ValueError("board_lrf: one normal per surface point")
        rf = np.empty((len(qx), 9), dtype=np.float32)
        p = board_params(tangent_radius, margin_thresh, find_holes)
        self._check(self._lib.pfx_board_lrf(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny), _ptr(snz),
                                            len(sx), _ptr(qx), _ptr(qy), _ptr(qz), len(qx), float(r), ctypes.byref(p),
                                            _ptr(rf)))
        return rf

    def boundary(self, sx, sy, sz, qx, qy, qz, qnx, qny, qnz, r, angle_threshold=math.pi / 2):
        """BoundaryEstimation (pfx_boundary): (nq,) uint8, 1 for a query on a boundary of the surface, 0
        for one that is not, BOUNDARY_NO_NEIGHBORS for one without a neighbour.  (qnx, qny, qnz) are the
        queries' normals, one per query.  Any number of neighbours; an angle_threshold below pi / 64 is
        PFX_ERR_UNSUPPORTED."""
        sx, sy, sz, qx, qy, qz, qnx, qny, qnz = map(_f32, (sx, sy, sz, qx, qy, qz, qnx, qny, qnz))
        if len(qnx) != len(qx):
            raise ValueError("boundary: one normal per query")
        out = np.empty(len(qx), dtype=np.uint8)
        self._check(self._lib.pfx_boundary(self.h, _ptr(sx), _ptr(sy), _ptr(sz), len(sx), _ptr(qx), _ptr(qy),
                                           _ptr(qz), _ptr(qnx), _ptr(qny), _ptr(qnz), len(qx), float(r),
                                           float(angle_threshold), _ptr(out)))
        return out

    def smooth_clusters(self, x, y, z, nx, ny, nz, tolerance, eps_angle, min_points):
        """extractEuclideanClustersSmooth (pfx_smooth_clusters): (labels (n,) int32, n_clusters).  A label
        is the point's cluster, numbered by the clusters' lowest index, or -1."""
        x, y, z, nx, ny, nz = map(_f32, (x, y, z, nx, ny, nz))
        if not len(x) == len(y) == len(z) == len(nx) == len(ny) == len(nz):
            raise ValueError("smooth_clusters: one normal per point")
        labels, n_out = np.empty(len(x), np.int32), np.zeros(1, np.int64)
        self._check(self._lib.pfx_smooth_clusters(self.h, _ptr(x), _ptr(y), _ptr(z), _ptr(nx), _ptr(ny), _ptr(nz),
                                                  len(x), float(tolerance), float(eps_angle), int(min_points),
                                                  _ptr(labels), _ptr(n_out)))
        return labels, int(n_out[0])

    def cvfh(self, sx, sy, sz, snx, sny, snz, scurvature, indices=None, params=None, cap=None):
        """CVFHEstimation (pfx_cvfh) over the surface points `indices` (None: all): Cvfh(rows, centroids,
        dominant_normals, labels), one row per smooth cluster, or one row when there is none.  cap (None:
        as many as can arise): fewer than the rows is PFX_ERR_CAPACITY."""
        params = params or cvfh_params()
        sx, sy, sz, snx, sny, snz, scurvature = map(_f32, (sx, sy, sz, snx, sny, snz, scurvature))
        if not len(sx) == len(sy) == len(sz) == len(snx) == len(sny) == len(snz) == len(scurvature):
            raise ValueError("cvfh: one normal and one curvature per surface point")
        idx = None if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
        n_idx = len(sx) if idx is None else len(idx)
        if cap is None:
            cap = max(1, n_idx // max(1, params.min_points))
        rows, cen, dn = (np.empty((cap, w), np.float32) for w in (308, 3, 3))
        labels, n_out = np.empty(n_idx, np.int32), np.zeros(1, np.int64)
        try:
            self._check(self._lib.pfx_cvfh(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny), _ptr(snz),
                                           _ptr(scurvature), len(sx), _ptr(idx), n_idx, ctypes.byref(params),
                                           _ptr(rows), cap, _ptr(n_out), _ptr(cen), _ptr(dn), _ptr(labels)))
        except N.PfxError as e:
            e.required = int(n_out[0])  # (PFX_ERR_CAPACITY: the rows the call needs)
            raise
        m = int(n_out[0])
        return Cvfh(rows[:m].copy(), cen[:m].copy(), dn[:m].copy(), labels)

    def range_image_planar(self, x, y, z, cam=None):
        cam = cam or camera()
        x, y, z = map(_f32, (x, y, z))
        out = np.empty((cam.height, cam.width, 4), dtype=np.float32)
        self._check(self._lib.pfx_range_image_planar(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), ctypes.byref(cam),
                                                     _ptr(out)))
        return out

    def narf_keypoints(self, x, y, z, params=None, cam=None, cap=1 << 20):
        cam = cam or camera()
        params = params or narf_params()
        x, y, z = map(_f32, (x, y, z))
        out = np.empty(cap, dtype=np.int32)
        nout = ctypes.c_int64()
        self._check(self._lib.pfx_narf_keypoints(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), ctypes.byref(cam),
                                                 ctypes.byref(params), _ptr(out), cap, ctypes.byref(nout)))
        return out[: nout.value].copy()

    def narf_descriptors(self, x, y, z, pixel_idx, params=None, cam=None):
        """NarfDescriptor (pfx_narf_descriptors) at the pixels pixel_idx (y * width + x) of the cloud's
        planar range image: NarfDescriptors(desc, pose, keypoint).  An entry gives 0 to 5 rows (one or
        none without rotation invariance), in entry order."""
        cam = cam or camera()
        params = params or narf_desc_params()
        x, y, z = map(_f32, (x, y, z))
        pix = np.ascontiguousarray(pixel_idx, dtype=np.int32)
        cap = 5 * len(pix)
        desc, pose = np.empty((cap, 36), np.float32), np.empty((cap, 12), np.float32)
        key = np.empty(cap, np.int32)
        nout = ctypes.c_int64()
        self._check(self._lib.pfx_narf_descriptors(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), ctypes.byref(cam),
                                                   _ptr(pix), len(pix), ctypes.byref(params), _ptr(desc), _ptr(pose),
                                                   _ptr(key), cap, ctypes.byref(nout)))
        m = nout.value
        return NarfDescriptors(desc[:m].copy(), pose[:m].copy(), key[:m].copy())

    def point_indices(self, x, y, z, kx, ky, kz, tol=1e-4):
        """Tools::getIndices (pfx_point_indices): for each keypoint in order, every cloud index ascending
        within tol of it on all three axes; (m,) int32."""
        x, y, z, kx, ky, kz = map(_f32, (x, y, z, kx, ky, kz))
        cap = max(64, 2 * len(kx))
        while True:
            out = np.empty(cap, np.int32)
            nout = ctypes.c_int64()
            code = self._lib.pfx_point_indices(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), _ptr(kx), _ptr(ky), _ptr(kz),
                                               len(kx), float(tol), _ptr(out), cap, ctypes.byref(nout))
            if code != N.PFX_ERR_CAPACITY:
                self._check(code)
                return out[: nout.value].copy()
            cap = nout.value  # the size the call asked for

    def narf_debug_image(self, which, width=640, height=480):
        dt = np.uint32 if which == "border_traits" else np.float32
        out = np.empty(width * height, dtype=dt)
        self._check(self._lib.pfx_narf_debug_image(self.h, which.encode(), _ptr(out), out.size))
        return out.reshape(height, width)

    def grid_debug(self, x, y, z, r, mode=0):
        """Test hook (pfx_grid_debug): the normal-radius grid of a cloud, built exactly (mode 0, leaves
        the bounds hint) or speculatively on that hint (mode 1, rebuilt exactly when its validation
        word is non-zero, as the callers do).  Returns a dict of perm, skeys, sp, cell_start, the
        exact cell mapping (ox, oy, oz, inv, nx, ny, nz, ncells), the raw validation `word`, the
        `builder` of the first build ("sort" / "count"), `rerun` and the counting builder's `cap`."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        info = np.zeros(8, dtype=np.int64)
        params = np.zeros(4, dtype=np.float64)
        self._check(self._lib.pfx_grid_debug(self.h, _ptr(x), _ptr(y), _ptr(z), n, float(r), int(mode), None, None,
                                             None, None, 0, _ptr(params), _ptr(info)))
        ncells = int(info[3])
        perm = np.empty(n, dtype=np.int32)
        skeys = np.empty(n, dtype=np.uint32)
        sp = np.empty((n, 4), dtype=np.float32)
        cell_start = np.empty(ncells + 2, dtype=np.int32)
        self._check(self._lib.pfx_grid_debug(self.h, None, None, None, n, float(r), -1, _ptr(perm), _ptr(skeys),
                                             _ptr(sp), _ptr(cell_start), cell_start.size, _ptr(params), _ptr(info)))
        return {"perm": perm, "skeys": skeys, "sp": sp, "cell_start": cell_start,
                "ox": float(params[0]), "oy": float(params[1]), "oz": float(params[2]), "inv": float(params[3]),
                "nx": int(info[0]), "ny": int(info[1]), "nz": int(info[2]), "ncells": ncells,
                "word": int(info[4]), "builder": "count" if info[5] else "sort", "rerun": bool(info[6]),
                "cap": int(info[7])}

    # ---- device (torch tensor) entry points, stream-ordered on the ctx stream ---------
    def normals_dev(self, x, y, z, r, nx, ny, nz, curv, viewpoint=(0.0, 0.0, 0.0)):
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r), _ptr(vp),
                                              _ptr(nx), _ptr(ny), _ptr(nz), _ptr(curv)))

    def knn_search_dev(self, x, y, z, qx, qy, qz, k, counts, idx, d2):
        """Device version: counts (nq,) int64, idx (nq, k) int32 and d2 (nq, k) float32 tensors."""
        nq, k = qx.numel(), int(k)
        if counts.numel() < nq or idx.numel() < nq * k or d2.numel() < nq * k:
            raise ValueError("knn_search_dev: an output holds fewer than nq rows of k")
        self._check(self._lib.pfx_knn_search_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), _ptr(qx), _ptr(qy),
                                                 _ptr(qz), nq, k, _ptr(counts), _ptr(idx), _ptr(d2)))

    def normals_knn_dev(self, x, y, z, k, nx, ny, nz, curv, viewpoint=(0.0, 0.0, 0.0)):
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals_knn_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), int(k), _ptr(vp),
                                                  _ptr(nx), _ptr(ny), _ptr(nz), _ptr(curv)))

    def normals_fast_dev(self, x, y, z, r, nx, ny, nz, curv, viewpoint=(0.0, 0.0, 0.0)):
        vp = _f32(viewpoint)
        self._check(self._lib.pfx_normals_fast_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r), _ptr(vp),
                                                   _ptr(nx), _ptr(ny), _ptr(nz), _ptr(curv)))

    def fpfh_dev(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, out, same_as_surface=False, after_normals=False):
        """after_normals: the caller vouches that (sx, sy, sz) still hold the cloud of this context's
        last normals_dev (Features::compute's sequence) -> pfx_fpfh_after_normals_dev, which may
        reuse that estimation's neighbour lists."""
        fn = self._lib.pfx_fpfh_after_normals_dev if after_normals else self._lib.pfx_fpfh_dev
        self._check(fn(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz), sx.numel(), _ptr(qx),
                       _ptr(qy), _ptr(qz), qx.numel(), 1 if same_as_surface else 0, float(r), _ptr(out)))

    def normals_lists_dev(self, x, y, z, r, nx, ny, nz, curv):
        """Phase 1 of normals_dev: neighbour lists of every point (kept in this context)."""
        self._check(self._lib.pfx_normals_lists_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r), _ptr(nx),
                                                    _ptr(ny), _ptr(nz), _ptr(curv)))

    def normals_launch_dev(self, x, y, z, r, nx, ny, nz, curv, viewpoint=(0.0, 0.0, 0.0)):
        """normals_dev with no host round trip (pfx_normals_launch_dev); normals_finish_dev must
        follow before the outputs are trusted."""
        vp = (ctypes.c_float * 3)(*viewpoint)
        self._check(self._lib.pfx_normals_launch_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r), vp,
                                                     _ptr(nx), _ptr(ny), _ptr(nz), _ptr(curv)))

    def normals_grid_launch_dev(self, x, y, z, r):
        """Queue the spatial grid of the next normals_launch_dev on this context's stream now
        (pfx_normals_grid_launch_dev) so it runs ahead of work issued later on other streams;
        the launch for the same cloud and radius then starts at its list kernels."""
        self._check(self._lib.pfx_normals_grid_launch_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r)))

    def normals_gate_dev(self, event):
        """The next normals launch on this context waits for `event` (a recorded torch.cuda.Event)
        between its grid build and its list kernels (pfx_normals_gate_dev); None clears it."""
        self._check(self._lib.pfx_normals_gate_dev(self.h, None if event is None else event.cuda_event))

    def normals_finish_dev(self) -> bool:
        """Validates the launched estimation; True when it had to be rerun (consumers of its
        outputs queued in between must run again)."""
        rerun = ctypes.c_int32(0)
        self._check(self._lib.pfx_normals_finish_dev(self.h, ctypes.byref(rerun)))
        return bool(rerun.value)

    def normals_prepare_dev(self, x, y, z, r):
        """The grid of the next normals_subset_dev calls on this cloud, built ahead (coordinates only)."""
        self._check(self._lib.pfx_normals_prepare_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r)))

    def normals_subset_dev(self, x, y, z, r, mask, want, nx, ny, nz, curv, viewpoint=(0.0, 0.0, 0.0)):
        """NormalEstimationOMP for the points with (mask != 0) == want only (uint8 device mask by
        point); the other output entries are left untouched."""
        vp = (ctypes.c_float * 3)(*viewpoint)
        self._check(self._lib.pfx_normals_subset_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), float(r),
                                                     _ptr(mask), int(want), vp, _ptr(nx), _ptr(ny), _ptr(nz),
                                                     _ptr(curv)))

    def normals_chains_dev(self, lists_ctx, nx, ny, nz, curv, mask=None, want=1, viewpoint=(0.0, 0.0, 0.0)):
        """Phase 2 on this context's stream for the points with (mask != 0) == want (all if mask
        is None), from the lists held by `lists_ctx`."""
        vp = (ctypes.c_float * 3)(*viewpoint)
        self._check(self._lib.pfx_normals_chains_dev(self.h, lists_ctx.h, _ptr(mask), int(want), vp, _ptr(nx),
                                                     _ptr(ny), _ptr(nz), _ptr(curv)))

    def fpfh_support_mask_dev(self, sx, sy, sz, qx, qy, qz, r, mask):
        """mask[i] = 1 for the surface points FPFH reads normals of (within r of a query)."""
        self._check(self._lib.pfx_fpfh_support_mask_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx),
                                                         _ptr(qy), _ptr(qz), qx.numel(), float(r), _ptr(mask)))

    def fpfh_support_ball_dev(self, sx, sy, sz, qx, qy, qz, r, mask):
        """Conservative support: mask[i] = 1 for the surface points within 2r of a query."""
        self._check(self._lib.pfx_fpfh_support_ball_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx),
                                                         _ptr(qy), _ptr(qz), qx.numel(), float(r), _ptr(mask)))

    def fpfh_prepare_queries_dev(self, sx, sy, sz, qx, qy, qz, r):
        """The next fpfh_dev's SPFH point set for these queries (same tensors), found ahead."""
        self._check(self._lib.pfx_fpfh_prepare_queries_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(),
                                                            _ptr(qx), _ptr(qy), _ptr(qz), qx.numel(), float(r)))

    def fpfh_prepare_dev(self, sx, sy, sz, r):
        """Build the FPFH search-surface index ahead of fpfh_dev (see pfx_fpfh_prepare_dev)."""
        self._check(self._lib.pfx_fpfh_prepare_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), float(r)))

    def shot_dev(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, desc, rf):
        self._check(self._lib.pfx_shot_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz),
                                           sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), qx.numel(), float(r),
                                           _ptr(desc), _ptr(rf)))

    def shot_color_dev(self, sx, sy, sz, nx, ny, nz, srgb, qx, qy, qz, qrgb, r, desc, rf):
        """pfx_shot_color_dev: srgb / qrgb are 32-bit integer device tensors of packed 0x00RRGGBB words,
        desc (nq, 1344) and rf (nq, 9) float32 device tensors."""
        if srgb.element_size() != 4 or qrgb.element_size() != 4:
            raise ValueError("shot_color_dev: the packed colours must be 32-bit words")
        if srgb.numel() != sx.numel() or qrgb.numel() != qx.numel():
            raise ValueError("shot_color_dev: one packed colour per surface point and per query")
        self._check(self._lib.pfx_shot_color_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz),
                                                 _ptr(srgb), sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qrgb),
                                                 qx.numel(), float(r), _ptr(desc), _ptr(rf)))

    def pfh_dev(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, out):
        """pfx_pfh_dev: out is an (nq, 125) float32 device tensor; no host synchronisation (a
        neighbourhood beyond capacity is reported by the next synchronize())."""
        self._check(self._lib.pfx_pfh_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny), _ptr(nz),
                                          sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), qx.numel(), float(r),
                                          _ptr(out)))

    def spin_image_dev(self, sx, sy, sz, qx, qy, qz, qnx, qny, qnz, r, out, image_width=8, support_angle_cos=0.0,
                       min_pts_neighb=0, surface_normals=None, raw=None, sums=None):
        """pfx_spin_image_dev: out is an (nq, S) float32 device tensor, raw / sums optional float64
        device tensors; no host synchronisation (too few neighbours, a cosine out of range or a
        neighbourhood beyond capacity is reported by the next synchronize())."""
        sn = (None, None, None) if surface_normals is None else tuple(surface_normals)
        p = spin_params(image_width, support_angle_cos, min_pts_neighb)
        self._check(self._lib.pfx_spin_image_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(sn[0]), _ptr(sn[1]),
                                                 _ptr(sn[2]), sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qnx),
                                                 _ptr(qny), _ptr(qnz), qx.numel(), float(r), ctypes.byref(p),
                                                 _ptr(out), _ptr(raw), _ptr(sums)))

    def intensity_gradient_dev(self, sx, sy, sz, si, qx, qy, qz, qnx, qny, qnz, r, out, same_as_surface=False):
        """pfx_intensity_gradient_dev: out is an (nq, 3) float32 device tensor.  same_as_surface=True
        needs qx, qy, qz to be sx, sy, sz themselves and reads the list sizes back inside the call;
        otherwise no host synchronisation (a neighbourhood beyond capacity is reported by the next
        synchronize())."""
        self._check(self._lib.pfx_intensity_gradient_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(si), sx.numel(),
                                                         _ptr(qx), _ptr(qy), _ptr(qz), _ptr(qnx), _ptr(qny),
                                                         _ptr(qnz), qx.numel(), 1 if same_as_surface else 0,
                                                         float(r), _ptr(out)))

    def rift_dev(self, sx, sy, sz, sgx, sgy, sgz, cx, cy, cz, r, out, nr_distance_bins=4, nr_gradient_bins=8):
        """pfx_rift_dev: out is an (nq, D G) float32 device tensor; no host synchronisation (a
        neighbourhood beyond capacity is reported by the next synchronize())."""
        self._check(self._lib.pfx_rift_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(sgx), _ptr(sgy), _ptr(sgz),
                                           sx.numel(), _ptr(cx), _ptr(cy), _ptr(cz), cx.numel(), float(r),
                                           int(nr_distance_bins), int(nr_gradient_bins), _ptr(out)))

    def intensity_spin_dev(self, sx, sy, sz, si, cx, cy, cz, r, out, nr_distance_bins=4, nr_intensity_bins=5,
                           sigma=1.0):
        """pfx_intensity_spin_dev: out is an (nq, D I) float32 device tensor; no host synchronisation
        (a neighbourhood beyond capacity is reported by the next synchronize())."""
        self._check(self._lib.pfx_intensity_spin_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(si), sx.numel(),
                                                     _ptr(cx), _ptr(cy), _ptr(cz), cx.numel(), float(r),
                                                     int(nr_distance_bins), int(nr_intensity_bins), float(sigma),
                                                     _ptr(out)))

    def moment_invariants_dev(self, sx, sy, sz, qx, qy, qz, r, out):
        """pfx_moment_invariants_dev: out is an (nq, 3) float32 device tensor; no host synchronisation
        (a neighbourhood beyond capacity is reported by the next synchronize())."""
        self._check(self._lib.pfx_moment_invariants_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx),
                                                        _ptr(qy), _ptr(qz), qx.numel(), float(r), _ptr(out)))

    def principal_curvatures_dev(self, sx, sy, sz, snx, sny, snz, qx, qy, qz, qnx, qny, qnz, r, out):
        """pfx_principal_curvatures_dev: out is an (nq, 5) float32 device tensor; no host
        synchronisation (a neighbourhood beyond capacity is reported by the next synchronize())."""
        self._check(self._lib.pfx_principal_curvatures_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny),
                                                           _ptr(snz), sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz),
                                                           _ptr(qnx), _ptr(qny), _ptr(qnz), qx.numel(), float(r),
                                                           _ptr(out)))

    def shape_context_dev(self, sx, sy, sz, nx, ny, nz, qx, qy, qz, r, desc, rf, min_radius=None,
                          point_density_radius=None, rnd=None):
        """pfx_shape_context_dev: desc (nq, 1980) and rf (nq, 9) float32 device tensors, rnd an optional
        (3 nq) float32 device tensor; a neighbourhood beyond capacity is reported by the next
        synchronize()."""
        rmin = float(r) / 10 if min_radius is None else float(min_radius)
        rho = float(r) / 5 if point_density_radius is None else float(point_density_radius)
        self._check(self._lib.pfx_shape_context_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(nx), _ptr(ny),
                                                    _ptr(nz), sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), qx.numel(),
                                                    float(r), rmin, rho, _ptr(rnd), _ptr(desc), _ptr(rf)))

    def usc_dev(self, sx, sy, sz, qx, qy, qz, frames, r, desc, rf, min_radius=None, point_density_radius=None):
        """pfx_usc_dev: frames (nq, 9), desc (nq, 1980) and rf (nq, 9) float32 device tensors; a
        neighbourhood beyond capacity is reported by the next synchronize()."""
        rmin = float(r) / 10 if min_radius is None else float(min_radius)
        rho = float(r) / 5 if point_density_radius is None else float(point_density_radius)
        self._check(self._lib.pfx_usc_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx), _ptr(qy),
                                          _ptr(qz), _ptr(frames), qx.numel(), float(r), rmin, rho, _ptr(desc),
                                          _ptr(rf)))

    def shot_lrf_dev(self, sx, sy, sz, qx, qy, qz, r, rf):
        """pfx_shot_lrf_dev: rf is an (nq, 9) float32 device tensor; a neighbourhood beyond capacity is
        reported by the next synchronize()."""
        self._check(self._lib.pfx_shot_lrf_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx), _ptr(qy),
                                               _ptr(qz), qx.numel(), float(r), _ptr(rf)))

    def board_lrf_dev(self, sx, sy, sz, snx, sny, snz, qx, qy, qz, r, rf, tangent_radius=0.0, margin_thresh=0.85,
                      find_holes=False):
        """pfx_board_lrf_dev: rf is an (nq, 9) float32 device tensor; no host synchronisation (a
        neighbourhood beyond capacity is reported by the next synchronize())."""
        p = board_params(tangent_radius, margin_thresh, find_holes)
        self._check(self._lib.pfx_board_lrf_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny), _ptr(snz),
                                                sx.numel(), _ptr(qx), _ptr(qy), _ptr(qz), qx.numel(), float(r),
                                                ctypes.byref(p), _ptr(rf)))

    def boundary_dev(self, sx, sy, sz, qx, qy, qz, qnx, qny, qnz, r, out, angle_threshold=math.pi / 2):
        """pfx_boundary_dev: out is an (nq,) uint8 device tensor; no host synchronisation (the statistics
        come with the next synchronize(); nothing else is reported late)."""
        self._check(self._lib.pfx_boundary_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), sx.numel(), _ptr(qx), _ptr(qy),
                                               _ptr(qz), _ptr(qnx), _ptr(qny), _ptr(qnz), qx.numel(), float(r),
                                               float(angle_threshold), _ptr(out)))

    def smooth_clusters_dev(self, x, y, z, nx, ny, nz, tolerance, eps_angle, min_points, labels, n_clusters):
        """pfx_smooth_clusters_dev: labels an (n,) int32 and n_clusters a (1,) int64 device tensor.  Waits
        on the host for the components to be complete; the statistics are set when it returns."""
        self._check(self._lib.pfx_smooth_clusters_dev(self.h, _ptr(x), _ptr(y), _ptr(z), _ptr(nx), _ptr(ny), _ptr(nz),
                                                      x.numel(), float(tolerance), float(eps_angle), int(min_points),
                                                      _ptr(labels), _ptr(n_clusters)))

    def cvfh_dev(self, sx, sy, sz, snx, sny, snz, scurvature, indices, out, n_rows, params=None, centroids=None,
                 dominant_normals=None, labels=None):
        """pfx_cvfh_dev: out a (cap, 308) float32, n_rows a (1,) int64 device tensor; indices an int32
        device tensor or None; centroids / dominant_normals (cap, 3) and labels (n_indices,) int32 or
        None.  Waits on the host for the cluster count; more rows than cap raises PFX_ERR_CAPACITY with
        the required count in n_rows."""
        params = params or cvfh_params()
        n_idx = sx.numel() if indices is None else indices.numel()
        self._check(self._lib.pfx_cvfh_dev(self.h, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(snx), _ptr(sny), _ptr(snz),
                                           _ptr(scurvature), sx.numel(), _ptr(indices), n_idx, ctypes.byref(params),
                                           _ptr(out), out.shape[0], _ptr(n_rows), _ptr(centroids),
                                           _ptr(dominant_normals), _ptr(labels)))

    def narf_keypoints_dev(self, x, y, z, params=None, cam=None, cap=1 << 20):
        cam = cam or camera()
        params = params or narf_params()
        out = np.empty(cap, dtype=np.int32)
        nout = ctypes.c_int64()
        self._check(self._lib.pfx_narf_keypoints_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(),
                                                     ctypes.byref(cam), ctypes.byref(params), _ptr(out), cap,
                                                     ctypes.byref(nout)))
        return out[: nout.value].copy()

    def narf_descriptors_dev(self, x, y, z, pixel_idx, desc, pose, row_key, params=None, cam=None):
        """pfx_narf_descriptors_dev: pixel_idx an int32 device tensor, desc (cap, 36) / pose (cap, 12)
        float32 and row_key (cap,) int32 device tensors.  Returns the (1,) int64 device tensor of the
        row count (the full count, also when it exceeds cap and only cap rows were written); no host
        synchronisation, the statistics come with the next synchronize()."""
        import torch
        cam = cam or camera()
        params = params or narf_desc_params()
        cap = min(desc.shape[0], pose.shape[0], row_key.shape[0])
        count = torch.empty(1, dtype=torch.int64, device=x.device)  # (always written by the call, on its stream)
        self._check(self._lib.pfx_narf_descriptors_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), ctypes.byref(cam),
                                                       _ptr(pixel_idx), pixel_idx.numel(), ctypes.byref(params),
                                                       _ptr(desc), _ptr(pose), _ptr(row_key), cap, _ptr(count)))
        return count

    def point_indices_dev(self, x, y, z, kx, ky, kz, out, tol=1e-4):
        """pfx_point_indices_dev: out an int32 device tensor; returns the (1,) int64 device tensor of the
        full count (out holds the first out.numel() indices).  No host synchronisation."""
        import torch
        count = torch.empty(1, dtype=torch.int64, device=x.device)  # (always written by the call, on its stream)
        self._check(self._lib.pfx_point_indices_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), _ptr(kx), _ptr(ky),
                                                    _ptr(kz), kx.numel(), float(tol), _ptr(out), out.numel(),
                                                    _ptr(count)))
        return count

    def gather_points_dev(self, x, y, z, idx_np, kx, ky, kz):
        idx = np.ascontiguousarray(idx_np, dtype=np.int32)
        nout = ctypes.c_int64()
        self._check(self._lib.pfx_gather_points_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), _ptr(idx),
                                                    len(idx), _ptr(kx), _ptr(ky), _ptr(kz),
                                                    min(kx.numel(), ky.numel(), kz.numel()), ctypes.byref(nout)))
        return nout.value

    # ---- PCD input: pcl::io::loadPCDFile<PointXYZRGB> (evaluation.cpp:226-235) -------------
    def pcd_load_xyz_dev(self, path, x, y, z):
        """x, y, z (float32 device tensors of >= POINTS elements) <- the file's points; returns
        (n, header)."""
        n = ctypes.c_int64()
        h = N.PcdHeader()
        self._check(self._lib.pfx_pcd_load_xyz_dev(self.h, str(path).encode(), _ptr(x), _ptr(y), _ptr(z), x.numel(),
                                                   ctypes.byref(n), ctypes.byref(h)))
        return n.value, h

    # ---- descriptor matching: Features<T>::findCorrespondences / getCorrespondences ----------
    def correspondences(self, src, tgt):
        """features.h:224-253: mutual nearest neighbours (index_query, index_match) in source
        order; src / tgt are (n, D) float32 descriptor matrices (host)."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        tgt = np.ascontiguousarray(tgt, dtype=np.float32)
        ns, d = src.shape
        q = np.empty(max(ns, 1), np.int32)
        m = np.empty(max(ns, 1), np.int32)
        n = ctypes.c_int64()
        self._check(self._lib.pfx_correspondences(self.h, _ptr(src), ns, d, _ptr(tgt), tgt.shape[0], tgt.shape[1], d,
                                                  _ptr(q), _ptr(m), ns, ctypes.byref(n)))
        return q[: n.value].copy(), m[: n.value].copy()

    def nearest_descriptors(self, src, tgt):
        """features.h:255-273 (one direction, host arrays): nearest target row of every source row
        (-1: non-finite row / empty target) and its L2_Simple squared distance."""
        src = np.ascontiguousarray(src, dtype=np.float32)
        tgt = np.ascontiguousarray(tgt, dtype=np.float32)
        ns, d = src.shape
        idx = np.empty(max(ns, 1), np.int32)
        dist = np.empty(max(ns, 1), np.float32)
        self._check(self._lib.pfx_nearest_descriptors(self.h, _ptr(src), ns, d, _ptr(tgt), tgt.shape[0], tgt.shape[1],
                                                      d, _ptr(idx), _ptr(dist)))
        return idx[:ns].copy(), dist[:ns].copy()

    def nearest_descriptors_dev(self, src, tgt, s2t, s2t_dist=None, t2s=None, t2s_dist=None, dim=None):
        """features.h:255-273 in both directions: (n, stride) device tensors, `dim` leading floats
        of each row compared (default: the whole row)."""
        dim = dim or src.shape[1]
        self._check(self._lib.pfx_nearest_descriptors_dev(self.h, _ptr(src), src.shape[0], src.stride(0),
                                                          _ptr(tgt), tgt.shape[0], tgt.stride(0), dim, _ptr(s2t),
                                                          _ptr(s2t_dist), _ptr(t2s), _ptr(t2s_dist)))

    def correspondences_dev(self, src, tgt, query, match, dim=None):
        """Device version of correspondences(); returns the number of pairs written."""
        dim = dim or src.shape[1]
        n = ctypes.c_int64()
        self._check(self._lib.pfx_correspondences_dev(self.h, _ptr(src), src.shape[0], src.stride(0), _ptr(tgt),
                                                      tgt.shape[0], tgt.stride(0), dim, _ptr(query), _ptr(match),
                                                      query.numel(), ctypes.byref(n)))
        return n.value


    # ---- active-list keypoints ------------------------------------------
    def cloud_resolution(self, x, y, z):
        """Keypoints::computeCloudResolution (keypoints.h:401-428), host arrays."""
        x, y, z = map(_f32, (x, y, z))
        out = ctypes.c_double()
        self._check(self._lib.pfx_cloud_resolution(self.h, _ptr(x), _ptr(y), _ptr(z), len(x), ctypes.byref(out)))
        return out.value

    def cloud_resolution_dev(self, x, y, z):
        """Keypoints::computeCloudResolution on device arrays (the value comes back to the host,
        as the reference's return value)."""
        out = ctypes.c_double()
        self._check(self._lib.pfx_cloud_resolution_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(),
                                                       ctypes.byref(out)))
        return out.value

    def iss_keypoints(self, x, y, z, salient_radius, non_max_radius, min_neighbors=5, threshold21=0.975,
                      threshold32=0.975, return_third=False):
        """ISSKeypoint3D::compute (keypoints.h:177-189), host arrays: keypoint indices ascending
        (and the per-point third eigenvalue map)."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        idx = np.empty(max(n, 1), np.int32)
        third = np.empty(max(n, 1), np.float64) if return_third else None
        k = ctypes.c_int64()
        self._check(self._lib.pfx_iss_keypoints(self.h, _ptr(x), _ptr(y), _ptr(z), n, salient_radius, non_max_radius,
                                                min_neighbors, threshold21, threshold32, _ptr(idx), len(idx),
                                                ctypes.byref(k), _ptr(third)))
        out = idx[: k.value].copy()
        return (out, third[:n].copy()) if return_third else out

    def iss_keypoints_dev(self, x, y, z, salient_radius, non_max_radius, idx, min_neighbors=5, threshold21=0.975,
                          threshold32=0.975, third=None):
        """Device version: indices into `idx` (int32 tensor), returns their number."""
        k = ctypes.c_int64()
        self._check(self._lib.pfx_iss_keypoints_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), salient_radius,
                                                    non_max_radius, min_neighbors, threshold21, threshold32,
                                                    _ptr(idx), idx.numel(), ctypes.byref(k), _ptr(third)))
        return k.value

    def uniform_sampling(self, x, y, z, radius, return_leaf=False):
        """UniformSampling::compute (keypoints.h:274-290), host arrays: one keypoint per occupied
        voxel of edge `radius`, int32 cloud indices in ascending leaf index (and the leaf indices)."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        idx = np.empty(max(n, 1), np.int32)
        leaf = np.empty(max(n, 1), np.int32) if return_leaf else None
        k = ctypes.c_int64()
        self._check(self._lib.pfx_uniform_sampling(self.h, _ptr(x), _ptr(y), _ptr(z), n, radius, _ptr(idx), len(idx),
                                                   ctypes.byref(k), _ptr(leaf)))
        out = idx[: k.value].copy()
        return (out, leaf[: k.value].copy()) if return_leaf else out

    def uniform_sampling_dev(self, x, y, z, radius, idx, leaf=None):
        """Device version: indices into `idx` (int32 tensor; its size is the capacity) and the leaf
        indices into `leaf` (int32 tensor of at least that size, optional); returns their number."""
        if leaf is not None and leaf.numel() < idx.numel():
            raise ValueError("uniform_sampling_dev: leaf holds fewer elements than idx")
        k = ctypes.c_int64()
        self._check(self._lib.pfx_uniform_sampling_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), radius,
                                                       _ptr(idx), idx.numel(), ctypes.byref(k), _ptr(leaf)))
        return k.value

    def harris3d_keypoints(self, x, y, z, radius=0.01, threshold=1e-6, refine=True, non_max=True, details=False):
        """HarrisKeypoint3D + getKeypointsCloud (keypoints.h:150-162, 365-395), host arrays: the
        snapped cloud indices in corner order (details: and the per-point response and the
        refined corners)."""
        x, y, z = map(_f32, (x, y, z))
        n = len(x)
        cap = max(n, 1)
        idx = np.empty(cap, np.int32)
        resp = np.empty(cap, np.float32) if details else None
        corners = np.empty((cap, 3), np.float32) if details else None
        k, nc = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.pfx_harris3d_keypoints(self.h, _ptr(x), _ptr(y), _ptr(z), n, radius, threshold,
                                                     1 if non_max else 0, 1 if refine else 0, _ptr(idx), cap,
                                                     ctypes.byref(k), _ptr(resp), _ptr(corners), ctypes.byref(nc),
                                                     None))
        out = idx[: k.value].copy()
        return (out, resp[:n].copy(), corners[: nc.value].copy()) if details else out

    def harris3d_keypoints_dev(self, x, y, z, idx, radius=0.01, threshold=1e-6, refine=True, response=None,
                               corners=None):
        """Device version: snapped indices into `idx` (int32 tensor); returns (count, corners)."""
        k, nc = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.pfx_harris3d_keypoints_dev(self.h, _ptr(x), _ptr(y), _ptr(z), x.numel(), radius,
                                                         threshold, 1, 1 if refine else 0, _ptr(idx), idx.numel(),
                                                         ctypes.byref(k), _ptr(response), _ptr(corners),
                                                         ctypes.byref(nc), None))
        return k.value, nc.value

    def harris6d_keypoints(self, x, y, z, rgb, radius=0.01, threshold=1e-6, refine=True, non_max=True,
                           details=False):
        """HarrisKeypoint6D + getKeypointsCloud (keypoints.h:164-176, 365-395), host arrays (rgb:
        packed 0x00RRGGBB per point): the snapped cloud indices in corner order (details: and the
        per-point response, the refined corners and the normalised intensity gradients (n, 3))."""
        x, y, z = map(_f32, (x, y, z))
        rgb = np.ascontiguousarray(rgb, dtype=np.uint32)
        n = len(x)
        if len(rgb) != n:
            raise ValueError("harris6d: one rgb word per point")
        cap = max(n, 1)
        idx = np.empty(cap, np.int32)
        resp = np.empty(cap, np.float32) if details else None
        corners = np.empty((cap, 3), np.float32) if details else None
        grad = np.empty((cap, 3), np.float32) if details else None
        k, nc = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.pfx_harris6d_keypoints(self.h, _ptr(x), _ptr(y), _ptr(z), _ptr(rgb), n, radius,
                                                     threshold, 1 if non_max else 0, 1 if refine else 0, _ptr(idx),
                                                     cap, ctypes.byref(k), _ptr(resp), _ptr(corners), ctypes.byref(nc),
                                                     _ptr(grad), None))
        out = idx[: k.value].copy()
        return (out, resp[:n].copy(), corners[: nc.value].copy(), grad[:n].copy()) if details else out

    def harris6d_keypoints_dev(self, x, y, z, rgb, idx, radius=0.01, threshold=1e-6, refine=True, response=None,
                               corners=None, grad=None):
        """Device version (rgb: int32/uint32 tensor of packed colours): snapped indices into `idx`
        (int32 tensor); returns (count, corners)."""
        k, nc = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.pfx_harris6d_keypoints_dev(self.h, _ptr(x), _ptr(y), _ptr(z), _ptr(rgb), x.numel(),
                                                         radius, threshold, 1, 1 if refine else 0, _ptr(idx),
                                                         idx.numel(), ctypes.byref(k), _ptr(response), _ptr(corners),
                                                         ctypes.byref(nc), _ptr(grad), None))
        return k.value, nc.value

    # ---- RANSAC correspondence rejection -----------------------------------
    def ransac_rejector(self, src, tgt, query, match, threshold=0.015, max_iterations=1000):
        """Features::filterCorrespondences (features.h:282-297): (kept correspondence positions in
        input order, best 4x4 transformation).  src / tgt: (n, 3) keypoint clouds (host)."""
        src = np.ascontiguousarray(src, np.float32)
        tgt = np.ascontiguousarray(tgt, np.float32)
        sx, sy, sz = (np.ascontiguousarray(src[:, i]) for i in range(3))
        tx, ty, tz = (np.ascontiguousarray(tgt[:, i]) for i in range(3))
        query = np.ascontiguousarray(query, np.int32)
        match = np.ascontiguousarray(match, np.int32)
        n = len(query)
        keep = np.empty(max(n, 1), np.int32)
        T = np.empty(16, np.float32)
        nk = ctypes.c_int64()
        self._check(self._lib.pfx_ransac_rejector(self.h, _ptr(sx), _ptr(sy), _ptr(sz), len(sx), _ptr(tx), _ptr(ty),
                                                  _ptr(tz), len(tx), _ptr(query), _ptr(match), n, threshold,
                                                  max_iterations, _ptr(keep), ctypes.byref(nk), _ptr(T)))
        return keep[: nk.value].copy(), T.reshape(4, 4)

    # ---- ICP alignment (evaluation.cpp:863-885) --------------------------------------------
    def _icp_call(self, fn, src, tgt, ns, nt, params, guess, aligned):
        params = params or icp_params()
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(16)
        T = np.empty(16, np.float32)
        fit = ctypes.c_double()
        conv, it, state = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        al = aligned if aligned is not None else (None, None, None)
        self._check(fn(self.h, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]), ns, _ptr(tgt[0]), _ptr(tgt[1]),
                       _ptr(tgt[2]), nt, ctypes.byref(params), _ptr(g), _ptr(T), ctypes.byref(fit), ctypes.byref(conv),
                       ctypes.byref(it), ctypes.byref(state), _ptr(al[0]), _ptr(al[1]), _ptr(al[2])))
        return IcpResult(T.reshape(4, 4), fit.value, bool(conv.value), it.value, state.value, aligned)

    def icp(self, sx, sy, sz, tx, ty, tz, params=None, guess=None, aligned=True):
        """IterativeClosestPoint::align (pfx_icp) of the source cloud onto the target cloud (host
        arrays): IcpResult(transformation 4x4, fitness score, converged, iterations, state, aligned
        source cloud).  params: icp_params(...); guess: 4x4 or None."""
        src = [_f32(v) for v in (sx, sy, sz)]
        tgt = [_f32(v) for v in (tx, ty, tz)]
        al = tuple(np.empty(len(src[0]), np.float32) for _ in range(3)) if aligned else None
        return self._icp_call(self._lib.pfx_icp, src, tgt, len(src[0]), len(tgt[0]), params, guess, al)

    def icp_dev(self, sx, sy, sz, tx, ty, tz, params=None, guess=None, aligned=None):
        """pfx_icp_dev: float32 device tensors; aligned: None or three device tensors of the source's
        length.  Returns after the last iteration (the scalars are host values)."""
        return self._icp_call(self._lib.pfx_icp_dev, (sx, sy, sz), (tx, ty, tz), sx.numel(), tx.numel(), params,
                              guess, aligned)


def batch_plan(n_scans, n_devices, rows_per_scan=None):
    """pfx_batch_plan (host only, no device): (device_of_scan, slot_of_scan, row_offset[n_scans + 1])
    of the batch's round-robin deal and scan-order gather layout."""
    lib = N.lib()
    n_scans = int(n_scans)
    if n_scans < 0:  # (checked here: np.zeros(n_scans + 1) would raise a numpy error first)
        raise N.PfxError(N.PFX_ERR_INVALID, f"pfx_batch_plan: n_scans = {n_scans} < 0")
    rows = None if rows_per_scan is None else np.ascontiguousarray(rows_per_scan, np.int64).ravel()
    if rows is not None and len(rows) != n_scans:  # the C side reads rows_per_scan[0..n_scans)
        raise N.PfxError(N.PFX_ERR_INVALID,
                         f"pfx_batch_plan: rows_per_scan has {len(rows)} entries for {n_scans} scans")
    dev = np.zeros(max(n_scans, 1), np.int32)
    slot = np.zeros(max(n_scans, 1), np.int32)
    off = np.zeros(n_scans + 1, np.int64)
    st = lib.pfx_batch_plan(int(n_scans), int(n_devices), None if rows is None else _ptr(rows), _ptr(dev), _ptr(slot),
                            _ptr(off))
    if st != 0:
        raise N.PfxError(st, "pfx_batch_plan")
    return dev[:n_scans], slot[:n_scans], off


class Batch:
    """pfx_batch: the multi-GPU scan batch of one process; scan s on devices[s % G],
    results gathered on devices[0] over RCCL and returned in scan order."""

    def __init__(self, devices=(0,)):
        self._lib = N.lib()
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        h = ctypes.c_void_p()
        st = self._lib.pfx_batch_create(devs.ctypes.data_as(ctypes.c_void_p), len(devs), ctypes.byref(h))
        if st != 0:
            raise N.PfxError(st, "pfx_batch_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._lib.pfx_batch_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def narf_fpfh(self, clouds, normal_radius=0.05, feature_radius=0.08, params=None, cam=None, cap_rows=1 << 20):
        """clouds: list of (x, y, z) host arrays.  Returns [(K_s x 33 descriptors, K_s cloud indices)]."""
        cl = [tuple(_f32(a) for a in c) for c in clouds]
        ns = len(cl)
        arr = lambda i: (ctypes.c_void_p * max(ns, 1))(*[c[i].ctypes.data for c in cl])  # noqa: E731
        xs, ys, zs = arr(0), arr(1), arr(2)
        n = np.array([len(c[0]) for c in cl], np.int64)
        desc = np.empty((cap_rows, 33), np.float32)
        idx = np.empty(cap_rows, np.int32)
        rows = np.zeros(max(ns, 1), np.int64)
        st = self._lib.pfx_batch_narf_fpfh(self.h, ns, xs, ys, zs, _ptr(n), ctypes.byref(cam or camera()),
                                           ctypes.byref(params or narf_params(support_size=0.2)),
                                           float(normal_radius), float(feature_radius), _ptr(desc), _ptr(idx),
                                           cap_rows, _ptr(rows))
        if st != 0:
            raise N.PfxError(st, self._lib.pfx_batch_last_error(self.h).decode())
        out, o = [], 0
        for k in rows[:ns]:
            out.append((desc[o:o + k].copy(), idx[o:o + k].copy()))
            o += int(k)
        return out
