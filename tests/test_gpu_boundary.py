"""Boundary points (pfx_boundary and its _dev form, pfx_boundary.hip) against the CPU restatement
(tests/cpp/boundary_ref.cpp, pinned by tests/test_boundary_ref.py): every byte and the three
statistics.  The shapes are the smallest that reach every path of the kernel: the ring's drain of full
waves and its remainder, gaps within an ulp of the threshold between bins and across the +-pi cut,
angles at the ends of the bin range, more neighbours than any sorted family holds, partial workgroups
and the stride loop."""
import math

import numpy as np
import pytest

import boundary_cases as K
import boundary_ref as P

pytestmark = pytest.mark.gpu

PI = math.pi
PI_64 = float(np.float32(PI / 64))
FAR = (9.0e3, 9.0e3, 9.0e3)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("boundary_ref"))


def stats(ctx):
    return tuple(ctx.stat("boundary" + s) for s in ("_neighbors", "_kmax", "_flagged"))


def check(ctx, ref, s, q, n, r, t=PI / 2):
    """ctx.boundary == the restatement, bytes and statistics; returns the restatement's result."""
    want = P.flags(ref, *s, *q, *n, r, t)
    got = ctx.boundary(*s, *q, *n, r, t)
    assert got.dtype == np.uint8 and got.shape == want.flags.shape
    bad = np.flatnonzero(got != want.flags)
    assert len(bad) == 0, f"rows {bad[:8].tolist()} of {len(got)}: {got[bad[:8]].tolist()} for {want.flags[bad[:8]].tolist()}"
    assert stats(ctx) == (want.neighbors, want.kmax, want.flagged)
    return want


# ---- 1. a noisy plane with a hole ----

@pytest.fixture(scope="module")
def plane(ctx, ref):
    """4096 points of the unit square without a disc of radius 0.2, z noise 0.002, r = 0.05; the
    normals are Context.normals' at the same radius; the restatement's rows, once."""
    xyz = K.holed_plane()
    nrm = tuple(ctx.normals(*xyz, 0.05)[:3])
    return dict(xyz=xyz, normals=nrm, want=P.flags(ref, *xyz, *xyz, *nrm, 0.05))


def test_plane_with_a_hole(ctx, plane):
    xyz, nrm, want = plane["xyz"], plane["normals"], plane["want"]
    # (on the restatement alone) both outcomes hold a twentieth of the rows at least
    assert (want.flags == 1).mean() >= 0.05 and (want.flags == 0).mean() >= 0.05 and set(want.flags.tolist()) == {0, 1}
    assert 25 < want.k.mean() < 45
    got = ctx.boundary(*xyz, *xyz, *nrm, 0.05)
    assert np.array_equal(got, want.flags)
    assert stats(ctx) == (want.neighbors, want.kmax, want.flagged)
    # the flagged rows are the square's edges and the hole's rim
    x, y = xyz[0].astype(np.float64), xyz[1].astype(np.float64)
    edge = np.minimum.reduce([x, 1 - x, y, 1 - y, np.abs(np.hypot(x - 0.5, y - 0.5) - 0.2)])
    assert (want.flags[edge < 0.005] == 1).mean() > 0.9 and (want.flags[edge > 0.05] == 1).mean() < 0.02


@pytest.mark.parametrize("t", [PI_64, PI / 4, PI, 3.0, 6.2])
def test_plane_at_other_thresholds(ctx, ref, plane, t):
    check(ctx, ref, plane["xyz"], plane["xyz"], plane["normals"], 0.05, t)


@pytest.mark.parametrize("nq", [1, 3, 5])
def test_partial_workgroups(ctx, plane, nq):
    rows = np.arange(nq) * 37 + 11
    q, n = (tuple(v[rows] for v in a) for a in (plane["xyz"], plane["normals"]))
    assert np.array_equal(ctx.boundary(*plane["xyz"], *q, *n, 0.05), plane["want"].flags[rows])
    assert ctx.stat("boundary_neighbors") == int(plane["want"].k[rows].sum())


def test_more_queries_than_wave_slots(ctx, ref, plane):
    """10,000 queries: more than the 2048 workgroups of four; the rows past them come by stride."""
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 4096, 10000)
    q = tuple((v[rows] + rng.normal(0, 0.003, 10000)).astype(np.float32) for v in plane["xyz"])
    n = tuple(v[rows] for v in plane["normals"])
    want = check(ctx, ref, plane["xyz"], q, n, 0.05)
    assert 0.05 < want.flagged / 10000 < 0.95


def test_special_queries_and_surface_points(ctx, ref, plane):
    xyz, nrm = plane["xyz"], plane["normals"]
    # queries that are no surface points; one outside the grid; non-finite ones
    q = K.points((0.31, 0.305, 0.001), (0.5, 0.28, 0.0), (0.004, 0.5, 0.0), FAR, (-5.0, 0.5, 0.0),
                 (np.nan, 0.5, 0.0), (0.5, np.inf, 0.0), (0.5, 0.5, -np.inf))
    n = K.f32(np.zeros(8), np.zeros(8), np.ones(8))
    want = check(ctx, ref, xyz, q, n, 0.05)
    assert want.flags[3:].tolist() == [255] * 5 and set(want.flags[:3].tolist()) <= {0, 1} and want.k[:3].min() > 10
    # non-finite surface points among the finite ones are nobody's neighbours
    s = tuple(v.copy() for v in xyz)
    s[0][5::97] = np.nan
    s[1][7::89] = np.inf
    s[2][3::83] = -np.inf
    want2 = check(ctx, ref, s, xyz, nrm, 0.05)
    assert want2.neighbors < plane["want"].neighbors and want2.kmax <= plane["want"].kmax
    # unusable normals: 0, whatever the neighbours
    nb = tuple(v.copy() for v in nrm)
    nb[0][::5] = np.nan
    nb[1][1::5] = np.inf
    for v in nb:
        v[2::5] = 0.0
    want3 = check(ctx, ref, xyz, xyz, nb, 0.05)
    rows = np.arange(4096) % 5 < 3
    assert not want3.flags[rows].any() and np.array_equal(want3.flags[~rows], plane["want"].flags[~rows])


# ---- 2. the closed forms, the axes' branches ----

@pytest.mark.parametrize("name", sorted(K.NORMALS))
def test_rings_in_every_plane(ctx, ref, name):
    n = K.NORMALS[name]
    for m, flag in ((1, 0), (3, 1), (5, 0), (64, 0), (65, 0), (200, 0)):
        want = check(ctx, ref, *K.ring(K.even(m), n=n, centre=(0.3, -0.2, 0.1)), K.R)
        assert want.flags[0] == flag and want.k[0] == m + 1
    assert check(ctx, ref, *K.ring([], n=n, duplicates=3), K.R).flags[0] == 0          # cp = 0
    assert check(ctx, ref, *K.ring([1.0], n=n, duplicates=3), K.R, 6.2).flags[0] == 1  # cp = 1


def test_lattice(ctx, ref):
    xyz, nrm, rim = K.lattice()
    assert np.array_equal(check(ctx, ref, xyz, xyz, nrm, 0.025).flags, rim.astype(np.uint8))


# ---- 3. gaps at the threshold, angles at the bins' ends ----

def gap_cases(t, cut, steps=1000):
    """A centre and the 1024 angles of four per bin without an arc of about t, closed by a neighbour
    at either end (alpha and beta: the ring's only wide gap); beta moves in steps of a quarter of the
    threshold's ulp.  cut: the arc lies across +-pi, where the wrap term measures it.  Yields the
    cases."""
    a = -PI + (np.arange(1024) + 0.5) * (2 * PI / 1024)
    alpha = PI - t / 2 if cut else 0.002
    beta = alpha + t - (2 * PI if cut else 0.0)
    keep = a[(a > beta + 1e-3) & (a < alpha - 1e-3)] if cut else a[(a < alpha - 1e-3) | (a > beta + 1e-3)]
    s, q, n = K.ring(np.concatenate([keep, [alpha]]))
    step = float(np.spacing(np.float32(t))) / 4
    for j in range(-steps, steps + 1):
        end = K.ring([beta + j * step], with_centre=False)[0]
        yield tuple(np.append(v, e) for v, e in zip(s, end)), q, n


@pytest.mark.parametrize("t", [PI_64, PI / 2], ids=["pi/64", "pi/2"])
@pytest.mark.parametrize("cut", [False, True], ids=["inside", "cut"])
def test_gap_within_ulps_of_the_threshold(ctx, ref, t, cut):
    """The removed arc's width swept over the threshold: of the widths that moving one end of the arc
    by fractions of an ulp reaches, the three nearest gaps (in the restatement) on either side of the
    float32 threshold, the threshold itself included when it is reached.  The angles' own spacing
    decides how near that is: an angle beside pi, and so the wrap term, moves in steps of 2.4e-7."""
    tf = np.float32(t)
    found = {}
    for case in gap_cases(t, cut):
        g = P.flags(ref, *case[0], *case[1], *case[2], K.R, t).max_gap[0]
        found.setdefault(int(g.view(np.int32)) - int(tf.view(np.int32)), case)
    above, below = sorted(u for u in found if u > 0)[:3], sorted(u for u in found if u <= 0)[-3:]
    assert above and below, sorted(found)
    if not cut and t > 1:
        assert above[0] == 1 and below[-1] == 0, sorted(found)    # (the angles' spacing is the threshold's ulp)
    flags = {u: int(check(ctx, ref, *found[u], K.R, t).flags[0]) for u in below + above}
    print("gap - threshold in ulps -> flag:", flags)
    assert all(flags[u] == (1 if u > 0 else 0) for u in flags), flags     # both outcomes, at the strict >


def test_angles_at_the_ends_of_the_bin_range(ctx, ref):
    pts, r = K.bin_edge_angles()
    origin, up = K.points((0.0, 0.0, 0.0)), K.points((0.0, 0.0, 1.0))
    for names in (("+pi", "-pi"), ("+0", "-0"), ("+pi", "+0"), ("-pi", "-0"), tuple(pts)):
        s = K.points((0.0, 0.0, 0.0), *(pts[k] for k in names))
        got = {t: int(check(ctx, ref, s, origin, up, r, t).flags[0]) for t in (PI / 2, 3.0, 3.15, 6.2)}
        want = {("+pi", "-pi"): [1, 1, 1, 1], ("+0", "-0"): [1, 1, 1, 1]}.get(names, [1, 1, 0, 0])
        assert list(got.values()) == want, names


# ---- 4. no capacity ----

def test_twenty_thousand_neighbours(ctx, ref):
    """Two queries over 20,000 surface points within r: above the 16,384 keys at which the sorted
    families report PFX_ERR_CAPACITY.  A ball seen from its middle (no boundary) and from outside (a
    boundary: it fills a quarter of the horizon)."""
    rng = np.random.default_rng(8)
    p = rng.normal(size=(20000, 3))
    p *= (0.02 * rng.random(20000) ** (1 / 3) / np.linalg.norm(p, axis=1))[:, None]
    s = K.f32(p[:, 0], p[:, 1], p[:, 2])
    q = K.points((0.0, 0.0, 0.0), (0.028, 0.0, 0.0))
    n = K.points((0.0, 0.0, 1.0), (0.0, 0.0, 1.0))
    want = check(ctx, ref, s, q, n, 0.05)
    assert want.kmax == 20000 and want.k.tolist() == [20000, 20000] and want.flags.tolist() == [0, 1]
    assert ctx.stat("boundary_kmax") == 20000


# ---- 5. the forms ----

def test_dev_form_equals_the_host_form_and_runs_repeat(plane):
    import torch
    from pcl_feature_extraction_amd import Context
    dev = torch.device("cuda", 0)
    up = lambda *a: [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for v in a]  # noqa: E731
    s, n = up(*plane["xyz"]), up(*plane["normals"])
    out = [torch.full((4096,), 7, dtype=torch.uint8, device=dev) for _ in range(2)]
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.set_stream(stream.cuda_stream)
        # no host wait between these launches and synchronize()
        c.boundary_dev(*s, *s, *n, 0.05, out[0])
        c.boundary_dev(*s, *s, *n, 0.05, out[1], angle_threshold=PI / 2)
        c.synchronize()
        want = plane["want"]
        assert (c.stat("boundary_neighbors"), c.stat("boundary_kmax"), c.stat("boundary_flagged")) == (
            want.neighbors, want.kmax, want.flagged)
        host = [c.boundary(*plane["xyz"], *plane["xyz"], *plane["normals"], 0.05) for _ in range(2)]
    for o in out + host:
        o = o.cpu().numpy() if hasattr(o, "cpu") else o
        assert np.array_equal(o, want.flags)
