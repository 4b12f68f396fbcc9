"""Pins tests/cpp/knn_ref.cpp, the CPU restatement of DESIGN.md "k-NN: the contract", without a GPU:
its rows against a numpy lexsort statement of the contract on every case of knn_cases (every query of
the small cases; of the 8,192-point ones every 16th query and all the separate ones), its normals
against the oracle's radius normals where the two neighbour lists are the same list, and closed
forms."""
import numpy as np
import pytest

import knn_cases as C
import knn_ref as R

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("knn_ref"))


def same_rows(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))


def _cases():
    x, y, z = C.room()
    sub = slice(0, None, 16)
    yield "room", (x, y, z), (x[sub], y[sub], z[sub]), 32
    yield "room_queries", (x, y, z), C.room_queries(), 32
    yield "lattice", C.lattice(), None, 30
    d = C.duplicates()
    yield "duplicates", d[:3], None, 10
    yield "two_densities", C.two_densities(), None, 32
    fx, fy, fz = C.far_origin()
    yield "far_origin", (fx, fy, fz), (fx[sub], fy[sub], fz[sub]), 32
    yield "identical", C.identical(), None, 10
    yield "collinear", C.collinear(), None, 10
    yield "coplanar", C.coplanar(), None, 10
    yield "single", C.single(), None, 5
    yield "short", C.short(), None, 10
    nx, ny, nz, _ = C.with_nonfinite(*C.two_densities())
    yield "non_finite", (nx, ny, nz), None, 10


@pytest.mark.parametrize("name,surface,queries,k", list(_cases()), ids=[c[0] for c in _cases()])
def test_rows_are_the_contract(ref, name, surface, queries, k):
    queries = queries or surface
    got = R.search(ref, *surface, *queries, k)
    assert same_rows(got, C.contract_rows(*surface, *queries, k))
    # a smaller k is the prefix of a larger one
    assert same_rows(R.search(ref, *surface, *queries, 3), R.prefix(got, 3))


def test_what_the_cases_are_for(ref):
    x, y, z, at = C.duplicates()
    counts, idx, d2 = R.search(ref, x, y, z, x[at], y[at], z[at], 10)
    assert (idx == at[:10]).all() and (d2 == 0).all()          # the ten lowest indices, for every copy
    counts, idx, d2, (inside, edge) = R.search(ref, *C.lattice(), *C.lattice(), 7, ties=True)
    assert inside == 4096 and edge > 0                          # 7 = self + 6 at d2 = 1 only in the interior
    counts, idx, d2 = R.search(ref, *C.short(), *C.short(), 10)
    assert (counts == 5).all() and (idx[:, 5:] == -1).all() and np.isnan(d2[:, 5:]).all()
    assert (idx[:, 0] == np.arange(5)).all()
    x, y, z, rows = C.with_nonfinite(*C.two_densities())
    counts, idx, d2 = R.search(ref, x, y, z, x, y, z, 10)
    assert (counts[rows] == 0).all() and (idx[rows] == -1).all() and np.isnan(d2[rows]).all()
    keep = np.setdiff1d(np.arange(len(x)), rows)
    assert (counts[keep] == 10).all() and not np.isin(idx[keep], rows).any()
    counts, idx, d2 = R.search(ref, *C.single(), *C.single(), 5)
    assert counts.tolist() == [1] and idx[0].tolist() == [0, -1, -1, -1, -1] and d2[0, 0] == 0


def test_normals_equal_the_oracle_where_the_lists_coincide(ref):
    """n = 200, k = n: the row of a point is every point in (d2, index) order, and so is the radius
    list at a radius that holds the whole cloud."""
    import oracle_lib as O
    x, y, z = (v[:200] for v in C.room())
    want = O.normals(x, y, z, 100.0)
    got = R.normals(ref, x, y, z, 200)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))
    assert np.isfinite(got[0]).all()
    vp = (0.5, -2.0, 7.0)
    for a, b in zip(R.normals(ref, x, y, z, 200, vp), O.normals(x, y, z, 100.0, vp=vp)):
        assert np.array_equal(bits(a), bits(b))


def test_plane_and_too_few_neighbours(ref):
    """A plane z = 1 seen from the origin: the z row and column of the covariance are exactly 0 (the
    sums of z and of x z are the sums of 1 and of x), so the normal is -z and the curvature 0 up to
    the rounding of eigen33's roots: a few ulp of the scaled matrix, divided by an in-plane eigenvalue
    gap above a tenth of the scale for the eigenvector, hence the 1e-5 below."""
    x, y, z = C.plane_grid()
    nx, ny, nz, curv = R.normals(ref, x, y, z, 10)
    assert (nz < -(1.0 - 1e-5)).all() and (np.abs(nx) < 1e-5).all() and (np.abs(ny) < 1e-5).all()
    assert (curv >= 0).all() and (curv < 1e-5).all()
    nx, ny, nz, curv = R.normals(ref, x, y, z, 10, (0.0, 0.0, 5.0))
    assert (nz > 1.0 - 1e-5).all()
    for k in (1, 2):
        for col in R.normals(ref, x, y, z, k):
            assert np.isnan(col).all()
    assert np.isfinite(R.normals(ref, x, y, z, 3)[3]).all()
