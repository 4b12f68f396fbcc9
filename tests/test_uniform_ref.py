"""The CPU restatement of PCL 1.7 UniformSampling (tests/cpp/uniform_ref.cpp), pinned against
closed forms and against the plain numpy statement of DESIGN.md "Uniform sampling: the contract"
(tests/uniform_cases.py: lexsort by leaf, diff and index, then the run heads).  No GPU needed.  The
restatement walks PCL's sequential loop (first point kept, replaced on a strict <); the numpy
statement sorts: that they agree confirms the "smallest (diff, index)" reading."""
import numpy as np
import pytest

import uniform_cases as C
import uniform_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("uniform_ref"))


def _same(r, stated):
    idx, leaf, points, cells = stated
    assert r.status == R.OK
    assert np.array_equal(r.idx, idx) and np.array_equal(r.leaf, leaf)
    assert (r.points, r.leaves, r.cells) == (points, len(idx), cells)


def test_one_point_per_cell(ref):
    x, y, z, idx, leaf = C.lattice()
    r = R.sample(ref, x, y, z, C.LATTICE_LEAF)
    assert r.status == R.OK
    assert np.array_equal(r.idx, idx) and np.array_equal(r.leaf, leaf)
    assert np.array_equal(r.leaf, np.arange(105)) and sorted(r.idx.tolist()) == list(range(105))
    assert (r.points, r.leaves, r.cells) == (105, 105, 7 * 5 * 3)
    assert (x < 0).any() and (y < 0).any() and (z < 0).any()
    _same(r, C.numpy_statement(x, y, z, C.LATTICE_LEAF))


def test_plus_one_tie(ref):
    """Both diffs round to 1.0f, so the first point of the cell stays although it is farther; a
    kernel that drops the +1 picks the nearer one."""
    for swapped in (False, True):
        x, y, z = C.tie(swapped)
        i, j, k = (C.cells_of(v, C.TIE_LEAF) for v in (x, y, z))
        assert i.tolist() == j.tolist() == k.tolist() == [1, 1]
        d = C.diffs(x, y, z, i, j, k)
        assert d[0] == d[1] == f32(1.0)
        dx = x - f32(1.0)
        assert (dx * dx)[0] != (dx * dx)[1]                          # ordered without the +1
        r = R.sample(ref, x, y, z, C.TIE_LEAF)
        assert r.status == R.OK and r.idx.tolist() == [0] and r.leaf.tolist() == [0]
        _same(r, C.numpy_statement(x, y, z, C.TIE_LEAF))
        nearer = 0 if swapped else 1
        assert C.numpy_statement(x, y, z, C.TIE_LEAF, plus_one=False)[0].tolist() == [nearer]
    # the farther point is index 0 in the first order
    assert C.tie(False)[0][0] > C.tie(False)[0][1]


def test_association(ref):
    """Eigen's (a0 + a2) + (a1 + a3): in every committed pair the scalar order ((dx^2 + dy^2) + dz^2) + 1
    picks the other point."""
    pairs = C.assoc_pairs()
    assert pairs.shape == (48, 2, 3)
    stated, scalar = C.assoc_winner(pairs, False), C.assoc_winner(pairs, True)
    assert (stated >= 0).all() and (stated != scalar).all()
    assert (stated == 0).sum() == 24 and (stated == 1).sum() == 24
    for a in range(3):
        assert (C.cells_of(pairs[..., a], C.ASSOC_LEAF) == C.ASSOC_CELL[a]).all()
    for p, w in zip(pairs, stated):
        r = R.sample(ref, p[:, 0], p[:, 1], p[:, 2], C.ASSOC_LEAF)
        assert r.status == R.OK and r.idx.tolist() == [int(w)] and r.cells == 1
        assert C.numpy_statement(p[:, 0], p[:, 1], p[:, 2], C.ASSOC_LEAF, scalar_order=True)[0].tolist() == [1 - int(w)]


def test_association_decides_often():
    """Where the committed pairs come from (assoc_traded_pairs): the two orders disagree often
    enough for the case to matter (measured on 200,000 draws: 14.5 %)."""
    pairs = C.assoc_traded_pairs(20000)
    stated, scalar = C.assoc_winner(pairs, False), C.assoc_winner(pairs, True)
    assert len(pairs) > 5000 and (stated >= 0).all()
    assert 0.05 < (stated != scalar).mean() < 0.5


#: the points whose float32 product puts them in a cell other than k, and whose cell differs from the
#: float64 quotient's (computed once for the issue, reproduced here)
EDGE_COUNTS = {0.05: (0, 1988), 0.01: (267, 1712), 0.08: (267, 1712)}


@pytest.mark.parametrize("leaf", C.EDGE_LEAVES)
def test_cell_edges(ref, leaf):
    x, y, z, k = C.cell_edges(leaf)
    cell = C.cells_of(x, leaf)
    quotient = np.floor(x.astype(np.float64) / np.float64(f32(leaf))).astype(np.int64)
    assert ((cell != k).sum(), (cell != quotient).sum()) == EDGE_COUNTS[leaf]
    trunc = np.trunc(x * C._inv(leaf)).astype(np.int64)
    # floor, not truncation: wherever a negative product is not a whole number (at 0.05 every one is)
    assert (trunc[x < 0] != cell[x < 0]).any() == (leaf != 0.05)
    r = R.sample(ref, x, y, z, leaf)
    _same(r, C.numpy_statement(x, y, z, leaf))
    # closed form: the occupied cells are the distinct float32 cells; the first point of each wins
    # unless a later one is nearer the integer cell coordinate
    assert np.array_equal(r.leaf, np.unique(cell) - cell.min())
    assert r.cells == cell.max() - cell.min() + 1


@pytest.mark.parametrize("leaf,count", zip(C.ROOM_LEAVES, (543, 3228)))
def test_synthetic_room(ref, leaf, count):
    x, y, z = C.room()
    r = R.sample(ref, x, y, z, leaf)
    _same(r, C.numpy_statement(x, y, z, leaf))
    assert 0.01 < r.leaves / len(x) < 0.5
    assert r.leaves == count                                         # the numpy prototype's count
    assert (np.diff(r.leaf) > 0).all()


def test_non_finite_points_take_no_part(ref):
    x, y, z, rows = C.room_with_nonfinite()
    r = R.sample(ref, x, y, z, 0.05)
    _same(r, C.numpy_statement(x, y, z, 0.05))
    assert r.points == len(x) - len(rows) and not np.isin(r.idx, rows).any()
    keep = np.setdiff1d(np.arange(len(x)), rows)
    s = R.sample(ref, x[keep], y[keep], z[keep], 0.05)                # the same cloud without the rows
    assert np.array_equal(keep[s.idx], r.idx) and np.array_equal(s.leaf, r.leaf) and s.cells == r.cells
    nan = np.full(7, np.nan, f32)
    for cloud in ((nan, nan, nan), (np.zeros(0, f32),) * 3):
        e = R.sample(ref, *cloud, 0.05)
        assert (e.status, len(e.idx), e.points, e.leaves, e.cells) == (R.OK, 0, 0, 0, 0)


def test_errors(ref):
    x, y, z = C.cube_corners(12.0)
    for radius in (0.0, -0.05, float("nan"), 1e-46, float("inf")):
        assert R.sample(ref, x, y, z, radius).status == R.INVALID
    ok = R.sample(ref, x, y, z, 0.01)                                 # ~1.73e9 cells: below 2^31
    assert ok.status == R.OK and ok.leaves == 8 and 1.7e9 < ok.cells < 2 ** 31
    assert R.sample(ref, *C.cube_corners(2000.0), 0.001).status == R.CAPACITY
    far = np.array([0.0, 1e12], f32)
    assert R.sample(ref, far, far * 0, far * 0, 0.05).status == R.CAPACITY
    assert R.sample(ref, far[1:], far[1:] * 0, far[1:] * 0, 0.05).status == R.CAPACITY
