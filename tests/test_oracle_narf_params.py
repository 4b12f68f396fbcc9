"""The CPU restatement (oracle/or_narf.cpp) off the default camera and parameters: the trusted side
of test_gpu_narf_params.py.  Every case of tests/narf_cases.py runs at the small camera S
(161 x 119, cx 80.5, cy 59, fx 131.25, fy 140) on the golden cloud indoor_source.

Measured with this oracle at S, default parameters: 21 keypoints, 47 pixels with interest >= 0.45,
10,323 observed pixels.  Pixels whose bits differ from that run, per parameter:

    parameter set to                          keypoints  traits  surface change  interest
    pixel_radius_borders 1                        14      1078       2535          5092
    pixel_radius_borders 5                        22      1735       3188          5618
    pixel_radius_plane_extraction 0                0      1596       9480          9328
    pixel_radius_plane_extraction 4                9      1383       9881          9904
    pixel_radius_border_direction 0               43         0         30          1946
    pixel_radius_border_direction 4               17         0         32          1626
    pixel_radius_principal_curvature 1            46         0       8949          9139
    pixel_radius_principal_curvature 4            13         0       8942          9237
    minimum_border_probability 0.5                37      1135       2702          4849
    min_surface_change_score 0.05                 16         0          0          2487
    optimal_distance_to_high_surface_change 0.5    6         0          0          3127
    min_interest_value 0.2                       371         0          0             0
    max_no_of_interest_points 5                    5         0          0             0
    min_distance_between_interest_points 1.0      18         0          0             0
    do_non_maximum_suppression 0                  21         0          0             0

The figures are counts of DIFFERING pixels, not of non-zero ones: at
pixel_radius_plane_extraction 0 every pixel has a single neighbour (itself), getSurfaceInformation
needs three, so no pixel has a normal and the trait, surface-change and interest images are zero
throughout (1596 is the default run's count of non-zero trait words).  That case therefore cannot
have "more than 0 pixels with a non-zero trait word"; it is kept as the degenerate path, and
pixel_radius_plane_extraction 1 and 3 (not in the table above) are swept beside it:

    pixel_radius_plane_extraction 1               34      1685       9175          9525
    pixel_radius_plane_extraction 3               18      1001       9354          9545

min_range 1.5 leaves 9,703 observed pixels and 20 keypoints.  On the general pose G with
LASER_FRAME: 20 keypoints at the default support size, 49 / 17 / 19 at support 0.1 / 0.5 / 1.0.
(test_table_reproduces pins these figures.)
"""
import numpy as np
import pytest

import narf_cases as C

TABLE = {  # id: (keypoints, traits, surface change, interest) as in the docstring
    "prb1": (14, 1078, 2535, 5092), "prb5": (22, 1735, 3188, 5618), "prpe0": (0, 1596, 9480, 9328),
    "prpe1": (34, 1685, 9175, 9525), "prpe3": (18, 1001, 9354, 9545), "prpe4": (9, 1383, 9881, 9904), "prbd0": (43, 0, 30, 1946), "prbd4": (17, 0, 32, 1626),
    "prpc1": (46, 0, 8949, 9139), "prpc4": (13, 0, 8942, 9237), "mbp0.5": (37, 1135, 2702, 4849),
    "min_scs0.05": (16, 0, 0, 2487), "opt_dist0.5": (6, 0, 0, 3127), "min_interest0.2": (371, 0, 0, 0),
    "cap5": (5, 0, 0, 0), "min_dist1.0": (18, 0, 0, 0), "nms0": (21, 0, 0, 0),
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32).ravel()


def _ndiff(a, b):
    return int(np.count_nonzero(_bits(a) != _bits(b)))


def test_laser_frame_is_the_pose_times_the_axis_matrix():
    """coordinate_frame = 1 with pose G gives the range image of coordinate_frame = 0 with pose
    G * L (L: entries 0, +-1, so the product is exact), bit for bit on all four channels."""
    import oracle_lib as O
    spec, cam = C.RANGE_CASES["S_G_laser"]
    gl = (C.pose32("G").astype(np.float64) @ C.L).astype(np.float32)
    assert np.array_equal(gl.astype(np.float64), C.pose32("G").astype(np.float64) @ C.L)  # exact in float32
    a = C.oracle_range("S_G_laser")
    b = O.range_image_planar(*C.cloud(spec), cam=dict(C.S, sensor_pose=gl, coordinate_frame=0))
    assert a.shape == (119, 161, 4) and np.array_equal(_bits(a), _bits(b))
    assert np.count_nonzero(np.isfinite(a[..., 3])) > 5000


def test_exact_pose_keeps_the_range_channel():
    """The quantised cloud moved by the 90-degree pose, seen from that pose, has the range channel
    of the unmoved cloud seen from the identity (every product and sum of to_ri * p is exact).
    x, y, z and the keypoints need not match: later float sums are not symmetric under the axis
    permutation."""
    import oracle_lib as O
    moved = C.oracle_range("S_exact90")
    still = O.range_image_planar(*C.cloud(("indoor_q",)), cam=C.S)
    assert np.array_equal(_bits(moved[..., 3]), _bits(still[..., 3]))
    assert np.count_nonzero(np.isfinite(moved[..., 3])) > 5000
    # the pose did something: the world coordinates differ
    assert _ndiff(moved[..., :3], still[..., :3]) > 5000


@pytest.mark.parametrize("row", C.SWEEP, ids=[r[0] for r in C.SWEEP])
def test_parameter_reaches_its_stage(row):
    name, _, stage = row
    kp0, d0 = C.oracle_narf("default")
    kp, d = C.oracle_narf(name)
    if stage is None:  # do_non_maximum_suppression = 0 changes nothing at S (k_nms still takes it)
        assert np.array_equal(kp, kp0)
    elif stage == "keypoints":
        assert not np.array_equal(kp, kp0)
    else:
        assert _ndiff(d[stage], d0[stage]) > 0
        for earlier in ("border_traits", "surface_change", "interest"):
            if earlier == stage:
                break
            assert _ndiff(d[earlier], d0[earlier]) == 0  # `stage` is the first that differs


def test_table_reproduces():
    kp0, d0 = C.oracle_narf("default")
    assert len(kp0) == 21
    assert int(np.count_nonzero(d0["interest"] >= 0.45)) == 47
    assert int(np.count_nonzero(np.isfinite(d0["range"]))) == 10323
    got = {}
    for name in TABLE:
        kp, d = C.oracle_narf(name)
        got[name] = (len(kp),) + tuple(_ndiff(d[k], d0[k]) for k in ("border_traits", "surface_change", "interest"))
    assert got == TABLE
    kp, d = C.oracle_narf("min_range1.5")
    assert (len(kp), int(np.count_nonzero(np.isfinite(d["range"])))) == (20, 9703)
    counts = [len(C.oracle_narf(n)[0]) for n in ("G_laser", "G_laser_support0.1", "G_laser_support0.5",
                                                   "G_laser_support1")]
    assert counts == [20, 49, 17, 19]


def test_selection_parameters_count():
    n0 = len(C.oracle_narf("default")[0])
    assert len(C.oracle_narf("cap5")[0]) == 5
    assert len(C.oracle_narf("min_interest0.2")[0]) > n0
    assert len(C.oracle_narf("min_dist1.0")[0]) <= n0


@pytest.mark.parametrize("name", C.SMALL_CASES)
def test_case_is_not_vacuous(name):
    kp, d = C.oracle_narf(name)
    assert int(np.count_nonzero(np.isfinite(d["range"]))) > 5000
    assert np.all(np.diff(kp) > 0)
    if name in C.NO_KEYPOINTS:
        # pixel_radius_plane_extraction = 0 (see the docstring): nothing but zeros, which still
        # differs from the default run in 1596 trait words and 9480 surface-change scores
        _, d0 = C.oracle_narf("default")
        assert len(kp) == 0
        assert np.count_nonzero(d["border_traits"]) == 0 and np.count_nonzero(d["surface_change"]) == 0
        assert _ndiff(d["border_traits"], d0["border_traits"]) > 0
        assert _ndiff(d["surface_change"], d0["surface_change"]) > 0
    elif name in C.FEW_KEYPOINTS:
        _, d0 = C.oracle_narf("default")
        assert len(kp) >= 1 and _ndiff(d["interest"], d0["interest"]) > 1000
    else:
        assert len(kp) >= 5


def test_looking_away_sees_nothing():
    a = C.oracle_range("S_away")
    assert np.all(np.isnan(a[..., :3])) and np.all(np.isneginf(a[..., 3]))


def test_tiny_images_see_something():
    assert np.count_nonzero(np.isfinite(C.oracle_range("17x13")[..., 3])) > 100
    assert np.isfinite(C.oracle_range("1x1")[0, 0, 3])
