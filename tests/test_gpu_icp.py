"""GPU parity: IterativeClosestPoint::align (evaluation.cpp:863-885) through the C-ABI against the
CPU restatement tests/cpp/icp_ref.cpp, which test_icp_ref.py pins by analytic cases.

Bar: the transformation's float bits, the fitness score's double bits, the iteration count, the
convergence state, the converged flag, the last iteration's correspondence count and the aligned
cloud's bits all equal the restatement's.  Parity of the restatement with real PCL is unpinned."""
import numpy as np
import pytest

import icp_cases as C
import icp_ref as R
import shot_color_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build(tmp_path_factory.mktemp("icp_ref"))


def params_of(p):
    from pcl_feature_extraction_amd import icp_params
    prm = dict(R.REFERENCE)
    prm.update(p or {})
    return icp_params(**prm)


def same_bits(a, b):
    """Equal float32 bits; a NaN is a NaN (its payload is not compared)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.nan_to_num(a, nan=-7.0).view(np.uint32), np.nan_to_num(b, nan=-7.0).view(np.uint32))


def check(ctx, ref, case, want=None):
    """Context.icp against the restatement; returns (result, restatement's result)."""
    s, t, p, g = case
    want = want or R.icp(ref, s, t, p, g)
    got = ctx.icp(*s, *t, params_of(p), g)
    print("icp: iterations %d/%d state %d/%d pairs %d/%d fitness %r/%r" % (
        got.iterations, want.iterations, got.state, want.state, ctx.stat("icp_correspondences"), want.n_last,
        got.fitness, want.fitness))
    print(got.transformation, want.transformation, sep="\n")
    assert (got.iterations, got.state, got.converged) == (want.iterations, want.state, want.converged)
    assert ctx.stat("icp_correspondences") == want.n_last
    assert ctx.stat("icp_iterations") == want.iterations and ctx.stat("icp_state") == want.state
    assert same_bits(got.transformation, want.transformation)
    assert np.float64(got.fitness).view(np.uint64) == np.float64(want.fitness).view(np.uint64)
    for a, b in zip(got.aligned, want.aligned):
        assert same_bits(a, b)
    return got, want


def test_identical_clouds(ctx, ref):
    got, _ = check(ctx, ref, C.identical())
    assert got.iterations == 1 and got.state == R.TRANSFORM and got.fitness == 0.0


def test_shifted_lattice(ctx, ref):
    got, _ = check(ctx, ref, C.shifted_lattice())
    assert got.iterations == 2 and got.state == R.TRANSFORM
    assert ctx.stat("icp_exact_sum") == 1 and ctx.stat("icp_brute") == 0


def test_no_correspondences(ctx, ref):
    got, _ = check(ctx, ref, C.far_apart())
    assert got.state == R.NO_CORRESPONDENCES and not got.converged and got.iterations == 0
    assert np.array_equal(got.transformation, np.eye(4, dtype=np.float32))


def test_iteration_cap(ctx, ref):
    got, _ = check(ctx, ref, C.one_iteration())
    assert got.state == R.ITERATIONS and got.converged


def test_ties_take_the_lowest_target_index(ctx, ref):
    case = C.ties()
    got, want = check(ctx, ref, case)
    # the other mirror image would have moved the fit: swap the pairs and the result differs
    s, t, p, g = case
    swapped = tuple(np.concatenate([v[:12].reshape(6, 2)[:, ::-1].ravel(), v[12:]]) for v in t)
    other = R.icp(ref, s, swapped, p, g)
    assert not same_bits(other.transformation, want.transformation)


def test_cap_is_inclusive_at_equality(ctx, ref):
    check(ctx, ref, C.exact_cap())
    assert ctx.stat("icp_correspondences") == 5


def test_non_finite_points(ctx, ref):
    dirty, clean = C.with_nans()
    got, _ = check(ctx, ref, dirty)
    finite = np.isfinite(np.stack(dirty[0])).all(axis=0)  # a non-finite coordinate spreads over its point
    assert np.array_equal(np.isfinite(np.stack(got.aligned)).all(axis=0), finite) and (~finite).sum() == 4
    other, _ = check(ctx, ref, clean)
    assert same_bits(got.transformation, other.transformation) and got.fitness == other.fitness


@pytest.mark.parametrize("n_list", [2, 3, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_list_lengths(ctx, ref, n_list):
    """Wave edges and depth-block edges of the correspondence list."""
    got, _ = check(ctx, ref, C.list_length(n_list))
    assert ctx.stat("icp_correspondences") == n_list
    assert got.state == (R.NO_CORRESPONDENCES if n_list < 3 else R.TRANSFORM)


def test_retry_rounds_and_certified_none(ctx, ref):
    got, want = check(ctx, ref, C.retry_rounds())
    # cells 0.12, 0.24, 0.48, 0.96: the pairs 0.17 apart fail the first grid, those 0.4 apart the
    # second, and the fourth is the first to reach the cap and certifies "none" for the two points
    # 2 away; the fitness score has no cap, so there they fall to the exhaustive scan
    assert ctx.stat("icp_nn_rounds") == 4 and ctx.stat("icp_brute") == 2
    assert want.n_last == len(want.aligned[0]) - 2


def test_default_distance_takes_the_exhaustive_tail(ctx, ref):
    got, want = check(ctx, ref, C.default_distance(R.PCL_DEFAULT))
    assert ctx.stat("icp_brute") >= 6 and ctx.stat("icp_nn_rounds") == 4
    assert want.n_last == 286  # without a cap every source point has a pair


def test_guess(ctx, ref):
    case = C.with_guess()
    got, want = check(ctx, ref, case)
    # the pose the case applied, then the lattice's own shift
    full = np.eye(4)
    full[:3, 3] = C.DELTA
    assert got.converged and np.abs(got.transformation - full @ case[3].astype(np.float64)).max() < 1e-4
    assert got.iterations == 2 and not same_bits(got.transformation, case[3])


def test_two_runs_are_identical(ctx, ref):
    case = C.retry_rounds()
    s, t, p, g = case
    a = ctx.icp(*s, *t, params_of(p), g)
    b = ctx.icp(*s, *t, params_of(p), g)
    assert same_bits(a.transformation, b.transformation) and a.fitness == b.fitness
    assert (a.iterations, a.state) == (b.iterations, b.state)
    for u, v in zip(a.aligned, b.aligned):
        assert same_bits(u, v)


def test_device_entry_point(ctx, ref):
    import torch
    s, t, p, g = C.shifted_lattice()
    want = R.icp(ref, s, t, p, g)
    dev = torch.device("cuda", 0)
    ds = [torch.from_numpy(v).to(dev) for v in s]
    dt = [torch.from_numpy(v).to(dev) for v in t]
    al = tuple(torch.empty_like(v) for v in ds)
    got = ctx.icp_dev(*ds, *dt, params_of(p), g, aligned=al)
    assert same_bits(got.transformation, want.transformation) and got.fitness == want.fitness
    for a, b in zip(al, want.aligned):
        assert same_bits(a.cpu().numpy(), b)


def test_invalid_arguments(ctx):
    from pcl_feature_extraction_amd import PfxError, icp_params
    s, t, _, _ = C.identical()
    for bad in (dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("nan")),
                dict(max_iterations=-1), dict(transformation_epsilon=float("nan"))):
        with pytest.raises(PfxError) as e:
            ctx.icp(*s, *t, icp_params(**bad))
        assert e.value.code == 1
    d = icp_params()
    assert (d.max_iterations, d.transformation_epsilon) == (10, 0.0)
    assert d.max_correspondence_distance == R.PCL_DEFAULT["max_correspondence_distance"]
    assert d.euclidean_fitness_epsilon == R.PCL_DEFAULT["euclidean_fitness_epsilon"]


# ---- the reference's flow on its indoor pair ----------------------------------------------
@pytest.fixture(scope="module")
def indoor():
    return tuple(S.read_cloud("indoor_" + w)[:3] for w in ("source", "target"))


def test_reference_flow_keypoints(ctx, ref, indoor):
    """ICP of the ISS keypoints, source onto target, reference parameters, 100-iteration cap."""
    kp = []
    for x, y, z in indoor:
        res = ctx.cloud_resolution(x, y, z)
        k = ctx.iss_keypoints(x, y, z, 6 * res, 4 * res)
        kp.append(tuple(np.ascontiguousarray(v[k]) for v in (x, y, z)))
    assert min(len(k[0]) for k in kp) > 500
    got, _ = check(ctx, ref, (kp[0], kp[1], {}, None))
    assert got.iterations > 2


def test_reference_flow_full_clouds(ctx, ref, indoor):
    """The direct ICP of the two clouds; 5 iterations keep the restatement within seconds."""
    got, _ = check(ctx, ref, (indoor[0], indoor[1], dict(max_iterations=5), None))
    assert got.iterations == 5 and got.state == R.ITERATIONS
    assert ctx.stat("icp_correspondences") > 10000
