"""The deferred reports of the stream-ordered descriptor calls (the error words of a *_dev call,
copied to pinned memory in stream order and read after the next synchronisation): the order in
which pending reports are raised, what a throw leaves pending, which reports a host entry point
resolves, that stat() resolves, and that trim() leaves the sticky words fresh.

Clouds: one blob of 16,385 points inside the radius of each of its points (one neighbour beyond the
second pass's capacity) with a lone anchor point, and ordinary clouds of 320 points (eight blobs of
40) with three queries."""
import numpy as np
import pytest

import list_edge_clouds as E
import moments_cases as M
import rift_cases as K
import spin_cases as S
from parity import bits

pytestmark = pytest.mark.gpu

QUERIES = 3


@pytest.fixture(scope="module")
def blob():
    xyz, ((k, lo, hi),) = E.exact_k_blobs(caps=[16384], deltas=(1,))
    assert k == 16385
    rows = [0, lo]     # the anchor (a lone point) and a point of the blob beyond capacity
    return dict(xyz=xyz, q=tuple(v[rows] for v in xyz), axes=S.axes(2), grads=K.random_vectors(len(xyz[0]), 701, 30.0))


@pytest.fixture(scope="module")
def ordinary():
    """The ordinary clouds of spin images and of moment invariants, with their rows from a fresh context."""
    from pcl_feature_extraction_amd import Context
    s, m = S.order_case(k=40, blobs=8), M.order_case(k=40, blobs=8)
    s = dict(xyz=s["xyz"], q=tuple(v[:QUERIES] for v in s["q"]), axes=tuple(v[:QUERIES] for v in s["axes"]))
    m = dict(xyz=m["xyz"], q=tuple(v[:QUERIES] for v in m["q"]))
    grads = K.random_vectors(len(m["xyz"][0]), 702, 30.0)
    with Context(0) as c:
        s["want"] = c.spin_image(*s["xyz"], *s["q"], *s["axes"], S.R)
        m["want"] = c.moment_invariants(*m["xyz"], *m["q"], M.R)
        rift = c.rift(*m["xyz"], *grads, *m["q"], M.R)
    assert np.isfinite(s["want"]).all() and np.isfinite(m["want"]).all() and np.isfinite(rift).all()
    return dict(spin=s, moments=m, grads=grads, rift=rift)


def up(*a):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.device("cuda", 0)) for v in a]


def zeros(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.float32, device=torch.device("cuda", 0))


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), what


def spin_rows(c, o):
    return c.spin_image(*o["xyz"], *o["q"], *o["axes"], S.R)


def moment_rows(c, o):
    return c.moment_invariants(*o["xyz"], *o["q"], M.R)


def raises_capacity(call, family):
    from pcl_feature_extraction_amd import PfxError
    from pcl_feature_extraction_amd._native import PFX_ERR_CAPACITY
    with pytest.raises(PfxError) as e:
        call()
    assert e.value.code == PFX_ERR_CAPACITY and "16385" in str(e.value)
    assert (" " + family + ": a query has ") in str(e.value), str(e.value)


def test_reports_are_raised_in_order_and_a_throw_leaves_the_later_ones_pending(blob, ordinary):
    import torch
    from pcl_feature_extraction_amd import Context
    s, q, ax = up(*blob["xyz"]), up(*blob["q"]), up(*blob["axes"])
    out_s, out_m = zeros(2, 153), zeros(2, 3)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.spin_image_dev(*s, *q, *ax, E.R, out_s)
        c.moment_invariants_dev(*s, *q, E.R, out_m)
        raises_capacity(c.synchronize, "spin_image")
        raises_capacity(c.synchronize, "moment_invariants")
        c.synchronize()   # each reported once
        same(spin_rows(c, ordinary["spin"]), ordinary["spin"]["want"], "spin images after the errors")
        same(moment_rows(c, ordinary["moments"]), ordinary["moments"]["want"], "moment invariants after the errors")
        c.synchronize()


def test_a_host_call_leaves_another_family_s_report_pending(blob, ordinary):
    import torch
    from pcl_feature_extraction_amd import Context
    s, q, ax = up(*blob["xyz"]), up(*blob["q"]), up(*blob["axes"])
    out_s = zeros(2, 153)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.spin_image_dev(*s, *q, *ax, E.R, out_s)
        same(moment_rows(c, ordinary["moments"]), ordinary["moments"]["want"], "moment invariants, spin's error pending")
        raises_capacity(c.synchronize, "spin_image")
        c.synchronize()


def test_stat_resolves_a_pending_report(blob, ordinary):
    import torch
    from pcl_feature_extraction_amd import Context
    s, sg, q = up(*blob["xyz"]), up(*blob["grads"]), up(*blob["q"])
    out_r = zeros(2, 32)
    torch.cuda.synchronize()
    with Context(0) as c:
        c.rift_dev(*s, *sg, *q, E.R, out_r)
        raises_capacity(lambda: c.stat("rift_kmax"), "rift")
        assert c.stat("rift_kmax") == 16385   # reported once; the statistics of that call stand
        c.synchronize()


def test_trim_leaves_the_sticky_words_fresh(blob, ordinary):
    from pcl_feature_extraction_amd import Context
    m = ordinary["moments"]
    with Context(0) as c:
        raises_capacity(lambda: c.spin_image(*blob["xyz"], *blob["q"], *blob["axes"], E.R), "spin_image")
        raises_capacity(lambda: c.rift(*blob["xyz"], *blob["grads"], *blob["q"], E.R), "rift")
        c.trim()
        same(spin_rows(c, ordinary["spin"]), ordinary["spin"]["want"], "spin images after trim")
        same(c.rift(*m["xyz"], *ordinary["grads"], *m["q"], M.R), ordinary["rift"], "rift after trim")
        c.synchronize()
