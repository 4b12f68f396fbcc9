"""Shared by the matching GPU tests: run the C-ABI matcher on device tensors and compare it with
the CPU restatement (oracle/or_match.cpp) -- both directions, indices, distance bits and the
correspondence list."""
import numpy as np

import oracle_lib as O


def _gpu_nearest(ctx, src, tgt, stride=None):
    import torch
    d = src.shape[1]
    if stride:
        def pad(a):
            p = np.full((a.shape[0], stride), 7.0, np.float32)
            p[:, :d] = a
            return p
        src, tgt = pad(src), pad(tgt)
    s = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(tgt)).cuda()
    s2t = torch.empty(len(src), dtype=torch.int32, device="cuda")
    t2s = torch.empty(len(tgt), dtype=torch.int32, device="cuda")
    ds = torch.empty(len(src), dtype=torch.float32, device="cuda")
    dt = torch.empty(len(tgt), dtype=torch.float32, device="cuda")
    ctx.nearest_descriptors_dev(s, t, s2t, ds, t2s, dt, dim=d)
    torch.cuda.synchronize()
    return s2t.cpu().numpy(), ds.cpu().numpy(), t2s.cpu().numpy(), dt.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.nan_to_num(a, nan=-7).view(np.uint32), np.nan_to_num(b, nan=-7).view(np.uint32))


def _check(ctx, src, tgt, stride=None):
    s2t, ds, t2s, dt = _gpu_nearest(ctx, src, tgt, stride)
    os2t, ods = O.nearest_descriptor(src, tgt)
    ot2s, odt = O.nearest_descriptor(tgt, src)
    assert np.array_equal(s2t, os2t)
    assert np.array_equal(t2s, ot2s)
    assert _same(ds, ods) and _same(dt, odt)
    q, m = ctx.correspondences(src, tgt)
    oq, om = O.correspondences(src, tgt)
    assert np.array_equal(q, oq) and np.array_equal(m, om)
    return len(q)
