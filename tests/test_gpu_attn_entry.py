"""k_attn_d's entry: the K passes it requests before the step position is known.

The dim-split kernel (path 6) issues the K passes that lie wholly below kv_bound - 256
together with q, ahead of the position; the passes that overlap the bucket's last 256
positions, and the V slice, keep their test on the position.  An early load must never
reach the output through a dead row, so every case here is driven through the attention
hook (llmi_attention, mode 6) and compared bit for bit with the NumPy reference of
tests/test_gpu_attention.py, at the KV lengths where the split between the two groups of
passes can go wrong:

  a pass holding exactly one live position       n_kv = 1, 65, 257, 513, 769
  the first conditional pass at its emptiest     n_kv = 257, 513, 769: one live position in
                                                 it, every later conditional pass empty
  every conditional pass live                    n_kv = 256, 512, 768, 1024
  a bucket with no always-live pass at all       kv_bound 256: n_kv = 1 .. 256
  the last live pass one short, full, one over   63 64 65, 255 256 257, 511 512 513, ...

Each length runs in a context larger than every bucket (the bucket rule gives kv_bound) and
in a context with n_ctx == kv_bound (the cap of kv_bucket_bound and the row clamp
min(t, kv_bound - 1) are live; another V stride).  The hook derives kv_bound from n_kv and
n_ctx by the bucket rule and takes no bound of its own, so a bound one bucket above the
natural one (a first conditional pass that is wholly empty) cannot be driven from here.

Positions past the live edge hold finite, live-like poison in one run (the wide regime's
data: keys past the edge are among the highest scores) and NaN in another.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_attention import _assert_same, _attend, _bound, _checked_path, _data

SHAPES = [(32, 8, 128), (8, 8, 64), (32, 4, 64)]
N_KV = [1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 767, 768, 769, 1023, 1024]
N_CTX = 8448
PATH = 6

_dev: dict = {}


def _caches(shape, n_ctx, n_kv, poison):
    """Device K [HK][n_ctx][D] and V [HK][D][n_ctx] of the shape's wide data; poison "nan": NaN
    in every position past the live edge.  One device copy per (shape, n_ctx, poison) for
    the finite caches, which do not depend on n_kv."""
    from helpers import to_dev

    d = _data(shape, "wide")
    key = (shape, n_ctx) if poison == "finite" else None
    if key in _dev:
        return _dev[key]
    K = d.K[:, :n_ctx, :].copy()  # copies: the shared data stays live-like
    V = d.V[:, :, :n_ctx].copy()
    if poison == "nan":
        K[:, n_kv:, :] = np.nan
        V[:, :, n_kv:] = np.nan
    out = (to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1)))
    if key is not None:
        if len(_dev) >= 4:
            _dev.clear()
        _dev[key] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["finite", "nan"])
@pytest.mark.parametrize("context", ["bucket", "tight"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_attn_d_entry(gpu, shape, context, poison):
    d = _data(shape, "wide")
    for n_kv in N_KV:
        kvb = _bound(n_kv, N_CTX)
        n_ctx = N_CTX if context == "bucket" else kvb
        assert _checked_path(shape, _bound(n_kv, n_ctx), PATH) == PATH
        kd, vd = _caches(shape, n_ctx, n_kv, poison)
        got = _attend(shape, n_kv, n_ctx, d.q(n_kv), kd, vd, PATH)
        where = f"{shape} n_kv {n_kv} n_ctx {n_ctx} {poison} poison"
        assert np.isfinite(got).all(), f"{where}: a dead position leaked into the output"
        _assert_same(got, d.ref(n_kv), where)
