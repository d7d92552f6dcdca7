"""k_kv_seq_cp at kernel level (llmi_kv_seq_copy over torch tensors as device memory): the copy
of positions [p0, p1) of a K cache, a transposed V cache and a token history is exact, 16 bits
for 16 bits (random patterns over the full range, NaN payloads included), writes nothing of dst
outside the range, nothing before or after its buffers, and nothing of src.

Every buffer sits inside a larger allocation (PAD bytes on both sides, a multiple of 16 so that
the buffer keeps the caches' alignment) and the WHOLE allocation is compared with a NumPy copy.
The ranges are where the V rows' unaligned head / 16-byte body / unaligned tail logic can go
wrong: single positions, ranges inside one 8-position window, ending or starting on a window
boundary, one past it, a whole row, and ranges across position 256.  The launcher picks the
kernel's items per thread (4 or 1) by the copy's size; the test option kv_cp_unroll forces
each, so both kernels meet every case at these small shapes."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
from helpers import to_dev

pytestmark = pytest.mark.gpu

N_PLANES = 3
PAD = 256  # bytes of guard on each side of every buffer
RANGES = [(0, 1), (0, 7), (0, 8), (0, 9), (3, 4), (5, 13), (7, 8), (8, 16), (1, 256), (255, 256)]
RANGES_512 = [(249, 263), (0, 512)]
CASES = [(hd, n_ctx, r) for hd in (64, 128) for n_ctx in (256, 512) for r in RANGES + (RANGES_512 if n_ctx == 512 else [])]


def _guarded(rng, n, dtype):
    """A random host array of n items between two random guards of PAD bytes: (whole, slice)."""
    g = PAD // np.dtype(dtype).itemsize
    info = np.iinfo(dtype)
    whole = rng.integers(info.min, int(info.max) + 1, n + 2 * g, dtype=np.int64).astype(dtype)
    return whole, slice(g, g + n)


@pytest.fixture(params=[4, 1], ids=["u4", "u1"])
def unroll(request):
    old = llmi.test_option("kv_cp_unroll", request.param)
    yield request.param
    llmi.test_option("kv_cp_unroll", old)


@pytest.mark.parametrize("head_dim,n_ctx,rng_", CASES, ids=[f"d{h}-c{c}-{a}_{b}" for h, c, (a, b) in CASES])
def test_copy_is_exact_and_stays_in_range(gpu, unroll, head_dim, n_ctx, rng_):
    p0, p1 = rng_
    rng = np.random.default_rng(1000 * head_dim + n_ctx + 7 * p0 + p1)
    kv = N_PLANES * n_ctx * head_dim
    host, dev, sl = {}, {}, {}
    for side in ("src", "dst"):
        for name, n, dt in (("k", kv, np.int16), ("v", kv, np.int16), ("h", n_ctx, np.int32)):
            host[side, name], sl[name] = _guarded(rng, n, dt)
            dev[side, name] = to_dev(host[side, name])
    addr = lambda side, name: dev[side, name].data_ptr() + PAD  # noqa: E731
    us = llmi.kv_seq_copy(N_PLANES, head_dim, n_ctx, p0, p1, addr("src", "k"), addr("src", "v"), addr("src", "h"),
                          addr("dst", "k"), addr("dst", "v"), addr("dst", "h"))
    assert us > 0.0

    want = {key: a.copy() for key, a in host.items() if key[0] == "dst"}
    ks = host["src", "k"][sl["k"]].reshape(N_PLANES, n_ctx, head_dim)
    want["dst", "k"][sl["k"]].reshape(N_PLANES, n_ctx, head_dim)[:, p0:p1, :] = ks[:, p0:p1, :]
    vs = host["src", "v"][sl["v"]].reshape(N_PLANES, head_dim, n_ctx)
    want["dst", "v"][sl["v"]].reshape(N_PLANES, head_dim, n_ctx)[:, :, p0:p1] = vs[:, :, p0:p1]
    want["dst", "h"][sl["h"]][p0:p1] = host["src", "h"][sl["h"]][p0:p1]
    for name in ("k", "v", "h"):
        got = dev["dst", name].cpu().numpy()
        bad = np.flatnonzero(got != want["dst", name])
        assert bad.size == 0, (f"dst {name}: {bad.size} items differ, first at item {int(bad[0])} of the allocation "
                               f"(the buffer starts at item {sl[name].start})")
        assert np.array_equal(dev["src", name].cpu().numpy(), host["src", name]), f"src {name} was written"
