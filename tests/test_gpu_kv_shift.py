"""k_kv_shift (the llmi_kv_shift hook over torch tensors) against a NumPy restatement of its
definition, bit for bit: positions [n_keep + d, n_past) of K, transposed V and the history move
down by d in place, the K pairs (2i, 2i + 1) below n_rot rotated back by row d of the table
(built here in float64, rounded to f32; f32 products and sums).  K holds normal f16 values below
2^10.  Every buffer lies between canaries and the WHOLE allocation is compared.  The kernel's
chunk is 256 positions: the tails lie below, at and above d and around one chunk."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
from helpers import to_dev

pytestmark = pytest.mark.gpu

N_PLANES, N_CTX, PAD = 2, 768, 256
# (n_keep, d, n_past); tail = n_past - n_keep - d
SHIFTS = [(0, 1, 768), (5, 1, 768), (1, 7, 600),          # tail >> d: overlap across chunks; n_past = n_ctx
          (5, 9, 269), (5, 8, 269), (0, 9, 266),          # tail 255, 256, 257: around one chunk
          (1, 255, 768), (0, 256, 768),                   # d = chunk - 1, chunk; tail two chunks
          (0, 256, 512), (1, 255, 511),                   # tail == d
          (5, 256, 300), (1, 8, 10),                      # tail < d: no overlap
          (5, 7, 12)]                                     # empty tail: nothing moves
CASES = [(hd, n_rot, s) for hd in (64, 128) for n_rot in (hd, hd // 2, hd - 2) for s in SHIFTS]


def rope_table(n_ctx, n_rot, base=10000.0):
    theta = base ** (-2.0 * np.arange(n_rot // 2, dtype=np.float64) / n_rot)
    ang = np.arange(n_ctx, dtype=np.float64)[:, None] * theta[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)  # [n_ctx][n_rot/2][cos, sin]


def shifted(k, v, h, tab, n_rot, n_keep, d, n_past):
    """The definition, on uint16 K [planes][n_ctx][D], uint16 V [planes][D][n_ctx], int32 hist [n_ctx]."""
    k, v, h, a = k.copy(), v.copy(), h.copy(), n_keep + d
    rows = k[:, a:n_past, :].copy()
    x = rows[..., :n_rot].view(np.float16).astype(np.float32)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    c, s = tab[d, :, 0], tab[d, :, 1]
    rows[..., 0:n_rot:2] = (x0 * c + x1 * s).astype(np.float16).view(np.uint16)
    rows[..., 1:n_rot:2] = (x1 * c - x0 * s).astype(np.float16).view(np.uint16)
    k[:, n_keep:n_past - d, :] = rows
    v[:, :, n_keep:n_past - d] = v[:, :, a:n_past].copy()
    h[n_keep:n_past - d] = h[a:n_past].copy()
    return k, v, h


@pytest.mark.parametrize("head_dim,n_rot,shift", CASES, ids=[f"d{h}-r{r}-k{s[0]}_d{s[1]}_p{s[2]}" for h, r, s in CASES])
def test_shift_is_exact_and_stays_in_range(gpu, head_dim, n_rot, shift):
    n_keep, d, n_past = shift
    rng = np.random.default_rng([head_dim, n_rot, n_keep, d, n_past])
    kv, g = N_PLANES * N_CTX * head_dim, PAD // 2
    # K: sign, exponent field 1..24 (2^-14 <= |x| < 2^10), any mantissa; the canaries too
    kw = (rng.integers(0, 2, kv + 2 * g) << 15 | rng.integers(1, 25, kv + 2 * g) << 10 | rng.integers(0, 1024, kv + 2 * g)).astype(np.uint16)
    vw = rng.integers(0, 65536, kv + 2 * g).astype(np.uint16)
    hw = rng.integers(-2**31, 2**31, N_CTX + PAD // 2, dtype=np.int64).astype(np.int32)
    tab = rope_table(N_CTX, n_rot)
    dk, dv, dh, dt = (to_dev(a) for a in (kw.view(np.int16), vw.view(np.int16), hw, tab))
    us = llmi.kv_shift(N_PLANES, head_dim, n_rot, N_CTX, n_keep, d, n_past, dt.data_ptr(), dk.data_ptr() + PAD,
                       dv.data_ptr() + PAD, dh.data_ptr() + PAD)
    assert (us > 0.0) == (n_keep + d < n_past)
    wk, wv, wh = kw.copy(), vw.copy(), hw.copy()  # what the allocations must hold afterwards
    k, v, h = shifted(kw[g:g + kv].reshape(N_PLANES, N_CTX, head_dim), vw[g:g + kv].reshape(N_PLANES, head_dim, N_CTX),
                      hw[PAD // 4:PAD // 4 + N_CTX], tab, n_rot, n_keep, d, n_past)
    wk[g:g + kv], wv[g:g + kv], wh[PAD // 4:PAD // 4 + N_CTX] = k.ravel(), v.ravel(), h
    for name, dev, want, g0 in (("k", dk, wk.view(np.int16), g), ("v", dv, wv.view(np.int16), g), ("hist", dh, wh, PAD // 4)):
        bad = np.flatnonzero(dev.cpu().numpy() != want)
        assert bad.size == 0, f"{name}: {bad.size} items differ, buffer items {int(bad[0]) - g0} .. {int(bad[-1]) - g0}"
