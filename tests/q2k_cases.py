"""Q2_K test inputs and the pure-NumPy references, written from the block layout alone
(ggml type 10, 84 B per 256 weights: u8 scales[16], u8 qs[64], f16 d, f16 dmin).

Weight n = 128 k + 32 j + l (l < 32) has q = (qs[32 k + l] >> 2 j) & 3, its sub-block is n / 16,
and its value is d * (scales[n / 16] & 15) * q - dmin * (scales[n / 16] >> 4).

  unpack(raw)         q [nb][256] in [0, 3], sc and mn [nb][16] in [0, 15], d and dmin [nb] float32
  dequant_f64(raw)    [nb][256] float64 weights
  dequant_f32(raw)    the same in float32, as ggml's dequantize_row_q2_K associates it
  dot_f32(raw, img)   ggml's generic vec_dot_q2_K_q8_K against a block_q8_K activation image
                      (pyoracle.quantize_act(Q4_K, x)), in float32, block after block
"""
from __future__ import annotations

import numpy as np

from helpers import f16_bytes

Q2_K = 10
Q2_BYTES = 84


def random_q2k(rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Uniform random bytes, fp16 d and dmin of the magnitude that gives weights of std ~0.02."""
    nb = rows * (cols // 256)
    raw = rng.integers(0, 256, size=(nb, Q2_BYTES), dtype=np.uint8)
    raw[:, 80:82] = f16_bytes(rng.uniform(1e-3, 2e-3, nb))
    raw[:, 82:84] = f16_bytes(rng.uniform(1.5e-3, 3e-3, nb))
    return raw.reshape(-1)


def extreme_q2k(rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """random_q2k with one extreme per block, by block number mod 8: scales all 0x00, scales all
    0xFF, qs all 0x00, qs all 0xFF, d = 0, dmin = 0, d negative, scales 0xFF with qs 0xFF."""
    raw = random_q2k(rows, cols, rng).reshape(-1, Q2_BYTES).copy()
    k = np.arange(raw.shape[0]) % 8
    raw[k == 0, 0:16] = 0x00
    raw[k == 1, 0:16] = 0xFF
    raw[k == 2, 16:80] = 0x00
    raw[k == 3, 16:80] = 0xFF
    raw[k == 4, 80:82] = 0
    raw[k == 5, 82:84] = 0
    raw[k == 6, 81] |= 0x80
    raw[k == 7, 0:80] = 0xFF
    return raw.reshape(-1)


def unpack(raw: np.ndarray):
    b = np.asarray(raw, dtype=np.uint8).reshape(-1, Q2_BYTES)
    nb = b.shape[0]
    j = np.arange(4).reshape(1, 1, 4, 1)
    q = ((b[:, 16:80].reshape(nb, 2, 1, 32) >> (2 * j)) & 3).reshape(nb, 256).astype(np.int64)  # [nb][k][j][l]
    sc, mn = (b[:, 0:16] & 15).astype(np.int64), (b[:, 0:16] >> 4).astype(np.int64)
    d = b[:, 80:82].copy().view(np.float16).reshape(nb).astype(np.float32)
    dmin = b[:, 82:84].copy().view(np.float16).reshape(nb).astype(np.float32)
    return q, sc, mn, d, dmin


def dequant_f64(raw: np.ndarray) -> np.ndarray:
    q, sc, mn, d, dmin = unpack(raw)
    d, dmin = d.astype(np.float64)[:, None], dmin.astype(np.float64)[:, None]
    return d * np.repeat(sc, 16, axis=1) * q - dmin * np.repeat(mn, 16, axis=1)


def dequant_f32(raw: np.ndarray) -> np.ndarray:
    """dl = d * (sc & 15), ml = dmin * (sc >> 4), y = dl * q - ml, every operation in float32."""
    q, sc, mn, d, dmin = unpack(raw)
    dl = d[:, None] * np.repeat(sc, 16, axis=1).astype(np.float32)
    ml = dmin[:, None] * np.repeat(mn, 16, axis=1).astype(np.float32)
    return dl * q.astype(np.float32) - ml


def act_image(img: np.ndarray, U: int):
    """block_q8_K records (f32 d, int8 qs[256], int16 bsums[16]) -> d_a [U] f32, a [U][256], bsums [U][16]."""
    img = np.asarray(img, dtype=np.uint8).reshape(U, 292)
    da = img[:, 0:4].copy().view(np.float32).reshape(U)
    a = img[:, 4:260].copy().view(np.int8).astype(np.int64)
    bs = img[:, 260:292].copy().view(np.int16).astype(np.int64)
    return da, a, bs


def dot_f32(raw: np.ndarray, img: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """Per row, blocks in ascending order: sumf += (d_a * d) * (float)isum - (d_a * dmin) *
    (float)summs, every float operation a float32 one (NumPy float32 arrays never contract)."""
    U = cols // 256
    q, sc, mn, d, dmin = unpack(raw)
    da, a, bs = act_image(img, U)
    q, sc, mn = q.reshape(rows, U, 256), sc.reshape(rows, U, 16), mn.reshape(rows, U, 16)
    d, dmin = d.reshape(rows, U), dmin.reshape(rows, U)
    isum = ((q * a[None]).reshape(rows, U, 16, 16).sum(axis=3) * sc).sum(axis=2)   # int64, exact
    summs = (mn * bs[None]).sum(axis=2)
    assert np.abs(isum).max() < 2 ** 24 and np.abs(summs).max() < 2 ** 24      # (float) is exact
    sumf = np.zeros(rows, dtype=np.float32)
    for u in range(U):
        dall, dmn = da[u] * d[:, u], da[u] * dmin[:, u]
        sumf = sumf + (dall * isum[:, u].astype(np.float32) - dmn * summs[:, u].astype(np.float32))
    return sumf
