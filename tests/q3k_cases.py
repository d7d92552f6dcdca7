"""Q3_K test inputs and the two pure-NumPy references, written from the block layout alone
(ggml type 11, 110 B per 256 weights: u8 hmask[32], u8 qs[64], u8 scales[12], f16 d).

Weight n = 128 h + 32 j + l (l < 32) has low bits (qs[32 h + l] >> 2 j) & 3 and high bit
hmask[l] & (1 << (4 h + j)); its value is low - (high ? 0 : 4); its scale is number n / 16 of
the sixteen 6-bit scales (4 low bits + 2 high bits, the kmask unpack), minus 32.

  unpack(raw)      q [nb][256] in [-4, 3], sc [nb][16] in [-32, 31], d [nb] float64
  twin_q6k(raw)    the Q6_K blocks with the same d, int8 scales sc and 6-bit quants q + 32: the
                   same weights, and ggml's generic dot runs the same operations on them
  dequant_f64(raw) d * sc * q in float64
"""
from __future__ import annotations

import numpy as np

from helpers import f16_bytes

Q3_K = 11
Q3_BYTES = 110


def random_q3k(rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Uniform random bytes, fp16 d of the magnitude that gives weights of std ~0.02."""
    nb = rows * (cols // 256)
    raw = rng.integers(0, 256, size=(nb, Q3_BYTES), dtype=np.uint8)
    raw[:, 108:110] = f16_bytes(rng.uniform(2e-4, 8e-4, nb))
    return raw.reshape(-1)


def extreme_q3k(rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """random_q3k with one extreme per block, by block number mod 8: scales all 0 (-32), scales
    all 63 (+31), hmask all zero (every q - 4), hmask all one, qs 0xFF, d = 0, d negative, and
    scales 63 + hmask zero + qs 0 (every product scale * q = 31 * -4) in turn."""
    raw = random_q3k(rows, cols, rng).reshape(-1, Q3_BYTES).copy()
    k = np.arange(raw.shape[0]) % 8
    raw[k == 0, 96:108] = 0x00
    raw[k == 1, 96:108] = 0xFF
    raw[k == 2, 0:32] = 0x00
    raw[k == 3, 0:32] = 0xFF
    raw[k == 4, 32:96] = 0xFF
    raw[k == 5, 108:110] = 0
    raw[k == 6, 109] |= 0x80
    raw[k == 7, 96:108] = 0xFF
    raw[k == 7, 0:96] = 0x00
    return raw.reshape(-1)


def unpack(raw: np.ndarray):
    b = np.asarray(raw, dtype=np.uint8).reshape(-1, Q3_BYTES)
    nb = b.shape[0]
    hmask, qs, scales = b[:, 0:32], b[:, 32:96], b[:, 96:108]
    j = np.arange(4).reshape(1, 1, 4, 1)
    low = (qs.reshape(nb, 2, 1, 32) >> (2 * j)) & 3                                   # [nb][h][j][l]
    high = (hmask.reshape(nb, 1, 1, 32) >> (4 * np.arange(2).reshape(1, 2, 1, 1) + j)) & 1
    q = (low.astype(np.int64) - 4 * (1 - high.astype(np.int64))).reshape(nb, 256)
    lo4 = np.concatenate([scales[:, 0:8] & 15, scales[:, 0:8] >> 4], axis=1)           # scales 0..7, 8..15
    hi2 = np.stack([(scales[:, 8 + i % 4] >> (2 * (i // 4))) & 3 for i in range(16)], axis=1)
    sc = (lo4 | (hi2 << 4)).astype(np.int64) - 32
    d = b[:, 108:110].copy().view(np.float16).reshape(nb).astype(np.float64)
    return q, sc, d


def twin_q6k(raw: np.ndarray) -> np.ndarray:
    q, sc, _ = unpack(raw)
    nb = q.shape[0]
    # Q6_K element 128 n + 32 k + l: k = 0, 1 the low nibbles of ql[64 n + 32 k + l], k = 2, 3 the
    # high nibbles of ql[64 n + 32 (k - 2) + l]; bits 2 k of qh[32 n + l]
    q6 = (q + 32).reshape(nb, 2, 4, 32)
    out = np.zeros((nb, 210), dtype=np.uint8)
    out[:, 0:128] = ((q6[:, :, 0:2, :] & 15) | ((q6[:, :, 2:4, :] & 15) << 4)).astype(np.uint8).reshape(nb, 128)
    qh = np.zeros((nb, 2, 32), dtype=np.uint8)
    for k in range(4):
        qh |= ((q6[:, :, k, :] >> 4) & 3).astype(np.uint8) << (2 * k)
    out[:, 128:192] = qh.reshape(nb, 64)
    out[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    out[:, 208:210] = np.asarray(raw, dtype=np.uint8).reshape(nb, Q3_BYTES)[:, 108:110]
    return out.reshape(-1)


def dequant_f64(raw: np.ndarray) -> np.ndarray:
    """[nb][256] float64 weights, (d * scale) * q as ggml's dequantize_row_q3_K associates it
    (a zero q under a negative d * scale is -0.0, as there)."""
    q, sc, d = unpack(raw)
    return (d[:, None] * np.repeat(sc, 16, axis=1).astype(np.float64)) * q.astype(np.float64)
