"""llmi.embedding.normalize against a plain-Python restatement of upstream's
common_embd_normalize: the squares in f32, their sum in double in index order, the norm
rounded to f32, the products in f32."""
from __future__ import annotations

import math
import struct

import numpy as np
import pytest

from llmi.embedding import normalize


def f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def reference(v) -> list[float]:
    total = 0.0
    for x in v:
        total += f32(float(x) * float(x))  # the product of two f32 rounds once to f32
    norm = f32(1.0 / math.sqrt(total)) if total > 0.0 else 0.0
    return [f32(float(x) * norm) for x in v]


@pytest.mark.parametrize("n,scale,seed", [(1, 1.0, 0), (7, 1.0, 1), (256, 1e-3, 2), (1024, 37.0, 3), (4096, 1.0, 4)])
def test_euclidean_matches_the_loop(n, scale, seed):
    v = (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)
    got = normalize(v)
    want = np.array(reference(v), dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(normalize(v, 2).view(np.uint32), got.view(np.uint32))
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-6


def test_zero_vector_gives_zeros():
    got = normalize(np.zeros(16, dtype=np.float32))
    assert np.array_equal(got, np.zeros(16, dtype=np.float32))


def test_minus_one_is_the_identity():
    v = np.random.default_rng(5).standard_normal(33).astype(np.float32)
    got = normalize(v, -1)
    assert np.array_equal(got.view(np.uint32), v.view(np.uint32)) and got is not v


@pytest.mark.parametrize("bad", [3, 0, 1])
def test_other_norms_raise(bad):
    with pytest.raises(ValueError):
        normalize(np.ones(4, dtype=np.float32), bad)
