"""The edge-input builders of tests/helpers.py, checked on the CPU: this file tests the
INPUTS of tests/test_gpu_matvec_edges.py, not any kernel.

The saturated blocks are decoded here with plain numpy integer code (written from ggml's
block formats, independent of the oracle) and the integer block sums of ggml's generic
dot are formed from them: per 256-block and residue l, aux32[l] = sum over the elements e
= l (mod 8) of scale(e) * q(e) * a(e); per Q8_0 block, sumi = sum q(e) * a(e).  They must
sit exactly on the bounds the kernels' exactness argument names (prefill.hip header):
  Q4_K  15 * 63 * 127 * 32 =  3 840 480
  Q5_K  31 * 63 * 127 * 32 =  7 936 992
  Q6_K  32 * 128 * 127 * 32 = 16 646 144   (variant 0; 0.8 % below 2^24)
  Q8_0  128 * 127 * 32     =    520 192
and every reference value of every edge family must be finite in both numerics."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as po
from helpers import (BLOCK_BYTES, F16_EDGE_BITS, Q4_K, Q5_K, Q6_K, Q8_0, QTYPES, SAT_VARIANTS, SCALE_BYTES, TNAME,
                     edge_weight_sets, first_diff, near_saturated_blocks, pack_k_scales, saturated_blocks,
                     scale_edge_blocks)

IDS = [TNAME[t] for t in QTYPES]
BOUND = {(Q4_K, 0): 15 * 63 * 127 * 32, (Q5_K, 0): 31 * 63 * 127 * 32, (Q6_K, 0): 32 * 128 * 127 * 32,
         (Q6_K, 1): 31 * 127 * 127 * 32, (Q8_0, 0): 128 * 127 * 32, (Q8_0, 1): 127 * 127 * 32}


def k_scale_min(sb: np.ndarray):
    """ggml's get_scale_min_k4 over the 12 scale bytes [nb][12] -> scales, mins [nb][8]."""
    sb = sb.astype(np.int64)
    sc, mn = np.empty((sb.shape[0], 8), np.int64), np.empty((sb.shape[0], 8), np.int64)
    for j in range(8):
        if j < 4:
            sc[:, j], mn[:, j] = sb[:, j] & 63, sb[:, j + 4] & 63
        else:
            sc[:, j] = (sb[:, j + 4] & 15) | ((sb[:, j - 4] >> 6) << 4)
            mn[:, j] = (sb[:, j + 4] >> 4) | ((sb[:, j] >> 6) << 4)
    return sc, mn


def decode_int(qtype, raw):
    """(q, scale) per element as integers, [nb][block elements]: the value ggml multiplies
    the activation with is scale * q (Q6_K: q - 32 already applied; Q8_0: scale 1)."""
    b = raw.reshape(-1, BLOCK_BYTES[qtype]).astype(np.int64)
    nb = b.shape[0]
    if qtype in (Q4_K, Q5_K):
        qs = b[:, 16:144] if qtype == Q4_K else b[:, 48:176]
        q = np.empty((nb, 256), np.int64)
        for j in range(4):
            q[:, 64 * j: 64 * j + 32] = qs[:, 32 * j: 32 * j + 32] & 15
            q[:, 64 * j + 32: 64 * j + 64] = qs[:, 32 * j: 32 * j + 32] >> 4
            if qtype == Q5_K:
                qh = b[:, 16:48]
                q[:, 64 * j: 64 * j + 32] += ((qh >> (2 * j)) & 1) << 4
                q[:, 64 * j + 32: 64 * j + 64] += ((qh >> (2 * j + 1)) & 1) << 4
        sc, _ = k_scale_min(b[:, 4:16])
        return q, np.repeat(sc, 32, axis=1)
    if qtype == Q6_K:
        ql, qh = b[:, 0:128], b[:, 128:192]
        q = np.empty((nb, 256), np.int64)
        for n in range(2):
            l0, h = ql[:, 64 * n: 64 * n + 32], qh[:, 32 * n: 32 * n + 32]
            l1 = ql[:, 64 * n + 32: 64 * n + 64]
            q[:, 128 * n + 0: 128 * n + 32] = (l0 & 15) | (((h >> 0) & 3) << 4)
            q[:, 128 * n + 32: 128 * n + 64] = (l1 & 15) | (((h >> 2) & 3) << 4)
            q[:, 128 * n + 64: 128 * n + 96] = (l0 >> 4) | (((h >> 4) & 3) << 4)
            q[:, 128 * n + 96: 128 * n + 128] = (l1 >> 4) | (((h >> 6) & 3) << 4)
        sc = raw.reshape(-1, 210)[:, 192:208].copy().view(np.int8).astype(np.int64)
        return q - 32, np.repeat(sc, 16, axis=1)
    q = raw.reshape(-1, 34)[:, 2:34].copy().view(np.int8).astype(np.int64)
    return q, np.ones_like(q)


def act_int(qtype, x):
    """The q8 values of the activation the matvec of a `qtype` weight uses, [cols] int."""
    a = po.quantize_act(qtype, x)
    if qtype == Q8_0:
        return a.reshape(-1, 34)[:, 2:34].copy().view(np.int8).astype(np.int64).reshape(-1)
    return a.reshape(-1, 292)[:, 4:260].copy().view(np.int8).astype(np.int64).reshape(-1)


def block_sums(qtype, raw, rows, cols, x):
    """K-quants: aux32 [rows][blocks][8]; Q8_0: sumi [rows][blocks][1]."""
    q, s = decode_int(qtype, raw)
    a = act_int(qtype, x)
    be = q.shape[1]
    p = (q * s).reshape(rows, cols // be, be) * a.reshape(1, cols // be, be)
    if qtype == Q8_0:
        return p.sum(axis=2, keepdims=True)
    return p.reshape(rows, cols // be, be // 8, 8).sum(axis=2)


def test_pack_k_scales_round_trips():
    rng = np.random.default_rng(3)
    sc, mn = rng.integers(0, 64, (50, 8)), rng.integers(0, 64, (50, 8))
    s2, m2 = k_scale_min(pack_k_scales(sc, mn))
    assert np.array_equal(s2, sc) and np.array_equal(m2, mn)


def test_numpy_decode_agrees_with_the_oracle_on_random_blocks():
    """The independent integer decode is a decode of the same format: scale * q equals
    the oracle's dequantized value divided by d (checked with d = 1, dmin = 0)."""
    from helpers import random_blocks

    rng = np.random.default_rng(5)
    for qtype in QTYPES:
        raw = random_blocks(qtype, 3, 512, rng).reshape(-1, BLOCK_BYTES[qtype]).copy()
        one = np.array([1.0], dtype=np.float16).view(np.uint8)
        raw[:, SCALE_BYTES[qtype][0]] = one
        if len(SCALE_BYTES[qtype]) > 1:
            raw[:, SCALE_BYTES[qtype][1]] = 0
        q, s = decode_int(qtype, raw.reshape(-1))
        ref = po.dequantize(qtype, raw.reshape(-1), 3 * 512)
        assert np.array_equal((q * s).reshape(-1).astype(np.float32), ref), TNAME[qtype]


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("cols", [256, 14336])
def test_saturated_block_sums_sit_on_the_bound(qtype, cols):
    rows = 2
    for v in SAT_VARIANTS[qtype]:
        rng = np.random.default_rng(cols + qtype + v)
        raw, acts = saturated_blocks(qtype, rows, cols, v, rng)
        q, s = decode_int(qtype, raw)
        if qtype in (Q4_K, Q5_K):
            assert (q == (15 if qtype == Q4_K else 31)).all() and (s == 63).all()
            sc, mn = k_scale_min(raw.reshape(-1, BLOCK_BYTES[qtype])[:, 4:16])
            assert (mn == 63).all()
        elif qtype == Q6_K:
            assert (q == (-32 if v == 0 else 31)).all() and (s == (-128 if v == 0 else 127)).all()
        else:
            assert (q == (-128 if v == 0 else 127)).all()
        for name, make in acts:
            x = make(rng)
            assert (np.abs(act_int(qtype, x)) == 127).all(), name
            aux = block_sums(qtype, raw, rows, cols, x)
            if name == "mixed_signs":
                assert np.abs(aux).max() <= BOUND[qtype, v]
                assert len(np.unique(aux)) > 2 or cols == 256  # sums all over the range
            else:
                assert (np.abs(aux) == BOUND[qtype, v]).all(), (TNAME[qtype], v, name)
            assert np.abs(aux).max() < 2 ** 24
            for x86 in (0, po.X86_ALL):
                assert np.isfinite(po.matvec(qtype, raw, rows, cols, x, x86=x86)).all(), (TNAME[qtype], v, name, x86)


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
def test_near_saturated_aligned_block_sums_are_near_the_bound(qtype):
    """Sign-aligned: every block sum within 86 % .. 100 % of the bound (the floor: the
    smaller top quant, the smallest scale magnitude and |a| = 120 throughout), Q6_K's above
    2^23, where an f32 holds integers only; varied low bits."""
    rows, cols = 4, 1024
    rng = np.random.default_rng(19 + qtype)
    raw, acts = near_saturated_blocks(qtype, rows, cols, rng, aligned=True)
    assert acts[0][0] == "near_sat_aligned"
    floor = {Q4_K: 14 * 60, Q5_K: 30 * 60, Q6_K: 30 * 124, Q8_0: 126}[qtype] * 120 * 32
    for _ in range(3):
        x = acts[0][1](rng)
        a = np.abs(act_int(qtype, x))
        assert a.min() >= 120 and a.max() == 127
        aux = block_sums(qtype, raw, rows, cols, x)
        assert floor <= np.abs(aux).min() and np.abs(aux).max() <= BOUND[qtype, 0]
        # (q8_K maps a block's first largest |x| to -127, so same-signed Q4_K / Q5_K
        # products are all negative; the Q6_K and Q8_0 sums take both signs)
        assert (aux < 0).any() and ((aux > 0).any() or qtype in (Q4_K, Q5_K))
        assert len(np.unique(aux & 15)) >= 12
        if qtype == Q6_K:
            assert np.abs(aux).min() > 2 ** 23 and (aux & 1).any()
        for x86 in (0, po.X86_ALL):
            assert np.isfinite(po.matvec(qtype, raw, rows, cols, x, x86=x86)).all()


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
def test_near_saturated_blocks_hold_the_extreme_values(qtype):
    rows, cols = 4, 1024
    rng = np.random.default_rng(17 + qtype)
    raw, acts = near_saturated_blocks(qtype, rows, cols, rng)
    q, s = decode_int(qtype, raw)
    top = {Q4_K: 15, Q5_K: 31, Q6_K: 31, Q8_0: 127}[qtype]
    bot = {Q4_K: 0, Q5_K: 0, Q6_K: -32, Q8_0: -128}[qtype]
    assert set(np.unique(q)) == {bot, bot + 1, top - 1, top}
    if qtype in (Q4_K, Q5_K):
        sc, mn = k_scale_min(raw.reshape(-1, BLOCK_BYTES[qtype])[:, 4:16])
        assert set(np.unique(sc)) == {60, 61, 62, 63} and set(np.unique(mn)) == {60, 61, 62, 63}
    if qtype == Q6_K:
        assert set(np.unique(s)) == {124, 125, 126, 127, -128, -127, -126, -125}
    x = acts[0][1](rng)
    a = np.abs(act_int(qtype, x))
    assert a.min() >= 120 and a.max() == 127 and len(np.unique(a)) == 8
    aux = block_sums(qtype, raw, rows, cols, x)
    assert np.abs(aux).max() < 2 ** 24
    assert len(np.unique(aux & 15)) == 16  # varied low bits


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
def test_scale_edge_blocks_hold_every_edge(qtype):
    rng = np.random.default_rng(23 + qtype)
    raw, _ = scale_edge_blocks(qtype, 8, 2048, rng)
    b = raw.reshape(-1, BLOCK_BYTES[qtype])
    for sl in SCALE_BYTES[qtype]:
        bits = set(int(v) for v in b[:, sl].copy().view(np.uint16).reshape(-1))
        assert set(F16_EDGE_BITS) <= bits
        rest = np.array(sorted(bits - set(F16_EDGE_BITS)), dtype=np.uint16).view(np.float16).astype(np.float32)
        assert (rest > 0).any() and (rest < 0).any() and np.isfinite(rest).all()
    if len(SCALE_BYTES[qtype]) == 2:  # d and dmin drawn independently
        d, m = (b[:, sl].copy().view(np.uint16).reshape(-1) for sl in SCALE_BYTES[qtype])
        assert (d != m).any()


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", [(3, 256), (2, 14336)])
def test_every_edge_family_has_a_finite_reference(qtype, rows, cols):
    """The condition of the GPU comparisons: no family's reference is NaN or infinite, in
    the generic or the x86 order; and the subnormal families are not trivially zero."""
    rng = np.random.default_rng(rows + cols + qtype)
    for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
        for aname, make in acts:
            x = make(rng)
            for x86 in (0, po.X86_ALL):
                y = po.matvec(qtype, raw, rows, cols, x, x86=x86)
                assert np.isfinite(y).all(), (TNAME[qtype], wname, aname, x86)
                # (Q8_0 at 1e-35: the fp16 activation d is zero, so is the result)
                if wname == "random" and aname in ("x1e-35", "x3e-5", "x1e30", "x1e5") and (qtype, aname) != (Q8_0, "x1e-35"):
                    assert (y != 0).all(), (TNAME[qtype], aname, x86)
    assert first_diff(np.array([0.0, 1.0], np.float32), np.array([-0.0, 1.0], np.float32)).startswith("1 of 2")
    assert first_diff(np.array([0.0, 1.0], np.float32), np.array([0.0, 1.0], np.float32)) == ""
