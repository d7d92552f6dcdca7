"""CPU check of the inputs of tests/test_gpu_epilogues.py (tests/epilogue_cases.py): the
REFERENCE of every (type set, shape, numerics) run on the GPU, taken over the four scale
families, lands on the edges the epilogue tests are about.  Conditions on the inputs, not
measurements of a kernel; no GPU."""
from __future__ import annotations

import numpy as np
import pytest

import epilogue_cases as ec
from helpers import QTYPES, TNAME

NUM_IDS = ["generic", "x86"]
NF = len(ec.FAMILIES)


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
@pytest.mark.parametrize("sh", ec.QKV_SHAPES, ids=lambda s: f"D{s[0]}-rot{s[1]}-{s[2]}")
@pytest.mark.parametrize("ts", ec.QKV_TYPE_SETS, ids=ec.tset_id)
def test_qkv_values_reach_every_f16_class(ts, sh, num):
    """Over the families, the values that become K and V at the positions the GPU tests run
    (row_sums asserted them finite): at least 4 each that overflow to inf, are f16 normals,
    f16 subnormals and round to zero, and at least 4 exact f16 ties -- already among the
    three single-token launches of the decode kernel, the smallest set any kernel sees."""
    c = ec.qkv_case(ts, *sh, num)
    for a in c.sums:
        assert np.isfinite(a).all()
    sets = {"decode": [(t, p) for t, p in enumerate(ec.DECODE_POS)]}
    for nt in ec.BATCH_NT[1:]:
        sets[f"batch{nt}"] = list(enumerate(ec.BATCH_POS[nt]))
    for T in ec.PREFILL_T:
        for pos0 in (0, ec.N_CTX - T):
            sets[f"prefill{T}@{pos0}"] = [(t, pos0 + t) for t in range(T)]
    for name, tp in sets.items():
        kv = [c.kv_f32(f, t, p) for f in range(NF) for t, p in tp]
        k, v = np.concatenate([a for a, _ in kv]), np.concatenate([b for _, b in kv])
        assert np.isfinite(k).all() and np.isfinite(v).all()
        for what, a in (("K", k), ("V", v)):
            counts = ec.f16_class_counts(a)
            assert min(counts) >= 4, f"{name} {what}: (inf, normal, subnormal, zero) = {counts}"
        ties = ec.f16_ties(np.concatenate([k, v]))
        assert ties >= 4, f"{name}: {ties} exact f16 ties"
    # the f16 conversion the reference uses gives inf, subnormals and zeros for them
    _, k16, v16 = c.token(0, 0, 0)
    assert k16.dtype == np.float16 and v16.dtype == np.float16


def test_tie_rows_are_ties_by_construction():
    """A tie row's sum is +-2159 * 2^(e - 4) * s in every type and numerics."""
    for ts in ec.QKV_TYPE_SETS[:4]:
        for num in (0, 1):
            c = ec.qkv_case(ts, 64, 64, 256, num)
            for r, e in ec.TIE_ROWS:
                for f, s in enumerate(ec.FAMILIES):
                    v = np.abs(c.sums[2][f, :, r].astype(np.float64))
                    assert (v == 2159.0 * 2.0 ** (e - 4) * s).all(), (TNAME[ts[0]], num, r, f, v[:3])


def test_rope_table_is_rope_norm():
    """theta by iterated f32 multiplication: pair 0 is cos / sin of the position itself, and
    position 0 is the identity rotation (K at position 0 is the bare row sum)."""
    for n_rot in (32, 64, 128):
        for base in ec.ROPE_BASES:
            tab = ec.rope_table(n_rot, base)
            assert tab.shape == (ec.N_CTX, n_rot // 2, 2) and tab.dtype == np.float32
            assert (tab[0, :, 0] == 1).all() and (tab[0, :, 1] == 0).all()
            assert np.allclose(tab[:, 0, 0], np.cos(np.arange(ec.N_CTX)), atol=1e-6)
            ts = np.float32(base) ** (np.float32(-2.0) / np.float32(n_rot))
            assert np.allclose(tab[7, 3, 1], np.sin(7.0 * float(ts) ** 3), atol=1e-5)
    v = np.arange(128, dtype=np.float32)
    assert (ec.rope_apply(v, ec.rope_table(32, 10000.0), 0, 64, 32) == v).all()
    r = ec.rope_apply(v, ec.rope_table(32, 10000.0), 9, 64, 32).reshape(2, 64)
    assert (r[:, 32:] == v.reshape(2, 64)[:, 32:]).all() and (r[:, :32] != v.reshape(2, 64)[:, :32]).any()


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
@pytest.mark.parametrize("cols", ec.SWIGLU_COLS)
@pytest.mark.parametrize("rows", ec.SWIGLU_ROWS)
@pytest.mark.parametrize("ts", ec.SWIGLU_TYPE_SETS, ids=ec.tset_id)
def test_gate_values_fill_every_expf_band(ts, rows, cols, num):
    """|g| < 88, (88.73, 103.97), (104, 133) and > 133.1 hold at least 8 gate values each,
    of both signs, over the families and the 8 tokens every kernel runs."""
    c = ec.swiglu_case(ts, rows, cols, num)
    assert np.isfinite(c.gate).all() and np.isfinite(c.up).all()
    sd = float(c.gate[1].astype(np.float64).std())
    assert 50.0 < sd < 200.0, f"family 1 gate standard deviation {sd}"
    for (lo, hi), (p, n) in zip(ec.BANDS, ec.band_counts(c.gate)):
        assert p + n >= 8 and p >= 1 and n >= 1, f"band ({lo}, {hi}): {p} positive, {n} negative"
    # the reference silu: finite, and both zero signs among its results (g / inf * u)
    assert np.isfinite(c.h).all()
    z = c.h[c.h == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
@pytest.mark.parametrize("lset", ec.LOGIT_SETS)
@pytest.mark.parametrize("rows", [33, 1001, 80, 1008])
@pytest.mark.parametrize("qtype", QTYPES, ids=[TNAME[t] for t in QTYPES])
def test_logit_sets_tie_as_claimed(qtype, rows, lset, num):
    c = ec.logit_case(qtype, rows, lset, num)
    L = c.logits
    assert np.isfinite(L).all()
    assert not (np.signbit(L) & (L == 0)).any(), "a -0 logit: the zero set must then hold both signs, -0 first"
    # the tied rows are byte copies: bit-equal logits in every family and slot; they are the
    # maximum of slot 0 in family 1, against which the set was built (a Q8_0 activation scale
    # that is an f16 subnormal reorders the logits of the smallest family)
    tied = L[:, :, list(c.tied)].view(np.uint32)
    assert (tied == tied[:, :, :1]).all()
    row = L[1, 0]
    top = np.flatnonzero(row.view(np.uint32) == row.max().view(np.uint32))
    assert tuple(top) == tuple(sorted(c.tied)), (top, c.tied)
    assert c.winner(1, 0) == min(c.tied)
    if lset in ("first_last", "pair", "boundary"):
        assert len(c.tied) == 2
    if lset == "pair":
        assert c.tied[0] % 2 == 0 and c.tied[1] == c.tied[0] + 1
    if lset == "boundary":
        assert c.tied[1] == c.tied[0] + 1 and c.tied[1] % 16 == 0
    if lset == "last":
        assert c.tied == (rows - 1,)
    if lset in ("negative", "zero_max"):
        body = np.delete(L, c.tied, axis=2) if lset == "zero_max" else L
        assert (body < 0).all(), "a pool row is not negative in every slot"
    if lset == "negative":
        assert len(c.tied) >= 2
    if lset == "zero_max":
        assert (L[:, :, list(c.tied)] == 0).all() and len(c.tied) == 3
    # every slot has its own activations, and (but for the zero set) its own winner
    if lset != "zero_max" and rows > 100:
        assert len({c.winner(1, t) for t in range(ec.LOGIT_TOKENS)}) >= 4
