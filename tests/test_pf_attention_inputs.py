"""The inputs of the batched-prefill attention matrix (tests/pf_attention_cases.py), proven
without a GPU:

  * the reference the matrix compares with -- pyoracle.attention, one row at a time -- equals
    the NumPy restatement (ref_pf_attention, restate) bit for bit on every regime;
  * the `range` regime reaches what it claims, counted per row and head through the
    restatement: e that are f32 subnormals, e zeroed by the exp's cut-off and e just above
    it (one float32 step on each side), p that are f16 subnormals, p = 0 with e > 0;
  * pf_expf (k_pf_fa's exp, csrc/prefill.hip: llmi_expf with the 2^n scaling as one
    ldexp) restated with a correctly rounded ldexp equals llmi_expf's restatement on EVERY
    float32 in [-104.5, -87] and [88, 89.5] -- the claim of the kernel's comment;
  * every mistake of pf_attention_cases.VARIANTS changes the result of a named case.
"""
from __future__ import annotations

import numpy as np
import pytest

import pf_attention_cases as pc
from pf_attention_cases import F32

SHAPES = [(64, 1), (64, 2), (64, 4), (64, 8), (128, 1), (128, 2), (128, 4), (128, 8), (64, 3), (128, 6), (64, 16)]


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("regime", pc.REGIMES)
@pytest.mark.parametrize("D,G", [(64, 2), (128, 4), (64, 3), (128, 1)])
def test_oracle_rows_equal_the_restatement(D, G, regime):
    """Windows at the start of the cache and across the first key-tile edge, both kinds of
    stale data: the oracle's rows (which never see the stale positions) are the restatement's."""
    d = pc.data(D, G, 2, regime, 256)
    for pos0, T, poison in ((0, 37, "nan"), (45, 40, "finite")):
        q, K, V = d.window(pos0, T, 256, poison)
        want = d.want(pos0, T)
        assert np.isfinite(want).all()
        assert _same(pc.restate(q, K, V, pos0, G, d.scale), want), (regime, D, G, pos0, T, poison)
        assert _same(pc.ref_pf_attention(q, K, V, pos0, G, d.scale), want), (regime, D, G, pos0, T, poison)


def test_reference_rows_do_not_depend_on_the_window():
    d = pc.data(64, 2, 2, "own-max", 256)
    a = d.want(0, 100)
    q, K, V = d.window(60, 40, 256, "finite")
    assert _same(pc.restate(q, K, V, 60, 2, d.scale), a[60:])


@pytest.mark.parametrize("D,G", SHAPES)
def test_range_regime_reaches_its_bands(D, G):
    L = 130
    d = pc.data(D, G, 2, "range", 256)
    q, K, V = d.window(0, L, 256, "finite")
    out, E, P, W = pc.restate(q, K, V, 0, G, d.scale, parts=True)
    assert np.isfinite(out).all()
    live = np.arange(256)[None, None, :] < (np.arange(L) + 1)[:, None, None]
    step = np.spacing(np.abs(pc.EXP_CUT))                      # one float32 step at the cut-off
    bands = {
        "e an f32 subnormal, w - max in (-103.98, -87.3)": (E > 0) & (E < F32(2.0 ** -126)) & (W > F32(-103.98)) & (W < F32(-87.3)),
        "e zeroed one float32 step below the cut-off": live & (W < pc.EXP_CUT) & (W >= pc.EXP_CUT - 2 * step) & (E == 0),
        "e > 0 within one float32 step above the cut-off": live & (W >= pc.EXP_CUT) & (W <= pc.EXP_CUT + 2 * step) & (E > 0),
        "p an f16 subnormal": (P > 0) & (P < F32(2.0 ** -14)),
        "p = 0 with e > 0": live & (P == 0) & (E > 0),
    }
    for name, m in bands.items():
        cnt = m.sum(axis=2)[pc.RANGE_FROM:]                     # [rows][heads]
        print(f"range D {D} G {G}: {name}: {int(cnt.min())} .. {int(cnt.max())} per row and head from position {pc.RANGE_FROM}")
        assert cnt.min() > 0, f"D {D} G {G}: no '{name}' in row {pc.RANGE_FROM + int(np.argwhere(cnt == 0)[0][0])}"
    assert bands["e an f32 subnormal, w - max in (-103.98, -87.3)"].sum(axis=2)[pc.RANGE_FROM:].min() >= 10


def _all_floats(lo, hi):
    a, b = (int(v) for v in np.array([lo, hi], F32).view(np.uint32))
    return np.arange(min(a, b), max(a, b) + 1, dtype=np.uint32).view(F32)


def test_pf_expf_equals_llmi_expf_on_every_float_of_its_edge_ranges():
    """pf_expf's one ldexp against llmi_expf's two-step scaling: every float32 in [-104.5, -87]
    (subnormal results, n < -126, and the 0 cut-off) and in [88, 89.5] (n = 128 and the
    overflow cut-off)."""
    total = 0
    for lo, hi in ((-104.5, -87.0), (88.0, 89.5)):
        x = _all_floats(lo, hi)
        want, got = pc.expf_np(x), pc.pf_expf_np(x)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        sub = int(((want > 0) & (want < F32(2.0 ** -126))).sum())
        print(f"pf_expf vs llmi_expf on [{lo}, {hi}]: {x.size} floats, {sub} subnormal results, {int((want == 0).sum())} zeros, "
              f"{int(np.isinf(want).sum())} infinities, {bad.size} differ")
        assert bad.size == 0, f"[{lo}, {hi}]: {bad.size} differ, first x = {x[bad[0]]!r}: {got[bad[0]]!r} vs {want[bad[0]]!r}"
        total += x.size
    assert total > 2_000_000
    # and a sample of everything between (normal n)
    x = np.random.default_rng(3).uniform(-104.5, 89.5, 1 << 20).astype(F32)
    assert _same(pc.pf_expf_np(x), pc.expf_np(x))


def test_expf_restatement_equals_the_oracle_at_the_edges():
    import pyoracle as po

    xs = np.concatenate([_all_floats(-103.9721, -103.9720), _all_floats(-87.3366, -87.3364), _all_floats(88.7228, 88.7229),
                         np.linspace(-104.5, -87.0, 3001).astype(F32)])
    want = np.array([po.expf(float(x)) for x in xs], dtype=F32)
    assert _same(pc.expf_np(xs), want)


# variant -> the named case that sees it: (regime, D, G, pos0, T, stale data, every row?)
SEEN_BY = {
    "mask_le_pos_plus_1": ("own-max", 128, 4, 45, 40, "finite", True),
    "mask_lt_pos": ("own-max", 128, 4, 45, 40, "finite", True),
    "max_over_padded_tile": ("wide", 64, 2, 45, 40, "finite", True),
    "pv_to_tile_end": ("ties", 128, 4, 45, 40, "finite", False),      # every row but the last of its query tile
    "kv_group_h_mod_hk": ("wide", 64, 2, 45, 40, "nan", True),
    "subgroup_kvg_is_g": ("own-max", 128, 6, 45, 40, "nan", True),
    "q_not_f16": ("wide", 64, 2, 45, 40, "nan", True),
    "p_not_f16": ("tiny-V", 64, 2, 45, 40, "nan", True),
    "inv_in_double": ("tiny-V", 64, 8, 0, 200, "nan", False),          # a few rows: one f16 step of one p
    "expf_without_subnormal_branch": ("range", 128, 4, 45, 40, "finite", True),
}


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_wrong_variant_is_seen_by_its_named_case(variant):
    regime, D, G, pos0, T, poison, every = SEEN_BY[variant]
    d = pc.data(D, G, 2, regime, 256)
    q, K, V = d.window(pos0, T, 256, poison)
    TQ = max(1, 64 // G)
    right = pc.restate(q, K, V, pos0, G, d.scale, TQ=TQ)
    assert _same(right, d.want(pos0, T))
    wrong = pc.restate(q, K, V, pos0, G, d.scale, variant, TQ=TQ)
    rows = (wrong.view(np.uint32) != right.view(np.uint32)).any(axis=(1, 2))
    heads = (wrong.view(np.uint32) != right.view(np.uint32)).any(axis=(0, 2))
    print(f"{variant}: seen by {regime} D {D} G {G} pos0 {pos0} T {T} ({poison} stale): {int(rows.sum())} of {T} rows, "
          f"{int(heads.sum())} of {2 * G} heads differ")
    assert rows.any(), f"{variant} is invisible to {SEEN_BY[variant]}"
    if every:
        assert rows.all(), f"{variant}: rows {np.flatnonzero(~rows).tolist()} of {SEEN_BY[variant]} do not see it"
    if variant == "pv_to_tile_end":
        last = (np.arange(T) % TQ == TQ - 1) | (np.arange(T) == T - 1)
        assert rows[~last].all() and not rows[last].any()
    if variant in ("mask_le_pos_plus_1", "mask_lt_pos", "q_not_f16", "p_not_f16"):
        assert heads.all()


@pytest.mark.parametrize("regime", ["own-max", "ties"])
def test_masks_are_seen_in_every_shape(regime):
    """The two off-by-one masks change every row of a window in every shape of the matrix,
    the window's last row included (its next position: live-like finite poison)."""
    for D, G in SHAPES:
        d = pc.data(D, G, 2, regime, 256)
        q, K, V = d.window(58, 12, 256, "finite")
        right = pc.restate(q, K, V, 58, G, d.scale)
        for variant in ("mask_le_pos_plus_1", "mask_lt_pos"):
            if regime == "ties" and variant == "mask_le_pos_plus_1":
                continue  # its finite poison drowns the row rather than joining the tie: seen, but not this test's point
            wrong = pc.restate(q, K, V, 58, G, d.scale, variant)
            rows = (wrong.view(np.uint32) != right.view(np.uint32)).any(axis=(1, 2))
            assert rows.all(), (regime, D, G, variant, np.flatnonzero(~rows).tolist())
