"""Batched-prefill attention (llmi_pf_attention) on the edges of its kernels' own loops:
the tiled FP64-MFMA kernel k_pf_fa (mode 0) and the LDS kernels k_pf_attn_g / k_pf_attn
(modes 1, 2), csrc/prefill.hip.  Every output is bit-identical (uint32 views) to the
oracle's rows (tests/pf_attention_cases.py: position-indexed data sets, one table of
reference rows each; tests/test_pf_attention_inputs.py proves on the CPU what these inputs
see).  `out` carries guard rows after row T - 1 that must come back unchanged, and every
case runs with NaN and with finite, highest-scoring poison past pos0 + T.

Tiled kernel: TQ = R / G tokens per query tile (R = 64 rows, 32 in the 2xx configurations),
key tiles of 64 positions, pass 2 stepping 2, 4 or 8 tiles at a time (WV = 1, 2, 4).
  causal sweep       T = 200 at pos0 = 0: lengths 1 .. 200, the live edge crossing 64, 128,
                     192 inside a query tile; all (D, G); every pf_fa_cfg at one G per D
                     (head_dim 64 folds 440 and 441 into 420: a K / V tile has fewer 16-byte
                     pieces than 1024 threads)
  key-tile sweep     pos0 + T = 64 k - 1, 64 k, 64 k + 1 for k = 1 .. 18 (every residue of the
                     8-tile step, twice), T = min(TQ + 1, L), in a cache that ends at
                     ceil(L / 256) 256 (L = 256, 512, 768, 1024 end at the cache's end) and in
                     a larger one (another V stride); default, 410 and a WV = 2 configuration
  token counts       T = 1, TQ - 1, TQ, TQ + 1, 2 TQ, 2 TQ + 1 at pos0 = 0, 1, 63, 64, 700
  chunks             five query tiles (the last ragged) through scratch for 1, 2, 3 tiles, in
                     440 and in 220 (R = 32: pf_fa_launch sizes its check with 64 rows,
                     pf_fa_chunks divides by 32)
  past 32768         pos0 + T = 32769, 33000, 33280 = n_ctx
  regimes            every regime at L = 130 and 700, default and the PE configurations
LDS kernels: every route of launch_pf_attn's ladder, asserted through llmi_pf_attn_path
before the launch: k_pf_attn_g<D, 8 / 4 / 2> on whole groups, <D, 2> on the sub-groups of
G = 6 and 16, k_pf_attn for G = 1, 3 and mode 2; T = 300 at pos0 = 0 (per-row lengths 1 ..
300: every residue of the 32-, 256- and 8 * 256 / D-position loops), the four residues of
the row width ldw, the ceilings of the ladder (found through the hook: they follow the
kernels' static LDS) and one position past each, k_pf_attn at 32768.
"""
from __future__ import annotations

import numpy as np
import pytest

import llmi
import pf_attention_cases as pc

pytestmark = pytest.mark.gpu

INST = [(D, G) for D in (64, 128) for G in (1, 2, 4, 8)]     # k_pf_fa's instantiations
HK = 2
N_POS = 1536
POISONS = ("nan", "finite")
GUARD = 3                                                      # guard rows behind out
SENTINEL = 0x5A5A5A5A
CFGS = (441, 420, 421, 410, 220, 221, 241)


def _rows(cfg):
    """R of a pf_fa_cfg value (digits RB WV PE): 16 RB rows per workgroup."""
    return 16 * (cfg // 100)


def _tq(D, G, cfg=440):
    if D == 64 and cfg in (440, 441):
        cfg = 420
    return _rows(cfg) // G


def _launched(us, where):
    """A refused launch fails the test; a device error ends the session, so that nothing
    more runs on a device that has faulted."""
    if us < 0 and "invalid" not in llmi.last_error().lower() and "not supported" not in llmi.last_error().lower() \
            and "bad arguments" not in llmi.last_error().lower():
        pytest.exit(f"{where}: {llmi.last_error()}", returncode=3)
    assert us >= 0, f"{where}: {llmi.last_error()}"


def _launch(d, pos0, T, n_ctx, poison, mode, scratch=0):
    """One llmi_pf_attention over the window; returns (microseconds or error, out rows
    [T][H][D], guard rows as uint32)."""
    import torch
    from helpers import to_dev

    q, K, V = d.window(pos0, T, n_ctx, poison)
    H, D = d.H, d.D
    out = torch.full(((T + GUARD) * H * D,), SENTINEL, dtype=torch.int32, device="cuda")
    qd, kd, vd = to_dev(q.reshape(-1)), to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1))
    us = llmi.lib().llmi_pf_attention(H, d.HK, D, T, pos0, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                      out.data_ptr(), mode, scratch)
    o = out.cpu().numpy().view(np.uint32)
    return us, o[:T * H * D].view(np.float32).reshape(T, H, D), o[T * H * D:]


def _check(d, pos0, T, n_ctx, mode, where, scratch=0, poisons=POISONS):
    want = d.want(pos0, T)
    assert np.isfinite(want).all()
    got = None
    for poison in poisons:
        w = f"{where} D {d.D} G {d.G} {d.regime} pos0 {pos0} T {T} n_ctx {n_ctx} {poison} stale"
        us, got, guard = _launch(d, pos0, T, n_ctx, poison, mode, scratch)
        _launched(us, w)
        assert (guard == SENTINEL).all(), f"{w}: {int((guard != SENTINEL).sum())} values written behind row T - 1"
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (f"{w}: {len(bad)} of {got.size} outputs differ, rows {sorted(set(bad[:, 0].tolist()))[:8]}, heads "
                               f"{sorted(set(bad[:, 1].tolist()))[:8]}, first {bad[0].tolist()}: {got[tuple(bad[0])]!r} vs "
                               f"{want[tuple(bad[0])]!r}")
    return got


class _cfg:
    """pf_fa_cfg for the block, restored after it."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        self.old = llmi.lib().llmi_test_option(b"pf_fa_cfg", self.cfg)

    def __exit__(self, *exc):
        llmi.lib().llmi_test_option(b"pf_fa_cfg", self.old)


def _tight(L):
    return (L + 255) // 256 * 256


# ---- the tiled kernel (mode 0) -----------------------------------------------------------------
def _causal_sweep(D, G, cfg):
    for regime in ("own-max", "wide"):
        with _cfg(cfg):
            _check(pc.data(D, G, HK, regime, N_POS), 0, 200, 256, 0, f"causal sweep cfg {cfg}")


@pytest.mark.parametrize("D,G", INST)
def test_fa_causal_sweep(gpu, D, G):
    _causal_sweep(D, G, 440)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("D,G", [(64, 8), (128, 4)])
def test_fa_causal_sweep_configurations(gpu, D, G, cfg):
    """(head_dim 64 folds 441 into 420, as it does 440.)"""
    _causal_sweep(D, G, cfg)


KEY_TILE_LENGTHS = [64 * k + r for k in range(1, 19) for r in (-1, 0, 1)]


@pytest.mark.parametrize("which", ["default", "wv1", "wv2"])
@pytest.mark.parametrize("D,G", INST)
def test_fa_key_tile_sweep(gpu, D, G, which):
    # head_dim 64's default is already 420 (WV = 2): its second WV = 2 configuration is 220
    cfg = {"default": 440, "wv1": 410, "wv2": 220 if D == 64 else 420}[which]
    TQ = _tq(D, G, cfg)
    for regime in ("own-max", "wide"):
        d = pc.data(D, G, HK, regime, N_POS)
        with _cfg(cfg):
            for L in KEY_TILE_LENGTHS:
                T = min(TQ + 1, L)
                for n_ctx in (_tight(L), N_POS):
                    _check(d, L - T, T, n_ctx, 0, f"key tiles cfg {cfg} L {L}")


@pytest.mark.parametrize("D,G", INST)
def test_fa_token_count_edges(gpu, D, G):
    TQ = _tq(D, G)
    for regime in ("own-max", "wide"):
        d = pc.data(D, G, HK, regime, N_POS)
        for pos0 in (0, 1, 63, 64, 700):
            for T in sorted({1, TQ - 1, TQ, TQ + 1, 2 * TQ, 2 * TQ + 1} - {0}):
                _check(d, pos0, T, _tight(pos0 + T), 0, "token counts")


@pytest.mark.parametrize("cfg", [440, 220])
@pytest.mark.parametrize("D,G", [(128, 4), (64, 2)])
def test_fa_chunked_launches(gpu, D, G, cfg):
    """Five query tiles, the last ragged, through scratch that holds fewer: the chunks 1+1+1+1+1,
    2+2+1, 3+2 (and 4+1 in 220), the same bits as one launch and as the reference.  In 220 a
    query tile has 32 rows, so the 64 rows pf_fa_launch insists on hold two of them."""
    R = _rows(cfg)
    TQ = R // G
    pos0, T = 300, 4 * TQ + TQ // 2 + 1
    ldw = (pos0 + T + 63) // 64 * 64
    tile = HK * R * ldw * 4                                   # one query tile of this configuration
    for regime in ("own-max", "wide"):
        d = pc.data(D, G, HK, regime, N_POS)
        with _cfg(cfg):
            whole = _check(d, pos0, T, 512, 0, f"cfg {cfg} one launch")
            for ntile in (1, 2, 3, 4):
                scratch = ntile * tile
                if scratch < HK * 64 * ldw * 4:
                    continue                                   # below one 64-row tile: refused (below)
                got = _check(d, pos0, T, 512, 0, f"cfg {cfg} scratch of {ntile} tiles", scratch=scratch)
                assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
            us, got, guard = _launch(d, pos0, T, 512, "nan", 0, HK * 64 * ldw * 4 - 4)
            assert us < 0 and "not supported" in llmi.last_error().lower(), "scratch below one 64-row tile was taken"
            assert (got.view(np.uint32) == SENTINEL).all() and (guard == SENTINEL).all()


@pytest.mark.parametrize("regime", ["wide", "own-max"])
@pytest.mark.parametrize("G", [1, 8])
def test_fa_past_32768(gpu, G, regime):
    """The tiled kernel runs to n_ctx wherever its scratch exists (prefill_max_kv): windows
    ending past kPfAttnMaxKV = 32768, the last at the end of the cache, scratch for two query
    tiles passed explicitly."""
    D, n_ctx = 128, 33280
    d = pc.data(D, G, 1, regime, n_ctx)
    T = 64 // G + 1
    for end in (32769, 33000, 33280):
        ldw = (end + 63) // 64 * 64
        _check(d, end - T, T, n_ctx, 0, f"past 32768, end {end}", scratch=2 * 64 * ldw * 4,
               poisons=POISONS if end < n_ctx else ("nan",))


WINDOWS = ((0, 130), (640, 60))                               # L = 130, 700


@pytest.mark.parametrize("D,G", INST)
def test_fa_regimes(gpu, D, G):
    """Every regime at L = 130 and 700: default, and 441 / 421 where e is stored by pass 2
    and read back by pass 3 instead of taken again."""
    for regime in pc.REGIMES:
        d = pc.data(D, G, HK, regime, N_POS)
        for cfg in (440, 441, 421):
            with _cfg(cfg):
                for pos0, T in WINDOWS:
                    _check(d, pos0, T, _tight(pos0 + T), 0, f"regimes cfg {cfg}")


# ---- the LDS kernels (modes 1, 2) ----------------------------------------------------------------
# (D, G, mode, the kernel launch_pf_attn takes well below every ceiling)
LDS_CASES = [(D, G, 1, G) for D in (64, 128) for G in (2, 4, 8)] + \
            [(D, 4, 2, 1) for D in (64, 128)] + \
            [(64, 1, 1, 1), (128, 1, 1, 1), (64, 3, 1, 1), (128, 3, 1, 1)] + \
            [(64, 6, 1, 2), (128, 6, 1, 2), (64, 16, 1, 2), (128, 16, 1, 2)]
_lds = pytest.mark.parametrize("D,G,mode,kernel", LDS_CASES)


def _path(H, HKV, D, max_kv, mode):
    return llmi.lib().llmi_pf_attn_path(H, HKV, D, max_kv, mode)


def _lds_check(d, pos0, T, n_ctx, mode, kernel, where, **kw):
    path = _path(d.H, d.HK, d.D, pos0 + T, mode)
    assert path == kernel, f"{where} D {d.D} G {d.G} mode {mode} max_kv {pos0 + T}: path {path}, expected {kernel}"
    return _check(d, pos0, T, n_ctx, mode, f"{where} (kernel {kernel})", **kw)


@_lds
def test_lds_causal_sweep(gpu, D, G, mode, kernel):
    for regime in ("own-max", "wide"):
        _lds_check(pc.data(D, G, HK, regime, N_POS), 0, 300, 512, mode, kernel, "LDS sweep")


@_lds
def test_lds_row_width_residues(gpu, D, G, mode, kernel):
    """ldw = (max_kv + 3) & ~3: pos0 + T = 0, 1, 2, 3 (mod 4) at pos0 > 0."""
    d = pc.data(D, G, HK, "own-max", N_POS)
    for T in (27, 28, 29, 30):
        _lds_check(d, 37, T, 256, mode, kernel, "LDS row width")


@_lds
def test_lds_regimes(gpu, D, G, mode, kernel):
    for regime in pc.REGIMES:
        d = pc.data(D, G, HK, regime, N_POS)
        for pos0, T in WINDOWS:
            _lds_check(d, pos0, T, _tight(pos0 + T), mode, kernel, "LDS regimes")


def _ceiling(G, D, kernel, lo, hi=32768):
    """The largest max_kv in lo .. hi at which G heads per KV head take `kernel` (the ladder
    is monotonic in max_kv: a kernel that no longer fits never fits again)."""
    assert _path(G, 1, D, lo, 1) == kernel
    if _path(G, 1, D, hi, 1) == kernel:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _path(G, 1, D, mid, 1) == kernel:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("gqa", [8, 4])
def test_lds_ceilings(gpu, gqa, D):
    """T = 2, one KV head, ending exactly at the last max_kv each kernel of the ladder takes
    and one position later, where the next kernel takes over; k_pf_attn at 32768, past which
    the LDS modes refuse."""
    n_pos = 33280
    d = pc.data(D, gqa, 1, "wide", n_pos)
    ladder = [g for g in (8, 4, 2) if g <= gqa]
    lo, found = 1, {}
    for kernel in ladder:
        found[kernel] = lo = _ceiling(gqa, D, kernel, lo)
        lo += 1
    print(f"k_pf_attn_g ceilings D {D} gqa {gqa}: " + ", ".join(f"<{D}, {k}> to {v}" for k, v in found.items()))
    for kernel, nxt in zip(ladder, ladder[1:] + [1]):
        top = found[kernel]
        assert top < 32768
        _lds_check(d, top - 2, 2, _tight(top + 1), 1, kernel, f"ceiling of <{D}, {kernel}>")
        _lds_check(d, top - 1, 2, _tight(top + 1), 1, nxt, f"one past the ceiling of <{D}, {kernel}>")
    _lds_check(d, 32766, 2, 33024, 1, 1, "k_pf_attn at 32768")
    assert _path(gqa, 1, D, 32769, 1) == -1 and _path(gqa, 1, D, 32769, 2) == -1
    us, got, guard = _launch(d, 32767, 2, 33024, "nan", 1)
    assert us < 0 and (got.view(np.uint32) == SENTINEL).all(), "an LDS mode took 32769 positions"
