"""Decode attention at kernel level: every single-sequence path (llmi_attention, modes 0..7)
and every batched path (llmi_battention) against the NumPy restatement of the oracle's
attn_head (ref_pf_attention of test_gpu_pf_attention.py, pinned there to the oracle's expf),
bit for bit, for every GQA group (1, 2, 4, 8), both head dims, the 2-, 4- and 8-slice
dim-split, and KV lengths on every tile, bucket and path edge.

Each case first asks llmi_attn_path which path will run and asserts it against the limits
restated here (a forced mode inside its path's limits runs that path; outside, the
documented fallback), then requires bit identity whichever path that is.

The caches hold live-like data over all of n_ctx: positions past the live edge are finite
poison, which is the engine's contract (caches are zeroed at creation, seq_rm leaves
earlier values behind).  Two data regimes:

  flat  tame K and q (score spread ~0.1): every live position has p ~ 1 / n_kv, an f16
        normal even at 8192 positions; V spans 2^-14 .. 2^14.  A position dropped or
        doubled anywhere changes the bits.
  wide  K and V over the f16 range; q built per tile or bucket edge so that the last live
        key and the first stale key are among the two to four highest scores (4 .. 13
        units above the rest, by head): an off-by-one at the live edge moves the result
        grossly either way.

test_inputs_can_see_an_off_by_one (CPU) proves that: for every case the references over
n_kv - 1, n_kv and n_kv + 1 positions differ in every head.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import llmi
from test_gpu_pf_attention import F32, _f16, ref_pf_attention

SHAPES = [(8, 8, 64), (32, 32, 128),        # G = 1
          (16, 8, 128), (8, 4, 64),         # G = 2
          (32, 8, 128),                     # G = 4
          (32, 4, 64), (64, 8, 128),        # G = 8 (4 dim slices at 64 heads)
          (128, 16, 128), (128, 32, 64)]    # 2 dim slices
REGIMES = ["flat", "wide"]
MODES = list(range(8))
N_CTX = 8448  # larger than every bucket, as in production
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025,
           2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193]
# one test per (shape, mode, regime) and length group: the reference of the longest lengths
# alone takes seconds on the widest shapes, so the lengths are split, none dropped
GROUPS = {"to1025": [n for n in LENGTHS if n <= 1025], "to4097": [n for n in LENGTHS if 1025 < n <= 4097],
          "to8193": [n for n in LENGTHS if n > 4097]}
TIGHT = (33, 256, 513, 1024, 2049, 4096)  # re-run with n_ctx == kv_bound (another V stride)
NAN_LENGTHS = (300, 511)                   # mid-bucket, and kv_bound - 1
# the wide regime's q is aimed at the positions around a bucket or tile edge: the lengths
# a - 1, a and a + 1 share one q, whose last live and first stale key are both aimed at
AIMS = [(0, 1, 2)] + [(a - 2, a - 1, a, a + 1) for a in LENGTHS[3::3]] + [(299, 300)]
_HOT = sorted({p for aim in AIMS for p in aim})


def _bound(n_kv, n_ctx):
    return min(n_ctx, (n_kv + 255) // 256 * 256)


def _slices(H, D):
    s = 2 if H >= 128 else 4 if H >= 64 else 8
    return s if D // s >= 8 else D // 8


def expected_path(H, HK, D, kvb, mode):
    """attn_path's limits (csrc/attn.hip, kernels.h), restated."""
    G = H // HK
    split_ok, fused_ok = G * kvb * 4 <= 128 * 1024, kvb <= 8192
    inside = {0: False, 1: fused_ok, 2: split_ok, 3: True, 4: G <= 8 and kvb <= 1024, 5: kvb <= 512,
              6: kvb <= 1024, 7: G <= 8}[mode]
    if inside:
        return mode
    if mode == 0:
        if G <= 8 and kvb <= 1024 and _slices(H, D) >= 2:
            return 6
        if (G == 8 and kvb > 1024) or (G <= 4 and kvb > 2048):
            return 7
        if G == 8 and D == 64 and kvb <= 256:
            return 5
        if G == 8 and fused_ok and kvb <= (2048 if D == 64 else 640):
            return 1
        if G == 4 and fused_ok and kvb <= 256:
            return 1
        if G == 4 and split_ok and kvb > 512:
            return 2
        if G <= 8 and kvb <= 1024:
            return 4
    return 2 if split_ok else 1 if fused_ok else 3


def _hadamard(n):
    h = np.ones((1, 1), F32)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


class _Data:
    """K [HK][N_CTX][D], V [HK][D][N_CTX] (f16, live-like everywhere) and q(n_kv) of one
    (shape, regime); device copies and references made on demand."""

    def __init__(self, shape, regime):
        H, HK, D = shape
        self.shape, self.regime, self.G = shape, regime, H // HK
        rng = np.random.default_rng(1000 * H + 10 * HK + D + (7 if regime == "wide" else 0))

        def wide(sh, lo, hi):
            sign = (rng.integers(0, 2, sh, dtype=np.int8) * 2 - 1).astype(F32)
            return np.exp2(rng.uniform(lo, hi, sh).astype(F32)) * sign

        self.V = _f16(wide((HK, D, N_CTX), -14, 14))
        if regime == "flat":
            self.K = _f16(rng.standard_normal((HK, N_CTX, D), dtype=F32) * F32(0.1))
            self.q0 = rng.standard_normal((H, D), dtype=F32)
        else:
            # the generator of test_gpu_pf_attention._case, with its aligned keys at the
            # positions a length can end on: mutually orthogonal sign rows, so the row a q is
            # aimed at scores scale * m * c * D and the other planted rows about zero
            self.K = _f16(wide((HK, N_CTX, D), -14, 4) * F32(0.05))
            had = _hadamard(D)
            self.rows = np.empty((HK, len(_HOT), D), F32)
            for g in range(HK):
                for i, t in enumerate(_HOT):
                    self.rows[g, i] = had[(i + g) % (D - 1) + 1]
                    self.K[g, t, :] = _f16(self.rows[g, i] * F32(0.5 + 0.0625 * (i % 3)))
            self.q0 = wide((H, D), -6, 0) * F32(0.5)
            self.c = (1.0 + 0.125 * (np.arange(H) % 8)).astype(F32)  # up to four rows of +-c each: |q| <= 2^3
        self.refs = {}
        self.dev = None

    def q(self, n_kv):
        if self.regime == "flat":
            return self.q0
        aim = self.rows[:, [_HOT.index(p) for p in self.aim(n_kv)]].sum(axis=1)  # [HK][D]
        return (self.q0 + self.c[:, None] * np.repeat(aim, self.G, axis=0)).astype(F32)

    @staticmethod
    def aim(n_kv):
        """The planted positions q(n_kv) is aimed at: the last live and the first stale among them."""
        (aim,) = [a for a in AIMS if n_kv - 1 in a and n_kv in a]
        return aim

    def ref_key(self, n_kv, n_pos):
        return (n_pos,) if self.regime == "flat" else (self.aim(n_kv), n_pos)

    def ref(self, n_kv, n_pos=None):
        """The reference of q(n_kv) over the first n_pos (default n_kv) positions."""
        n_pos = n_kv if n_pos is None else n_pos
        key = self.ref_key(n_kv, n_pos)
        if key not in self.refs:
            D = self.shape[2]
            self.refs[key] = ref_pf_attention(self.q(n_kv)[None], self.K, self.V, n_pos - 1, self.G,
                                              1.0 / np.sqrt(F32(D)))[0]
            self.refs[key].setflags(write=False)
        return self.refs[key]

    def device(self):
        from helpers import to_dev

        if self.dev is None:
            self.dev = (to_dev(self.K.view(np.uint16).reshape(-1)), to_dev(self.V.view(np.uint16).reshape(-1)))
        return self.dev


_cache: dict = {}


def _data(shape, regime) -> _Data:
    """One (shape, regime) at a time (the tests come grouped by it): the eight modes and
    three length groups share its arrays, device copies and references."""
    key = (shape, regime)
    if key not in _cache:
        _cache.clear()
        _cache[key] = _Data(shape, regime)
    return _cache[key]


def _launched(rc, where):
    """A refused launch fails the test; a device error ends the session, so that nothing
    more runs on a device that has faulted."""
    if rc != 0 and "invalid" not in llmi.last_error().lower() and "not supported" not in llmi.last_error().lower():
        pytest.exit(f"{where}: {llmi.last_error()}", returncode=3)
    assert rc == 0, f"{where}: {llmi.last_error()}"


def _attend(shape, n_kv, n_ctx, q, kd, vd, mode):
    import torch
    from helpers import to_dev

    H, HK, D = shape
    out = torch.full((H * D,), float("nan"), dtype=torch.float32, device="cuda")
    qd = to_dev(q.reshape(-1))
    rc = llmi.lib().llmi_attention(H, HK, D, n_kv, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), mode)
    _launched(rc, f"{shape} mode {mode} n_kv {n_kv} n_ctx {n_ctx}")
    return out.cpu().numpy().reshape(H, D)


def _assert_same(got, want, where):
    assert np.isfinite(want).all()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{where}: {len(bad)} of {got.size} outputs differ, heads {sorted(set(bad[:, 0].tolist()))[:8]}, "
                           f"first {bad[:3].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def _checked_path(shape, kvb, mode):
    H, HK, D = shape
    path = llmi.lib().llmi_attn_path(H, HK, D, kvb, mode)
    print(f"attn_path {shape} mode {mode} kv_bound {kvb} -> {path}")
    assert path == expected_path(H, HK, D, kvb, mode), f"{shape} mode {mode} kv_bound {kvb}: path {path}"
    return path


_MATRIX = [pytest.param(s, r, g, m, id=f"{s[0]}-{s[1]}-{s[2]}-{r}-{g}-mode{m}")
           for s in SHAPES for r in REGIMES for g in GROUPS for m in MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,regime,group,mode", _MATRIX)
def test_decode_attention_matrix(gpu, shape, regime, group, mode):
    from helpers import to_dev

    d = _data(shape, regime)
    kd, vd = d.device()
    for n_kv in GROUPS[group]:
        kvb = _bound(n_kv, N_CTX)
        path = _checked_path(shape, kvb, mode)
        want = d.ref(n_kv)
        got = _attend(shape, n_kv, N_CTX, d.q(n_kv), kd, vd, mode)
        _assert_same(got, want, f"{shape} {regime} mode {mode} (path {path}) n_kv {n_kv}")
        if n_kv in TIGHT:  # the same bucket as the whole context
            kt = to_dev(np.ascontiguousarray(d.K[:, :kvb, :]).view(np.uint16).reshape(-1))
            vt = to_dev(np.ascontiguousarray(d.V[:, :, :kvb]).view(np.uint16).reshape(-1))
            got = _attend(shape, n_kv, kvb, d.q(n_kv), kt, vt, mode)
            _assert_same(got, want, f"{shape} {regime} mode {mode} (path {path}) n_kv {n_kv} n_ctx {kvb}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 8, 64), (16, 8, 128), (32, 8, 128), (32, 4, 64)], ids=str)
@pytest.mark.parametrize("path", [1, 2, 3, 4, 5, 6, 7])
def test_decode_attention_nan_stale(gpu, shape, path):
    """NaN in every cache position past the live edge, inside the bucket and past it: a path
    that multiplies a stale value by a zero probability instead of skipping it shows NaN."""
    from helpers import to_dev

    d = _data(shape, "wide")
    n_ctx = 768
    for n_kv in NAN_LENGTHS:
        assert _checked_path(shape, _bound(n_kv, n_ctx), path) == path
        K = np.ascontiguousarray(d.K[:, :n_ctx, :])
        V = np.ascontiguousarray(d.V[:, :, :n_ctx])
        K[:, n_kv:, :] = np.nan
        V[:, :, n_kv:] = np.nan
        got = _attend(shape, n_kv, n_ctx, d.q(n_kv), to_dev(K.view(np.uint16).reshape(-1)),
                      to_dev(V.view(np.uint16).reshape(-1)), path)
        assert np.isfinite(got).all(), f"{shape} path {path} n_kv {n_kv}: a stale (NaN) position leaked into the output"
        _assert_same(got, d.ref(n_kv), f"{shape} path {path} n_kv {n_kv}, NaN stale")


def _heads_equal(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)).all(axis=1)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_inputs_can_see_an_off_by_one(shape, regime):
    """A condition on the generators above (no GPU): one position fewer or one more changes
    at least one output of every head, at every length of the matrix."""
    d = _Data(shape, regime)
    lengths = LENGTHS + list(NAN_LENGTHS)
    # the distinct references, a few at a time (NumPy releases the interpreter lock in them)
    todo = {d.ref_key(n, p): (n, p) for n in lengths for p in (n - 1, n, n + 1) if p > 0}
    with ThreadPoolExecutor(4) as pool:
        list(pool.map(lambda a: d.ref(*a), todo.values()))
    for n_kv in lengths:
        at = d.ref(n_kv)
        assert np.isfinite(at).all()
        more = d.ref(n_kv, n_kv + 1)
        same = _heads_equal(at, more)
        assert not same.any(), f"{shape} {regime} n_kv {n_kv}: heads {np.flatnonzero(same).tolist()} blind to one position more"
        if n_kv > 1:
            same = _heads_equal(at, d.ref(n_kv, n_kv - 1))
            assert not same.any(), f"{shape} {regime} n_kv {n_kv}: heads {np.flatnonzero(same).tolist()} blind to one fewer"


# ---- the batched step's attention -----------------------------------------------------------
BSHAPES = [(8, 8, 64), (16, 8, 128), (32, 8, 128), (32, 4, 64), (128, 16, 128)]
# lengths per slot: slots straddle buckets, tiles and the batch's KV bound
BCASES = {
    "1": [513],
    "2": [250, 10],
    "3": [257, 256, 255],
    "4": [1025, 3, 700, 64],
    "5": [33, 512, 1, 300, 129],
    "8": [1, 2049, 31, 256, 1024, 511, 1500, 768],
    "8short": [17, 500, 64, 1, 255, 129, 384, 33],   # bound 512: the auto slice count of > 4 slots is 1
    "2long": [4100, 17],                              # past 4096: the long path's 4-pass scores
}
V_EXP_FA = -11  # flash-attention numerics accumulate V in f16 unnormalised: 4100 * 2^3 < 65504


def _battn_path(H, HK, D, kvb, nt, forced):
    """battn_path's choice (csrc/attn.hip), restated for the record this test prints."""
    G = H // HK
    split_ok = G * kvb * 4 <= 128 * 1024
    dim_ok = G <= 8 and kvb <= 1024 and _slices(H, D) >= 2
    if (forced == 2 and split_ok) or (forced == 6 and dim_ok) or (forced == 7 and G <= 8):
        return forced
    if dim_ok and (nt <= 3 or kvb <= 512):
        return 6
    if split_ok and kvb <= (2048 if G <= 4 else 1024):
        return 2
    return 6 if dim_ok else 7 if G <= 8 else 2


class _BData:
    """One batch: per-slot q, K [nt][HK][n_ctx][D] and V [nt][HK][D][n_ctx] in the flat regime
    (every position counts), finite poison past each slot's own length."""

    def __init__(self, shape, case):
        H, HK, D = shape
        self.shape, self.lens, self.G = shape, BCASES[case], H // HK
        nt = len(self.lens)
        self.n_ctx = (max(self.lens) + 255) // 256 * 256 + 256
        rng = np.random.default_rng(77 * H + 5 * HK + D + 1000 * nt + max(self.lens))
        self.K = _f16(rng.standard_normal((nt, HK, self.n_ctx, D), dtype=F32) * F32(0.1))
        sign = (rng.integers(0, 2, (nt, HK, D, self.n_ctx), dtype=np.int8) * 2 - 1).astype(F32)
        self.V = _f16(np.exp2(rng.uniform(-14, 14, (nt, HK, D, self.n_ctx)).astype(F32)) * sign)
        self.q = rng.standard_normal((nt, H, D), dtype=F32)
        self._ref = None
        self.dev = {}

    def ref(self):
        if self._ref is None:
            D = self.shape[2]
            self._ref = np.stack([ref_pf_attention(self.q[t][None], self.K[t], self.V[t], n - 1, self.G,
                                                   1.0 / np.sqrt(F32(D)))[0] for t, n in enumerate(self.lens)])
            self._ref.setflags(write=False)
        return self._ref

    def device(self, v_exp=0):
        from helpers import to_dev

        if v_exp not in self.dev:
            V = self.V if v_exp == 0 else (self.V.astype(F32) * F32(2.0 ** v_exp)).astype(np.float16)
            if "qk" not in self.dev:
                self.dev["qk"] = (to_dev(self.q.reshape(-1)), to_dev(self.K.view(np.uint16).reshape(-1)))
            self.dev[v_exp] = to_dev(V.view(np.uint16).reshape(-1))
        return self.dev["qk"] + (self.dev[v_exp],)


def _bdata(shape, case) -> _BData:
    key = (shape, case)
    if key not in _cache:
        _cache.clear()
        _cache[key] = _BData(shape, case)
    return _cache[key]


def _battend(d, v_exp=0):
    import torch

    H, HK, D = d.shape
    nt = len(d.lens)
    qd, kd, vd = d.device(v_exp)
    out = torch.full((nt * H * D,), float("nan"), dtype=torch.float32, device="cuda")
    rc = llmi.lib().llmi_battention(H, HK, D, nt, (C.c_int32 * nt)(*d.lens), d.n_ctx, qd.data_ptr(), kd.data_ptr(),
                                    vd.data_ptr(), out.data_ptr())
    _launched(rc, f"{d.shape} slots {d.lens}")
    return out.cpu().numpy().reshape(nt, H, D)


def _bcases():
    for s in BSHAPES:
        for case in BCASES:
            if case == "2long" and s != (32, 4, 64):
                continue
            yield s, case


# (forced path, forced slices): auto, each forced path, and under the dim split every slice count
_BMODES = [(0, 0), (2, 0), (6, 0), (7, 0), (6, 1), (6, 2), (6, 4), (6, 8)]
_BMATRIX = [pytest.param(s, c, f, sl, id=f"{s[0]}-{s[1]}-{s[2]}-slots{c}-mode{f}-s{sl}")
            for s, c in _bcases() for f, sl in _BMODES
            if not sl or max(BCASES[c]) <= 1024]  # a slice count only applies to the dim split (kv_bound <= 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,case,forced,slices", _BMATRIX)
def test_battention_matrix(gpu, monkeypatch, shape, case, forced, slices):
    """Every slot of a batched launch equals its own reference, under the auto choice, each
    forced path and each slice count of the dim split."""
    d = _bdata(shape, case)
    H, HK, D = shape
    kvb = _bound(max(d.lens), d.n_ctx)
    monkeypatch.delenv("LLMI_BATTN_MODE", raising=False)
    monkeypatch.delenv("LLMI_BATTN_S", raising=False)
    if forced:
        monkeypatch.setenv("LLMI_BATTN_MODE", str(forced))
    if slices:
        monkeypatch.setenv("LLMI_BATTN_S", str(slices))
    path = _battn_path(H, HK, D, kvb, len(d.lens), forced)
    assert not slices or path == 6
    print(f"battn_path {shape} slots {d.lens} forced {forced} slices {slices or 'auto'} kv_bound {kvb} -> {path}")
    got = _battend(d)
    want = d.ref()
    for t, n in enumerate(d.lens):
        _assert_same(got[t], want[t], f"{shape} slots {d.lens} forced {forced} slices {slices} (path {path}) slot {t} n_kv {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", ["generic", "x86", "fa", "x86-fa"])
@pytest.mark.parametrize("shape,case", list(_bcases()), ids=lambda v: str(v).replace(" ", ""))
def test_battention_equals_single_launches(gpu, monkeypatch, shape, case, numerics):
    """Every slot of a batched launch equals a single-sequence launch of that slot bit for
    bit, in the generic, the x86 and the flash-attention numerics."""
    import torch

    monkeypatch.delenv("LLMI_BATTN_MODE", raising=False)
    monkeypatch.delenv("LLMI_BATTN_S", raising=False)
    d = _bdata(shape, case)
    H, HK, D = shape
    nt = len(d.lens)
    num = {"generic": llmi.NUMERICS_GENERIC, "x86": llmi.NUMERICS_X86, "fa": llmi.NUMERICS_FA,
           "x86-fa": llmi.NUMERICS_X86 | llmi.NUMERICS_FA}[numerics]
    v_exp = V_EXP_FA if num & llmi.NUMERICS_FA else 0
    qd, kd, vd = d.device(v_exp)
    kvl = HK * d.n_ctx * D
    single = torch.full((nt, H * D), float("nan"), dtype=torch.float32, device="cuda")
    old = llmi.test_option("numerics", num)
    try:
        got = _battend(d, v_exp)
        for t, n in enumerate(d.lens):
            rc = llmi.lib().llmi_attention(H, HK, D, n, d.n_ctx, qd.data_ptr() + 4 * t * H * D, kd.data_ptr() + 2 * t * kvl,
                                           vd.data_ptr() + 2 * t * kvl, single[t].data_ptr(), 0)
            assert rc == 0, llmi.last_error()
    finally:
        llmi.test_option("numerics", old)
    want = single.cpu().numpy().reshape(nt, H, D)
    for t, n in enumerate(d.lens):
        _assert_same(got[t], want[t], f"{shape} slots {d.lens} {numerics} slot {t} n_kv {n}")
