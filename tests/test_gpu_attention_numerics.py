"""Attention at kernel level in the other three numerics -- the x86 association
(k_a86_h, k_a86_scores / k_a86_softmax / k_a86_pv, k_pf_a86: csrc/attn86.hip), flash
attention in the generic and in the x86 dot association (k_attn_fa, csrc/attnfa.hip;
k_pf_attn_fa, csrc/pfattnfa.hip) -- against the oracle's own attention bodies
(oracle/ggml_oracle.c or_attention: the code or_decode and or_prefill run), bit for bit on
the u32 patterns, with the shapes, lengths and one-(shape, regime)-at-a-time data cache of
test_gpu_attention.py.  There is no tolerance anywhere in this file.

The reference is pinned on the CPU first (no GPU needed):
  * or_attention equals the NumPy restatements the GPU suite already trusts
    (ref_pf_attention, _ref_attention_x86), and a NumPy restatement of the flash
    recurrence (ref_fa below), at small sizes in every data regime, and in x86 mode past
    the 8192 positions its fixed arrays used to stop at;
  * the flat and wide inputs see an off-by-one at the live edge in every head, at every
    length of the matrices, in each of the four numerics;
  * the recurrence regimes drive the branch they are meant to drive.

Data regimes (K [HK][N_CTX][D], V [HK][D][N_CTX], live-like over all of N_CTX: finite
poison past the live edge):
  flat    test_gpu_attention's: score spread ~0.1, every position counts.
  wide    test_gpu_attention's: q aimed at the positions around each length's edge.
  climb   planted K rows (two integer "digits" over the two halves of the dims, q the digit
          weights): the scores are exact and rise strictly with t over all of N_CTX.  Per
          edge segment one step > 104 (ms = expf(-step) == 0: the accumulator is wiped
          and S restarts at 1), then steps of about 1, then steps of 2^-6 .. 2^-3 up to
          the next edge (ms near 1).  Every position rescales the f16 accumulator.
  fall    the same construction falling strictly from position 0: only position 0 raises
          the maximum, vs = expf(s - M) passes through the f32 subnormals to exactly 0.
  ties    flat plus duplicated K rows at t = C j - 1 and C j for every scan chunk size C =
          1 .. 32 (C = ceil(n_kv / 256), the positions a thread of k_attn_fa owns) and
          several j: half of them rows aligned with the KV group's queries, each a new
          running maximum, so the duplicate is an equal-to-maximum score (the `else`
          branch, vs = expf(0)) on the first position of a scan chunk.
  tiny-V  wide with V in 2^-24 .. 2^-14: the f16 accumulator is subnormal or within a few
          binades of it.
In the flash numerics V is unnormalised in an f16 accumulator, |VKQ| <= sum of the
weights (each <= 1) times max |v|: flat, wide and ties scale V per length by the largest
power of two with n_kv * max |v| < 32752 (one position more still stays below 65504);
climb (sum of weights < 65, |v| <= 2^8) and fall (< 10, |v| <= 2^11) are bounded by their
step sizes.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import llmi
import pyoracle as po
from test_gpu_attention import (GROUPS, LENGTHS, N_CTX, NAN_LENGTHS, SHAPES, TIGHT, _assert_same, _attend, _bound,
                                _cache, _Data, _heads_equal, _launched)
from test_gpu_pf_attention import F32, _case, _f16, ref_pf_attention

# numerics: (the hooks' "numerics" test option, the oracle's mode flags)
NUM = {"generic": (llmi.NUMERICS_GENERIC, 0), "x86": (llmi.NUMERICS_X86, po.X86_ALL),
       "fa": (llmi.NUMERICS_FA, po.X86_FA), "x86-fa": (llmi.NUMERICS_X86 | llmi.NUMERICS_FA, po.X86_ALL | po.X86_FA)}
FA_NUMS = ("fa", "x86-fa")
KINDS = ["flat", "wide", "climb", "fall", "ties", "tiny-V"]
FA_MAX_KV = 8192   # kFaMaxKV (csrc/kernels.h)
FA_LENGTHS = [n for n in LENGTHS if n <= FA_MAX_KV]
EDGES = [0, 32, 64, 128, 256, 512, 768, 1024, 2048, 4096, 8192, N_CTX]  # the lengths' edges: climb's segments
TIE_J_MAX, TIE_J_DUP = (1, 3, 17, 200), (2, 5, 100, 255)


def _v_exp(n_kv):
    """The largest e with n_kv * 2^(14 + e) < 32752 (|v| <= 2^14 in flat, wide and ties)."""
    e = 0
    while n_kv * 2.0 ** (14 + e) >= 32752:
        e -= 1
    return e


def _climb_units():
    """N(t), in units of 2^-6 (at head_dim 64 and head factor 1), rising strictly."""
    step = np.zeros(N_CTX, np.int64)
    for e0, e1 in zip(EDGES[:-1], EDGES[1:]):
        L = e1 - e0
        p = np.arange(1, L + 1)
        s = np.where(p == 2, 160 * 64, np.where((p >= 3) & (p <= L // 2), 64, 1 + p % 8))
        t = e0 + p
        step[t[t < N_CTX]] = s[t < N_CTX]
    return np.cumsum(step)


def _fall_units():
    t = np.arange(N_CTX)
    step = np.where(t == 0, 0, np.where(t < 8, 16, np.where(t <= 40, 256, 1)))
    return step.sum() - np.cumsum(step)


class _NData(_Data):
    """_Data of test_gpu_attention in one of KINDS, with references from or_attention per
    numerics and, for the flash numerics, V scaled per length."""

    def __init__(self, shape, kind):
        super().__init__(shape, "wide" if kind in ("wide", "tiny-V") else "flat")
        H, HK, D = shape
        self.kind = kind
        rng = np.random.default_rng(31 * H + 7 * HK + D + 1000 * KINDS.index(kind))

        def wide(sh, lo, hi):
            sign = (rng.integers(0, 2, sh, dtype=np.int8) * 2 - 1).astype(F32)
            return np.exp2(rng.uniform(lo, hi, sh).astype(F32)) * sign

        if kind == "tiny-V":
            self.V = _f16(wide((HK, D, N_CTX), -24, -14))
        elif kind in ("climb", "fall"):
            N = _climb_units() if kind == "climb" else _fall_units()
            assert 0 <= N.min() and N.max() < 1 << 19
            sgn = (rng.integers(0, 2, (HK, D), dtype=np.int8) * 2 - 1).astype(F32)
            digits = np.concatenate([np.repeat((N % 1024)[:, None], D // 2, 1), np.repeat((N // 1024)[:, None], D // 2, 1)], 1)
            self.K = _f16(sgn[:, None, :] * digits[None].astype(F32))                 # integers < 2048: exact in f16
            c = (1.0 + 0.125 * (np.arange(H) % 8)).astype(F32)
            w = np.concatenate([np.full(D // 2, 2.0 ** -8, F32), np.full(D // 2, 4.0, F32)])
            self.qp = (c[:, None] * w[None, :] * np.repeat(sgn, self.G, axis=0)).astype(F32)
            self.V = _f16(wide((HK, D, N_CTX), -14, 8 if kind == "climb" else 11))
        elif kind == "ties":
            self._plant_ties()
        self.nrefs, self.vs, self.vdev, self.kdev = {}, None, None, None

    def _plant_ties(self):
        H, HK, D = self.shape
        scale = 1.0 / np.sqrt(F32(D))
        qf = _f16(self.q0).astype(np.float64).reshape(HK, self.G, D)
        m = qf.mean(axis=1)                                                   # [HK][D]
        aligned = m / (scale * (m * m).sum(axis=1, keepdims=True))            # scores about alpha in every head of the group
        top = sorted({C * j - 1 for C in range(1, 33) for j in TIE_J_MAX})
        dup = {C * j - 1 for C in range(1, 33) for j in TIE_J_DUP}
        starts = sorted(set(top) | dup)
        for t in starts:
            if t in top and t - 1 not in starts:   # (a row that is itself a duplicate stays one)
                alpha = 3.0 + 3.0 * top.index(t) / len(top)
                self.K[:, t, :] = _f16(alpha * aligned)
            self.K[:, t + 1, :] = self.K[:, t, :]

    def q(self, n_kv):
        if self.kind in ("climb", "fall"):
            return self.qp
        return super().q(n_kv)

    def v_exp(self, num, n_kv):
        return _v_exp(n_kv) if num in FA_NUMS and self.kind in ("flat", "wide", "ties") else 0

    def v_scaled(self, e):
        if e == 0:
            return self.V
        if self.vs is None or self.vs[0] != e:
            self.vs = None
            out = np.empty_like(self.V)

            def scale(g):  # (NumPy releases the interpreter lock in these)
                out[g] = (self.V[g].astype(F32) * F32(2.0 ** e)).astype(np.float16)

            with ThreadPoolExecutor(4) as pool:
                list(pool.map(scale, range(self.V.shape[0])))
            self.vs = (e, out)
        return self.vs[1]

    def nref(self, num, n_kv, n_pos=None):
        """or_attention in numerics num: q(n_kv), V as for n_kv, over the first n_pos (default n_kv) positions."""
        n_pos = n_kv if n_pos is None else n_pos
        e = self.v_exp(num, n_kv)
        key = (num, e, self.ref_key(n_kv, n_pos))
        if key not in self.nrefs:
            self.nrefs[key] = po.attention(self.q(n_kv), self.K, self.v_scaled(e), n_pos, x86=NUM[num][1])
            self.nrefs[key].setflags(write=False)
        return self.nrefs[key]

    def device_kv(self, e):
        from helpers import to_dev

        if self.kdev is None:
            self.kdev = to_dev(self.K.view(np.uint16).reshape(-1))
        if self.vdev is None or self.vdev[0] != e:
            self.vdev = None
            self.vdev = (e, to_dev(self.v_scaled(e).view(np.uint16).reshape(-1)))
        return self.kdev, self.vdev[1]


def _ndata(shape, kind) -> _NData:
    """One (shape, kind) at a time, in the cache test_gpu_attention's data shares."""
    key = ("numerics", shape, kind)
    if key not in _cache:
        _cache.clear()
        _cache[key] = _NData(shape, kind)
    return _cache[key]


# ---- the flash recurrence, restated in NumPy ---------------------------------------------------
def _expf_libm(x):
    """libm's expf, which the oracle pins llmi_expf_glibc to (test_oracle_math.py)."""
    with po.x86_mode(po.X86_LIBM):
        return np.array([po.expf(float(v)) for v in x], dtype=F32)


def _fma32(a, b, c):
    """fmaf(a, b, c) on f32 arrays: the product (<= 48 bits) is exact in double, the sum is
    rounded to odd in double (53 >= 2 * 24 + 2 bits), so the rounding to f32 is the only one."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)   # TwoSum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    with np.errstate(under="ignore"):
        return np.where((err != 0) & even, odd, s).astype(F32)


def fa_scores(q, K, n_kv, G, x86):
    """s[h][t] of the flash path: the f16 dot of K[t] with f16(q) (generic: sequential double
    sum; x86: the 4 x 8-lane fp32 chains) * (1 / sqrt(D)) + 0."""
    from test_gpu_x86 import _x86_dot

    H, D = q.shape
    qf = _f16(q).astype(F32)
    s = np.empty((H, n_kv), F32)
    for h in range(H):
        k = K[h // G, :n_kv, :].astype(F32)
        if x86:
            raw = _x86_dot(k, np.broadcast_to(qf[h], k.shape))
        else:
            raw = np.cumsum(k.astype(np.float64) * qf[h].astype(np.float64), axis=1)[:, -1].astype(F32)
        s[h] = raw * (F32(1.0) / np.sqrt(F32(D))) + F32(0.0)
    return s


def ref_fa(q, K, V, n_kv, G, x86, scores=None):
    """The one_chunk recurrence as the header of csrc/attnfa.hip states it: a loop over t,
    vectorised over heads and dims.  q [H][D] f32, K [HK][n_ctx][D], V [HK][D][n_ctx] f16."""
    H, D = q.shape
    s = fa_scores(q, K, n_kv, G, x86) if scores is None else scores
    g = np.arange(H) // G
    M, S, y = np.full(H, -np.inf, F32), np.zeros(H, F32), np.zeros((H, D), np.float16)
    one = np.ones(H, F32)
    with np.errstate(under="ignore", invalid="ignore"):
        for t in range(n_kv):
            st = s[:, t]
            new = st > M
            e = _expf_libm(np.where(new, M - st, st - M).astype(F32))
            ms, vs = np.where(new, e, one), np.where(new, one, e)
            M = np.where(new, st, M)
            y = (y.astype(F32) * ms[:, None]).astype(np.float16)          # vec_scale_f16 (by 1: exact)
            v = V[g, :, t].astype(F32)
            if x86:
                y = _fma32(v, vs[:, None], y.astype(F32)).astype(np.float16)
                S = _fma32(S, ms, vs)
            else:
                y = (y.astype(F32) + v * vs[:, None]).astype(np.float16)
                S = S * ms + vs
        S_inv = np.where(S == 0, F32(0.0), F32(1.0) / np.where(S == 0, one, S)).astype(F32)
    return y.astype(F32) * S_inv[:, None]


def _branches(s):
    """new[h][t]: position t raises the running maximum; tie[h][t]: it equals it."""
    before = np.concatenate([np.full((s.shape[0], 1), -np.inf, F32), np.maximum.accumulate(s, axis=1)[:, :-1]], axis=1)
    return s > before, s == before


# ---- CPU: the reference is pinned ----------------------------------------------------------------
SMALL = [(G * 2, 2, D) for D in (64, 128) for G in (1, 2, 4, 8)]
SMALL_LENGTHS = (1, 2, 31, 32, 33, 257)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_or_attention_equals_the_numpy_restatements(shape, kind):
    """or_attention in each of the four numerics against NumPy, bit for bit, for every (D, G)
    and data regime at lengths around the 32-position padding and past one 256-chunk.
    Independent of the oracle here: the whole arithmetic -- the f16 dots of both
    associations (ref_fa recomputes the scores itself; it shares none with the oracle), the
    softmax sums, the f16 roundings, the fma of the x86 flash form (_fma32).  Shared with
    it: expf alone (generic: expf_np, pinned by test_expf_np_matches_the_oracle; x86: the
    oracle's ggml_v_expf through po.expf; flash: libm's expf through po.expf under
    X86_LIBM, which test_oracle_math.py pins llmi_expf_glibc to)."""
    from test_gpu_x86 import _ref_attention_x86

    d = _NData(shape, kind)
    H, HK, D = shape
    scale = 1.0 / np.sqrt(F32(D))
    for n_kv in SMALL_LENGTHS:
        q = d.q(n_kv)
        want = {"generic": ref_pf_attention(q[None], d.K, d.V, n_kv - 1, d.G, scale)[0],
                "x86": _ref_attention_x86(q, d.K, d.V, n_kv, d.G, scale)}
        for num in FA_NUMS:
            want[num] = ref_fa(q, d.K, d.v_scaled(d.v_exp(num, n_kv)), n_kv, d.G, num == "x86-fa")
        for num, w in want.items():
            _assert_same(d.nref(num, n_kv), w, f"{shape} {kind} {num} n_kv {n_kv}")


@pytest.mark.parametrize("n_kv", [8193, 12000])
def test_or_attention_x86_past_8192_positions(n_kv):
    """The x86 PV dot's scratch comes from the heap, sized from n_kv: past the 8192 positions
    of the fixed arrays it replaced (where attn_head returned without writing its output)."""
    from test_gpu_x86 import _ref_attention_x86

    H, HK, D = 2, 1, 64
    rng = np.random.default_rng(n_kv)
    n_ctx = (n_kv + 255) // 256 * 256
    K = _f16(rng.standard_normal((HK, n_ctx, D)) * 0.6)
    V = _f16(rng.standard_normal((HK, D, n_ctx)))
    q = (rng.standard_normal((H, D)) * 0.8).astype(F32)
    got = po.attention(q, K, V, n_kv, x86=po.X86_ALL)
    _assert_same(got, _ref_attention_x86(q, K, V, n_kv, H // HK, 1.0 / np.sqrt(F32(D))), f"n_kv {n_kv}")


def test_or_attention_rejects_bad_arguments():
    q, K, V = np.zeros((4, 64), F32), np.zeros((2, 256, 64), np.float16), np.zeros((2, 64, 256), np.float16)
    out = np.full((4, 64), np.nan, F32)
    L = po.lib()
    for args in [(4, 2, 64, 257, 256), (4, 3, 64, 10, 256), (4, 2, 64, 0, 256), (4, 2, 48, 10, 256)]:
        assert L.or_attention(*args, po._p(q), po._p(K), po._p(V), po._p(out), 2) != 0
        assert b"or_attention" in L.or_last_error() and np.isnan(out).all()


@pytest.mark.parametrize("num", list(NUM))
@pytest.mark.parametrize("kind", ["flat", "wide"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_inputs_can_see_an_off_by_one_in_each_numerics(shape, kind, num):
    """A condition on the generators (no GPU): in numerics num, one position fewer or one
    more changes at least one output of every head, at every length of the GPU matrices."""
    d = _NData(shape, kind)
    lengths = (FA_LENGTHS if num in FA_NUMS else LENGTHS) + list(NAN_LENGTHS)
    for n_kv in lengths:   # (or_attention runs its heads in parallel itself)
        at = d.nref(num, n_kv)
        assert np.isfinite(at).all(), f"{shape} {kind} {num} n_kv {n_kv}: the reference is not finite"
        more = d.nref(num, n_kv, n_kv + 1)
        assert np.isfinite(more).all()
        same = _heads_equal(at, more)
        assert not same.any(), f"{shape} {kind} {num} n_kv {n_kv}: heads {np.flatnonzero(same).tolist()} blind to one position more"
        if n_kv > 1:
            same = _heads_equal(at, d.nref(num, n_kv, n_kv - 1))
            assert not same.any(), f"{shape} {kind} {num} n_kv {n_kv}: heads {np.flatnonzero(same).tolist()} blind to one fewer"


@pytest.mark.parametrize("x86", [0, 1], ids=["generic", "x86"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_regimes_drive_their_branches(shape, x86):
    """climb raises the maximum at all n_kv positions (with a step > 104, steps of about 1
    and small last steps), fall raises it at exactly one (with subnormal and zero vs), ties
    has in every head an equal-to-maximum position that is the first of a scan chunk: at
    every length of the flash matrix, from the scores of either association."""
    for kind in ("climb", "fall", "ties"):
        d = _NData(shape, kind)
        s = fa_scores(d.q(FA_MAX_KV), d.K, FA_MAX_KV, d.G, x86)
        new, tie = _branches(s)
        for n_kv in FA_LENGTHS:
            where = f"{shape} {kind} n_kv {n_kv}"
            if kind == "climb":
                assert new[:, :n_kv].all(), where
                step = np.diff(s[:, :n_kv].astype(np.float64), axis=1)
                if n_kv >= 3:
                    assert (step > 104).any(axis=1).all() and (_expf_libm(-step.max(axis=1).astype(F32)) == 0).all(), where
                if n_kv >= 31:
                    assert ((step > 0.5) & (step < 3.5)).any(axis=1).all() and (step[:, -1] < 0.5).all(), where
            elif kind == "fall":
                assert (new[:, :n_kv].sum(axis=1) == 1).all() and new[:, 0].all(), where
                if n_kv >= 63:
                    vs = _expf_libm((s[0, :n_kv] - s[0, 0]).astype(F32))
                    assert ((vs > 0) & (vs < 2.0 ** -126)).any() and (vs == 0).any(), where
            elif n_kv >= 2:
                C = (n_kv + 255) // 256
                first = (np.arange(n_kv) % C == 0) & (np.arange(n_kv) > 0)
                assert (tie[:, :n_kv] & first[None, :]).any(axis=1).all(), where
                assert (tie[:, :n_kv] & ~new[:, :n_kv]).sum() >= 1


# ---- GPU: flash-attention decode ------------------------------------------------------------------
class _numerics:
    def __init__(self, num):
        self.num = NUM[num][0]

    def __enter__(self):
        self.old = llmi.test_option("numerics", self.num)

    def __exit__(self, *exc):
        llmi.test_option("numerics", self.old)
        return False


def _refused(shape, n_kv, n_ctx, q, kd, vd):
    import torch
    from helpers import to_dev

    H, HK, D = shape
    out = torch.full((H * D,), float("nan"), dtype=torch.float32, device="cuda")
    qd = to_dev(q.reshape(-1))
    rc = llmi.lib().llmi_attention(H, HK, D, n_kv, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), 0)
    assert rc != 0 and "not supported" in llmi.last_error().lower(), f"{shape} n_kv {n_kv}: rc {rc}, {llmi.last_error()}"
    assert bool(torch.isnan(out).all()), f"{shape} n_kv {n_kv}: a refused launch wrote its output"


def _tight(d, e, kvb):
    from helpers import to_dev

    return (to_dev(np.ascontiguousarray(d.K[:, :kvb, :]).view(np.uint16).reshape(-1)),
            to_dev(np.ascontiguousarray(d.v_scaled(e)[:, :, :kvb]).view(np.uint16).reshape(-1)))


_FA_MATRIX = [pytest.param(s, k, g, a, id=f"{s[0]}-{s[1]}-{s[2]}-{k}-{g}-{a}")
              for s in SHAPES for k in KINDS for g in GROUPS for a in FA_NUMS]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind,group,num", _FA_MATRIX)
def test_fa_decode_matrix(gpu, shape, kind, group, num):
    """k_attn_fa in both dot associations against or_attention, at every length up to
    kFaMaxKV; past it (n_kv 8193: KV bound 8448) the launch is refused and writes nothing."""
    d = _ndata(shape, kind)
    with _numerics(num):
        for n_kv in GROUPS[group]:
            kvb = _bound(n_kv, N_CTX)
            e = d.v_exp(num, n_kv)
            kd, vd = d.device_kv(e)
            if kvb > FA_MAX_KV:
                _refused(shape, n_kv, N_CTX, d.q(n_kv), kd, vd)
                continue
            want = d.nref(num, n_kv)
            got = _attend(shape, n_kv, N_CTX, d.q(n_kv), kd, vd, 0)
            _assert_same(got, want, f"{shape} {kind} {num} n_kv {n_kv}")
            if n_kv in TIGHT:  # the same bucket as the whole context (another V stride)
                kt, vt = _tight(d, e, kvb)
                got = _attend(shape, n_kv, kvb, d.q(n_kv), kt, vt, 0)
                _assert_same(got, want, f"{shape} {kind} {num} n_kv {n_kv} n_ctx {kvb}")


NAN_SHAPES = [(8, 8, 64), (16, 8, 128), (32, 8, 128), (32, 4, 64)]


def _nan_stale(d, num, n_kv, n_ctx, mode):
    from helpers import to_dev

    K = np.ascontiguousarray(d.K[:, :n_ctx, :])
    V = np.ascontiguousarray(d.v_scaled(d.v_exp(num, n_kv))[:, :, :n_ctx])
    K[:, n_kv:, :] = np.nan
    V[:, :, n_kv:] = np.nan
    got = _attend(d.shape, n_kv, n_ctx, d.q(n_kv), to_dev(K.view(np.uint16).reshape(-1)),
                  to_dev(V.view(np.uint16).reshape(-1)), mode)
    assert np.isfinite(got).all(), f"{d.shape} {num} mode {mode} n_kv {n_kv}: a stale (NaN) position leaked into the output"
    _assert_same(got, d.nref(num, n_kv), f"{d.shape} {num} mode {mode} n_kv {n_kv}, NaN stale")


@pytest.mark.gpu
@pytest.mark.parametrize("num", FA_NUMS)
@pytest.mark.parametrize("shape", NAN_SHAPES, ids=str)
def test_fa_decode_nan_stale(gpu, shape, num):
    """NaN in every cache position past the live edge, inside the bucket and past it."""
    d = _ndata(shape, "wide")
    with _numerics(num):
        for n_kv in NAN_LENGTHS:
            _nan_stale(d, num, n_kv, 768, 0)


# ---- GPU: x86 decode ----------------------------------------------------------------------------
def expected_x86_form(kvb, mode):
    """a86_launch's limits (csrc/attn86.hip), restated: k_a86_h in pass class U = 1 / 2 / 4 / 8
    by KV bound up to 2048 positions, else (and in mode 3) the three launches (0)."""
    if mode == 3 or kvb > 2048:
        return 0
    return 1 if kvb <= 128 else 2 if kvb <= 256 else 4 if kvb <= 512 else 8


def _checked_x86_form(kvb, mode):
    form = llmi.lib().llmi_attn_x86_form(kvb, mode)
    print(f"x86 attention mode {mode} kv_bound {kvb} -> " + (f"k_a86_h U = {form}" if form else "three launches"))
    assert form == expected_x86_form(kvb, mode), f"mode {mode} kv_bound {kvb}: form {form}"
    return form


def test_x86_form_limits():
    """Host only.  (The hooks and the engine round the KV bound up to 256, so U = 1 never
    runs: its class is reachable only through a bound of 128 or less.)"""
    for kvb, form in [(1, 1), (128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 8), (2048, 8), (2049, 0), (8448, 0)]:
        assert llmi.lib().llmi_attn_x86_form(kvb, 0) == form == expected_x86_form(kvb, 0)
        assert llmi.lib().llmi_attn_x86_form(kvb, 3) == 0
    assert llmi.lib().llmi_attn_x86_form(0, 0) < 0 and "llmi_attn_x86_form" in llmi.last_error()


_X86_MATRIX = [pytest.param(s, k, g, m, id=f"{s[0]}-{s[1]}-{s[2]}-{k}-{g}-mode{m}")
               for s in SHAPES for k in ("flat", "wide") for g in GROUPS for m in (0, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind,group,mode", _X86_MATRIX)
def test_x86_decode_matrix(gpu, shape, kind, group, mode):
    """The x86 association's decode forms against or_attention at every length: one launch
    of k_a86_h up to 2048 positions (mode 0), the three launches past it and in mode 3."""
    d = _ndata(shape, kind)
    kd, vd = d.device_kv(0)
    with _numerics("x86"):
        for n_kv in GROUPS[group]:
            kvb = _bound(n_kv, N_CTX)
            form = _checked_x86_form(kvb, mode)
            want = d.nref("x86", n_kv)
            got = _attend(shape, n_kv, N_CTX, d.q(n_kv), kd, vd, mode)
            _assert_same(got, want, f"{shape} {kind} x86 mode {mode} (form {form}) n_kv {n_kv}")
            if n_kv in TIGHT:
                kt, vt = _tight(d, 0, kvb)
                got = _attend(shape, n_kv, kvb, d.q(n_kv), kt, vt, mode)
                _assert_same(got, want, f"{shape} {kind} x86 mode {mode} (form {form}) n_kv {n_kv} n_ctx {kvb}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("shape", NAN_SHAPES, ids=str)
def test_x86_decode_nan_stale(gpu, shape, mode):
    d = _ndata(shape, "wide")
    with _numerics("x86"):
        for n_kv in NAN_LENGTHS:
            _checked_x86_form(_bound(n_kv, 768), mode)
            _nan_stale(d, "x86", n_kv, 768, mode)


# ---- GPU: prefill against the reference ------------------------------------------------------------
def _rows_reference(q, K, V, pos0, flags):
    return np.stack([po.attention(q[t], K, V, pos0 + t + 1, x86=flags) for t in range(q.shape[0])])


def _decode_rows(q, kd, vd, HK, pos0, n_ctx):
    """llmi_attention (this thread's numerics, auto mode) per row of q [T][H][D]."""
    import torch
    from helpers import to_dev

    T, H, D = q.shape
    qd = to_dev(np.ascontiguousarray(q.reshape(-1)))
    out = torch.full((T, H * D), float("nan"), dtype=torch.float32, device="cuda")
    for t in range(T):
        rc = llmi.lib().llmi_attention(H, HK, D, pos0 + t + 1, n_ctx, qd.data_ptr() + 4 * t * H * D, kd.data_ptr(),
                                       vd.data_ptr(), out[t].data_ptr(), 0)
        _launched(rc, f"decode row {t}")
    return out.cpu().numpy().reshape(T, H, D)


def _pf(hook, q, kd, vd, HK, pos0, n_ctx):
    import torch
    from helpers import to_dev

    T, H, D = q.shape
    qd = to_dev(np.ascontiguousarray(q.reshape(-1)))
    out = torch.full((T * H * D,), float("nan"), dtype=torch.float32, device="cuda")
    us = getattr(llmi.lib(), hook)(H, HK, D, T, pos0, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    return us, out.cpu().numpy().reshape(T, H, D)


PF_FA_CASES = [(32, 8, 128, 64, 0, -10), (32, 8, 128, 37, 700, -10), (32, 4, 64, 40, 300, -10), (64, 8, 128, 24, 500, -10),
               (16, 8, 128, 21, 260, -10), (8, 8, 64, 70, 130, -10), (8, 8, 64, 3, 0, -10),
               (32, 8, 128, 12, 8192 - 12, -14)]   # test_gpu_fa_prefill's shapes, and its KV-limit case


@pytest.mark.gpu
@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("H,HK,D,T,pos0,v_exp", PF_FA_CASES)
def test_pf_attention_fa_vs_reference(gpu, H, HK, D, T, pos0, v_exp, assoc):
    """k_pf_attn_fa against or_attention per row (test_gpu_fa_prefill.py compares it with
    k_attn_fa alone: an error the two kernels share passes there), on that test's data."""
    from helpers import to_dev
    from test_gpu_fa_prefill import ASSOC, _tie_case

    num, flags = ASSOC[assoc]
    q, K, V, n_ctx, G = _tie_case(H, HK, D, T, pos0, seed=131 * T + pos0 + num, v_exp=v_exp)
    old = llmi.test_option("numerics", num | llmi.NUMERICS_FA)
    try:
        us, got = _pf("llmi_pf_attention_fa", q, to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1)),
                      HK, pos0, n_ctx)
    finally:
        llmi.test_option("numerics", old)
    _launched(0 if us >= 0 else int(us), f"pf fa {assoc} {(H, HK, D, T, pos0)}")
    assert np.isfinite(got).all(), "a stale (NaN) cache position leaked into the output"
    _assert_same(got, _rows_reference(q, K, V, pos0, flags | po.X86_FA), f"pf fa {assoc} {(H, HK, D, T, pos0)}")


# one case per (D, G) instantiation of k_pf_a86; T in 1, 5, 37, 70; pos0 in 0, 130, 700 (and
# others, for the remainders); (pos0 + T) % 32 in 0, 1 and 31 (the ldw and np rounding)
PF_X86_CASES = [(4, 4, 128, 1, 0), (8, 4, 128, 5, 700), (16, 4, 128, 37, 130), (32, 4, 128, 70, 0),
                (4, 4, 64, 70, 130), (8, 4, 64, 37, 700), (16, 4, 64, 5, 130), (32, 4, 64, 1, 700),
                (32, 8, 128, 37, 27), (32, 4, 64, 70, 153), (8, 8, 64, 5, 123), (16, 8, 128, 37, 186)]


def test_pf_x86_cases_cover_what_they_claim():
    assert {(D, H // HK) for H, HK, D, _, _ in PF_X86_CASES} == {(D, G) for D in (64, 128) for G in (1, 2, 4, 8)}
    assert {T for *_, T, _ in PF_X86_CASES} == {1, 5, 37, 70} and {0, 130, 700} <= {p for *_, p in PF_X86_CASES}
    assert {0, 1, 31} <= {(T + p) % 32 for *_, T, p in PF_X86_CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("H,HK,D,T,pos0", PF_X86_CASES)
def test_pf_attention_x86_vs_reference_and_decode(gpu, H, HK, D, T, pos0):
    """k_pf_a86 alone (llmi_pf_attention_x86) on _case's data, NaN in every stale position:
    each row equals or_attention in x86 mode and the decode kernel at the same position."""
    from helpers import to_dev

    q, K, V, n_ctx, G = _case(H, HK, D, T, pos0, seed=53 * T + pos0 + D + H)
    kd, vd = to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1))
    us, got = _pf("llmi_pf_attention_x86", q, kd, vd, HK, pos0, n_ctx)
    _launched(0 if us >= 0 else int(us), f"pf x86 {(H, HK, D, T, pos0)}")
    assert np.isfinite(got).all(), "a stale (NaN) cache position leaked into the output"
    _assert_same(got, _rows_reference(q, K, V, pos0, po.X86_ALL), f"pf x86 {(H, HK, D, T, pos0)} vs or_attention")
    with _numerics("x86"):
        steps = _decode_rows(q, kd, vd, HK, pos0, n_ctx)
    _assert_same(got, steps, f"pf x86 {(H, HK, D, T, pos0)} vs decode steps")


# pf_attn_x86_max_kv (csrc/attn86.hip), restated: 160 KiB less the kernel's static arrays
# (q [G][D] f32, 12 bytes per wave and head of reductions, 64 spare), over 4 G bytes per
# position, rounded down to 32
PF_X86_LIMIT = {8: 4960, 4: 10080, 2: 20320, 1: 40800}
PF_MAX_KV = 32768   # kPfAttnMaxKV: the engine's (and the hooks') longest prefill


def test_pf_attn_x86_max_kv_host_only():
    L = llmi.lib()
    for G, lim in PF_X86_LIMIT.items():
        assert L.llmi_pf_attn_x86_max_kv(G, 1, 128) == lim == ((160 * 1024 - (G * 128 * 4 + 48 * G + 64)) // (4 * G)) // 32 * 32
    assert L.llmi_pf_attn_x86_max_kv(32, 4, 64) == ((160 * 1024 - (8 * 64 * 4 + 48 * 8 + 64)) // 32) // 32 * 32
    assert L.llmi_pf_attn_x86_max_kv(32, 5, 128) < 0 and "llmi_pf_attn_x86_max_kv" in llmi.last_error()
    assert L.llmi_pf_attention_x86(32, 8, 96, 16, 0, 256, 1, 1, 1, 1) < 0 and "llmi_pf_attention_x86" in llmi.last_error()
    assert L.llmi_pf_attention_x86(32, 8, 128, 16, 250, 256, 1, 1, 1, 1) < 0
    assert L.llmi_pf_attention_x86(32, 8, 128, 16, 0, 256, None, 1, 1, 1) < 0


@pytest.mark.gpu
@pytest.mark.parametrize("G", [8, 4, 2, 1])
def test_pf_attention_x86_at_the_lds_ceiling(gpu, G):
    """T = 2 ending exactly at min(llmi_pf_attn_x86_max_kv, 32768) positions, one KV head, D =
    128: the dynamic LDS plus the kernel's static arrays come within a few dozen bytes of
    160 KiB.  The launch succeeds and matches the reference and the decode kernel; one
    position more is refused and the output keeps its fill."""
    from helpers import to_dev

    H, HK, D, T = G, 1, 128, 2
    lim = llmi.lib().llmi_pf_attn_x86_max_kv(H, HK, D)
    assert lim == PF_X86_LIMIT[G]
    end = min(lim, PF_MAX_KV)
    n_ctx = (end + 1 + 255) // 256 * 256
    rng = np.random.default_rng(900 + G)
    K = _f16(rng.standard_normal((HK, n_ctx, D), dtype=F32) * F32(0.1))
    sign = (rng.integers(0, 2, (HK, D, n_ctx), dtype=np.int8) * 2 - 1).astype(F32)
    V = _f16(np.exp2(rng.uniform(-14, 14, (HK, D, n_ctx)).astype(F32)) * sign)
    q = rng.standard_normal((T, H, D), dtype=F32)
    kd, vd = to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1))
    pos0 = end - T
    us, got = _pf("llmi_pf_attention_x86", q, kd, vd, HK, pos0, n_ctx)
    print(f"k_pf_a86 G {G}: limit {lim}, launched T {T} ending at {end}: {us}")
    _launched(0 if us >= 0 else int(us), f"pf x86 G {G} at the ceiling ({end} positions)")
    _assert_same(got, _rows_reference(q, K, V, pos0, po.X86_ALL), f"pf x86 G {G} ending at {end} vs or_attention")
    with _numerics("x86"):
        steps = _decode_rows(q, kd, vd, HK, pos0, n_ctx)
    _assert_same(got, steps, f"pf x86 G {G} ending at {end} vs decode steps")
    us, out = _pf("llmi_pf_attention_x86", q, kd, vd, HK, pos0 + 1, n_ctx)
    assert us < 0 and "llmi_pf_attention_x86" in llmi.last_error(), f"G {G}: {end + 1} positions were not refused"
    assert np.isnan(out).all(), f"G {G}: a refused launch wrote its output"
