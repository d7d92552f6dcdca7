"""Inputs and references of the batched-prefill attention matrix (tests/
test_gpu_pf_attention_edges.py on the device, tests/test_pf_attention_inputs.py for the
proof on the CPU that these inputs see the mistakes they claim to see).  No GPU needed.

Reference.  Generic numerics: the oracle's own attention body, one row at a time --
pyoracle.attention(q[t], K, V, n_kv = pos0 + t + 1, x86 = 0).  ref_pf_attention / expf_np are
its NumPy restatement (held to it bit for bit by the CPU test); `restate` is the same
restatement with one named mistake applied, which is how the inputs are proven.

Position-indexed data.  A data set (`Data`) is K, V and a query row PER POSITION: the token
at position p always asks q(p).  The reference row of position p is then independent of the
window (pos0, T) it is computed in, and one lazily filled table of reference rows per data
set serves every window of the matrix.

Regimes (one data set per (D, G, HK, regime, n_pos)):

  wide      K and V over most of the f16 range, aligned ("hot") keys every 23 positions
            whose scores stand 5 .. 25 units above the rest: p from ~1 down to f16
            subnormals and 0; q has bits below f16.
  range     scores set through dims 0, 1 (and 2 for the per-head spread) of q and K, in a
            cycle of 32 positions: w - max in (-103.98, -87.3) (e an f32 subnormal: the
            n < -126 branch of the exp), the two nearest reachable scores on each side of
            the exp's -103.97208 cut-off, w - max in -10 .. -17 (p an f16 subnormal) and
            -20 .. -80 (p = 0 with e > 0).  Every row from position RANGE_FROM on has all
            of them (test_pf_attention_inputs counts them).
  ties      KV group 0: every key equal, so every score of a row is equal; KV group 1: two
            levels, the upper in blocks that straddle every 64-position key tile edge
            (64 m - 3 .. 64 m + 2) and 20 .. 24.
  own-max   scores rise with the key position by >= 1 unit per position: row p's largest
            score is its own key p, and key p + 1 scores higher still.  A mask that drops
            the own position, or one a position too long, changes every row -- the last
            row of a window too, whose next position holds the data set's own (finite,
            live) key.
  tiny-V    V values are f16 subnormals (and +-0) of mixed signs over tame scores: outputs
            are tiny and compared as integers like everything else.

Stale positions.  `window(..., poison=)` fills the positions past pos0 + T with NaN, or with
finite poison: a key per KV group that would score above every live key (own-max: the data
set's own later keys) and V of magnitude 2^14.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
RANGE_FROM = 40           # range regime: every row at or past this position reaches every band
EXP_CUT = F32(-103.97208404541015625)
REGIMES = ("wide", "range", "ties", "own-max", "tiny-V")


def expf_np(x: np.ndarray, subnormal_branch: bool = True) -> np.ndarray:
    """include/llmi_math.h llmi_expf, vectorized (float32 ops, one rounding each).
    subnormal_branch False: the mistake of building 2^n for n < -126 like any other n (the
    exponent field wraps into the sign bit)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = x * F32(1.44269502162933349609375)
        nf = (t + F32(12582912.0)) - F32(12582912.0)
        n = np.where(np.isfinite(nf), nf, 0).astype(np.int64)
        r = x - nf * F32(0.693359375)
        r = r - nf * F32(-2.12194440e-4)
        p = np.full_like(x, F32(1.98412698e-4))
        for c in (1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5, 1.0, 1.0):
            p = p * r + F32(c)
        big = n > 127
        p = np.where(big, p * F32(2.0), p)
        n = np.where(big, n - 1, n)
        small = n < -126
        if subnormal_branch:
            nn = np.where(small, n + 126 + 127, n + 127).clip(0, 255).astype(np.uint32)
            sc = (nn << np.uint32(23)).view(F32)
            out = np.where(small, (p * sc) * F32(1.17549435e-38), p * sc)
        else:
            sc = (((n + 127) << 23) & 0xFFFFFFFF).astype(np.uint32).view(F32)
            out = p * sc
        out = np.where(x < EXP_CUT, F32(0.0), out)
        out = np.where(x > F32(88.72283935546875), F32(np.inf), out)
        out = np.where(np.isnan(x), x, out)
    return out.astype(F32)


def pf_expf_np(x: np.ndarray) -> np.ndarray:
    """csrc/prefill.hip pf_expf: llmi_expf's polynomial, the 2^n scaling as ONE correctly
    rounded ldexp (exact in double, one rounding to float32, subnormals included)."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = x * F32(1.44269502162933349609375)
        nf = (t + F32(12582912.0)) - F32(12582912.0)
        n = np.where(np.isfinite(nf), nf, 0).astype(np.int64)
        r = x - nf * F32(0.693359375)
        r = r - nf * F32(-2.12194440e-4)
        p = np.full_like(x, F32(1.98412698e-4))
        for c in (1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5, 1.0, 1.0):
            p = p * r + F32(c)
        out = np.ldexp(p.astype(np.float64), n).astype(F32)
        out = np.where(x < EXP_CUT, F32(0.0), out)
        out = np.where(x > F32(88.72283935546875), F32(np.inf), out)
        out = np.where(np.isnan(x), x, out)
    return out.astype(F32)


def _f16(a):
    return np.asarray(a, dtype=F32).astype(np.float16)


def ref_pf_attention(q, K, V, pos0, G, scale):
    """q [T][H][D] f32; K [HK][n_ctx][D] f16; V [HK][D][n_ctx] f16 -> out [T][H][D]."""
    T, H, D = q.shape
    nkv = pos0 + T
    live = np.arange(nkv)[None, :] < (pos0 + np.arange(T) + 1)[:, None]  # [T][nkv]
    out = np.empty((T, H, D), F32)
    qf = _f16(q).astype(np.float64)
    for h in range(H):
        g = h // G
        k = K[g, :nkv, :].astype(np.float64)                               # [nkv][D]
        kq = np.cumsum(qf[:, h, None, :] * k[None, :, :], axis=2)[:, :, -1]  # [T][nkv], sequential over d
        w = kq.astype(F32) * F32(scale)
        mx = np.where(live, w, F32(-np.inf)).max(axis=1)
        e = np.where(live, expf_np(w - mx[:, None]), F32(0.0))
        s = np.cumsum(e.astype(np.float64), axis=1)[:, -1]
        inv = (1.0 / s).astype(F32)
        p = _f16(e * inv[:, None]).astype(np.float64)                      # [T][nkv]
        v = V[g, :, :nkv].astype(np.float64)                               # [D][nkv]
        out[:, h, :] = np.cumsum(p[:, None, :] * v[None, :, :], axis=2)[:, :, -1].astype(F32)
    return out


# ---- the restatement with one mistake applied -------------------------------------------------
VARIANTS = ("mask_le_pos_plus_1", "mask_lt_pos", "max_over_padded_tile", "pv_to_tile_end", "kv_group_h_mod_hk",
            "subgroup_kvg_is_g", "q_not_f16", "p_not_f16", "inv_in_double", "expf_without_subnormal_branch")


def restate(q, K, V, pos0, G, scale, variant=None, TQ=64, sub=2, parts=False):
    """ref_pf_attention over the window q [T][H][D] at pos0, K / V as wide as the caller's
    cache (stale positions included: some mistakes read them), with `variant`:

      mask_le_pos_plus_1    a row's live keys end one position late
      mask_lt_pos           ... one position early (the own position dropped)
      max_over_padded_tile  the row max runs to the end of the last 64-key tile of the row's
                            query tile (TQ tokens), dead and stale keys included
      pv_to_tile_end        p is not zeroed between a row's own length and the last live
                            position of its query tile, so the V values there are not
                            multiplied away
      kv_group_h_mod_hk     head h reads KV group h % HK, not h / G
      subgroup_kvg_is_g     k_pf_attn_g<D, sub> on part of a group: workgroup g reads KV group
                            g (wrapped into the cache), not g * sub / gqa
      q_not_f16, p_not_f16  the f16 rounding of q / of p left out
      inv_in_double         p = f16((float)(e * (1 / S))) with the product in double
      expf_without_subnormal_branch   2^n built for n < -126 like any other n

    parts: also return e, p and w - max of every (row, head, key) as float32 [T][H][n] (dead keys 0).
    """
    assert variant is None or variant in VARIANTS
    T, H, D = q.shape
    HK = K.shape[0]
    n = K.shape[1]
    n_kv = pos0 + np.arange(T) + 1
    tile_end = np.minimum((np.arange(T) // TQ + 1) * TQ, T) + pos0          # the query tile's last live length
    pad_end = np.minimum((tile_end + 63) // 64 * 64, n)
    cols = np.arange(n)[None, :]
    live = cols < (n_kv + {"mask_le_pos_plus_1": 1, "mask_lt_pos": -1}.get(variant, 0))[:, None]
    mx_set = cols < pad_end[:, None] if variant == "max_over_padded_tile" else live
    pv_set = cols < tile_end[:, None] if variant == "pv_to_tile_end" else live
    out = np.empty((T, H, D), F32)
    E, P, W = (np.zeros((T, H, n), F32) for _ in range(3)) if parts else (None, None, None)
    qf = (q if variant == "q_not_f16" else _f16(q)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for h in range(H):
            g = h // G
            if variant == "kv_group_h_mod_hk":
                g = h % HK
            elif variant == "subgroup_kvg_is_g":
                g = (h // sub) % HK
            k = K[g].astype(np.float64)
            kq = np.zeros((T, n))
            for d in range(D):                                               # sequential over d
                kq += qf[:, h, d, None] * k[None, :, d]
            w = kq.astype(F32) * F32(scale)
            mx = np.where(mx_set, w, F32(-np.inf)).max(axis=1)
            ex = expf_np(w - mx[:, None], subnormal_branch=variant != "expf_without_subnormal_branch")
            e = np.where(live, ex, F32(0.0))
            s = np.cumsum(e.astype(np.float64), axis=1)[:, -1]
            ep = np.where(pv_set, ex, F32(0.0))
            if variant == "inv_in_double":
                pr = (ep.astype(np.float64) * (1.0 / s)[:, None]).astype(F32)
            else:
                pr = ep * (1.0 / s).astype(F32)[:, None]
            p = pr if variant == "p_not_f16" else _f16(pr).astype(F32)
            v = V[g].astype(np.float64)                                      # [D][n]
            acc = np.zeros((T, D))
            for j in range(int(pv_set.any(axis=0).nonzero()[0].max()) + 1):  # sequential over the positions
                acc += p[:, j, None].astype(np.float64) * v[None, :, j]
            out[:, h, :] = acc.astype(F32)
            if parts:
                E[:, h], P[:, h], W[:, h] = e, np.where(live, p, F32(0.0)), np.where(live, w - mx[:, None], F32(0.0))
    return (out, E, P, W) if parts else out


# ---- data sets -----------------------------------------------------------------------------
def _cut_keys(q0, q1, scale):
    """The range regime's cut-off keys: (K0, K1) pairs (f16) whose score w = (float)(q0 K0 +
    q1 K1) * scale is the two largest reachable values below the exp's cut-off and the two
    smallest at or above it (K1 over every f16 in +-16)."""
    k0 = np.float16(-104.0 / (float(q0) * float(scale)))
    k1 = np.arange(0x0000, 0x4C01, dtype=np.uint16).view(np.float16)          # 0 .. 16
    k1 = np.concatenate([-k1[::-1], k1])
    w = (float(q0) * float(k0) + float(q1) * k1.astype(np.float64)).astype(F32) * F32(scale)
    order = np.argsort(w, kind="stable")
    ws = w[order]
    i = int(np.searchsorted(ws, EXP_CUT, side="left"))                        # first w >= cut
    assert 2 <= i <= len(ws) - 2
    below = [order[np.flatnonzero(ws == u)[0]] for u in np.unique(ws[:i])[-2:]]
    above = [order[np.flatnonzero(ws == u)[0]] for u in np.unique(ws[i:])[:2]]
    return k0, [k1[j] for j in above], [k1[j] for j in below]


class Data:
    """One data set: K [HK][n_pos][D], V [HK][D][n_pos] (f16), q(p) per position, the lazily
    filled table of reference rows, and the windows cut from it."""

    QP = 2048  # period of the tabulated part of q

    def __init__(self, D, G, HK, regime, n_pos):
        assert regime in REGIMES
        self.D, self.G, self.HK, self.H, self.regime, self.n_pos = D, G, HK, HK * G, regime, n_pos
        self.scale = F32(1.0) / np.sqrt(F32(D))
        H = self.H
        rng = np.random.default_rng([D, G, HK, REGIMES.index(regime), n_pos])
        S = rng.choice(np.array([-1.0, 1.0], F32), (HK, D))                  # one sign pattern per KV group
        Sh = np.repeat(S, G, axis=0)                                         # [H][D]
        P = min(self.QP, n_pos)
        pos = np.arange(n_pos)

        def wide(sh, lo, hi):
            sign = (rng.integers(0, 2, sh, dtype=np.int8) * 2 - 1).astype(F32)
            return np.exp2(rng.uniform(lo, hi, sh).astype(F32)) * sign

        self.poisonV = _f16(F32(16384.0) * rng.choice(np.array([-1.0, 1.0], F32), (HK, D)))
        self.qrow = None  # optional per-position factor of q
        if regime == "wide":
            self.K = _f16(wide((HK, n_pos, D), -14, 4) * F32(0.05))
            self.V = _f16(wide((HK, D, n_pos), -14, 14))
            self.qtab = np.abs(wide((P, H, D), -6, 3)) * F32(0.5) * Sh
            hot = pos[pos % 23 == 5]
            for g in range(HK):
                c = 1.0 + 0.5 * ((hot // 23 + g) % 6)
                self.K[g, hot, :] = _f16(S[g][None, :] * c[:, None])
            self.poisonK = _f16(S * F32(64.0))
        elif regime == "range":
            q0, q1 = F32(8.0 if D == 64 else 11.3125), F32(0.0625)
            u = float(q0) * float(self.scale)                                # score units per unit of K0
            k0c, above, below = _cut_keys(q0, q1, self.scale)
            self.K = np.zeros((HK, n_pos, D), np.float16)
            for g in range(HK):
                c, blk = (pos + 7 * g) % 32, pos // 32
                x = np.zeros(n_pos)
                x = np.where((c >= 1) & (c <= 8), c * 1.0, x)
                x = np.where((c >= 9) & (c <= 18), 87.6 + 1.6 * (c - 9) + 0.1 * (blk % 8), x)
                x = np.where((c >= 23) & (c <= 27), 10.0 + 1.5 * (c - 23) + 0.1 * (blk % 8), x)
                x = np.where(c >= 28, np.choose(np.clip(c - 28, 0, 3), [20.0, 30.0, 50.0, 80.0]) + 0.1 * (blk % 8), x)
                self.K[g, :, 0] = _f16(-x / u)
                self.K[g, :, 2] = np.where((c >= 1) & (c <= 8), _f16(-0.25 * (blk % 4)), np.float16(0))
                for cc, k1 in zip((19, 20, 21, 22), above + below):
                    self.K[g, c == cc, 0] = k0c
                    self.K[g, c == cc, 1] = k1
                self.K[g, 0, :] = 0                                          # the row max of every row: w = 0
            self.V = _f16(wide((HK, D, n_pos), -4, 4))
            self.qtab = (rng.standard_normal((P, H, D)).astype(F32) * F32(0.25))  # dims 3..: K is 0 there
            self.qtab[:, :, 0], self.qtab[:, :, 1] = q0, q1
            j, g = np.arange(H) % G, np.arange(H) // G
            self.qtab[:, :, 2] = (0.5 + j / 8.0 + g / 32.0)[None, :] * (1.0 + (np.arange(P) % 5) / 8.0)[:, None]
            self.poisonK = np.zeros((HK, D), np.float16)
            self.poisonK[:, 0] = _f16(120.0 / u)
        elif regime == "ties":
            ks = _f16(S * F32(0.25))
            self.K = np.repeat(ks[:, None, :], n_pos, axis=1).copy()
            if HK > 1:
                up = ((pos + 3) % 64 < 6) & (pos >= 61) | ((pos >= 20) & (pos <= 24))
                self.K[1, up, :] = _f16(S[1] * F32(0.5))
            self.V = _f16(wide((HK, D, n_pos), -8, 8))
            self.qtab = rng.uniform(0.5, 1.5, (P, H, D)).astype(F32) * Sh
            self.poisonK = _f16(S * F32(32.0))
        elif regime == "own-max":
            self.K = _f16(rng.standard_normal((HK, n_pos, D)).astype(F32) * F32(2.0 ** -6))
            self.K[:, :, 0] = (pos % 64).astype(np.float16)[None, :]
            self.K[:, :, 1] = (pos // 64).astype(np.float16)[None, :]       # exact to 2048 blocks
            self.V = _f16(wide((HK, D, n_pos), -8, 8))
            self.qtab = rng.standard_normal((P, H, D)).astype(F32) * F32(0.5)
            j, g = np.arange(H) % G, np.arange(H) // G
            a = (1.0 + j / 16.0 + g / 64.0) / float(self.scale)             # 1 .. 2 score units per position
            self.qtab[:, :, 0] = a[None, :]
            self.qtab[:, :, 1] = 136.0 / float(self.scale)                  # a block: 136 > 63 * 2 units
            self.qrow = (1.0 + (pos % 7) / 16.0).astype(F32)
            self.poisonK = None                                              # the data set's own later keys
        else:  # tiny-V
            self.K = _f16(rng.standard_normal((HK, n_pos, D)).astype(F32) * F32(0.1))
            bits = rng.integers(0, 0x400, (HK, D, n_pos)).astype(np.uint16) | (rng.integers(0, 2, (HK, D, n_pos)).astype(np.uint16) << 15)
            self.V = bits.view(np.float16)
            self.qtab = np.abs(rng.standard_normal((P, H, D)).astype(F32)) * Sh
            self.poisonK = _f16(S * F32(32.0))
        for a in (self.K, self.V, self.qtab):
            a.setflags(write=False)
        self.rows: dict = {}

    def q(self, pos) -> np.ndarray:
        """The query rows of the tokens at positions `pos`: [len(pos)][H][D] f32."""
        pos = np.asarray(pos)
        q = self.qtab[pos % len(self.qtab)]
        if self.qrow is not None:
            q = q.copy()
            q[:, :, :2] *= self.qrow[pos][:, None, None]
        return np.ascontiguousarray(q, dtype=F32)

    def ref_row(self, p: int) -> np.ndarray:
        """The oracle's output of position p: [H][D], computed once."""
        if p not in self.rows:
            import pyoracle as po

            r = po.attention(self.q([p])[0], self.K, self.V, p + 1, x86=0, threads=min(self.H, 8))
            r.setflags(write=False)
            self.rows[p] = r
        return self.rows[p]

    def want(self, pos0, T) -> np.ndarray:
        return np.stack([self.ref_row(p) for p in range(pos0, pos0 + T)])

    def window(self, pos0, T, n_ctx, poison):
        """q [T][H][D], K [HK][n_ctx][D], V [HK][D][n_ctx] of the tokens pos0 .. pos0 + T - 1;
        positions past them hold NaN (poison "nan") or finite poison ("finite")."""
        L = pos0 + T
        assert L <= n_ctx and L <= self.n_pos and poison in ("nan", "finite")
        K = np.full((self.HK, n_ctx, self.D), np.nan, np.float16)
        V = np.full((self.HK, self.D, n_ctx), np.nan, np.float16)
        K[:, :L], V[:, :, :L] = self.K[:, :L], self.V[:, :, :L]
        if poison == "finite":
            if self.poisonK is None:
                assert n_ctx <= self.n_pos
                K[:, L:] = self.K[:, L:n_ctx]
            else:
                K[:, L:] = self.poisonK[:, None, :]
            V[:, :, L:] = self.poisonV[:, :, None]
        return self.q(np.arange(pos0, L)), K, V


_sets: dict = {}


def data(D, G, HK, regime, n_pos) -> Data:
    """The data set, built once per process (the last few kept: the tests come grouped)."""
    key = (D, G, HK, regime, n_pos)
    if key not in _sets:
        while len(_sets) >= 6:
            _sets.pop(next(iter(_sets)))
        _sets[key] = Data(*key)
    return _sets[key]
