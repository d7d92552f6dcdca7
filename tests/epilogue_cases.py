"""Inputs and references for the QKV, SwiGLU and logits epilogues at kernel level
(llmi_mv_epilogue): weights, norm weights and activations whose REFERENCE lands on the edges
the epilogues' own arithmetic has, and the NumPy restatement of each epilogue on top of the
oracle's row sums.  tests/test_epilogue_inputs.py checks the inputs on the CPU,
tests/test_gpu_epilogues.py runs them through every kernel.

  ladder weights   random_blocks with every fp16 scale of row r set to +-2^e, e cycling
                   -24..4 down the rows, the sign alternating every cycle: with the four scale
                   families the row sums overflow f16, are f16 normals, f16 subnormals and
                   round to f16 zero (below 2^-25)
  scale families   the norm weight uniform(0.5, 1.5) * s, s = 2^4, 1, 2^-8, 2^-16 (the RMSNorm
                   removes a scale put on x itself); s a power of two, so a family scales every
                   normalised activation, and its q8 scale, exactly
  tie rows         exact f16 ties cannot come from random payloads.  Every activation row
                   gets one element tuned (against the oracle's RMSNorm) so that its normalised
                   value is 127 * 2^-4 * s exactly and the maximum of its block: the q8 scale
                   of that block is then 2^-4 * s in both activation kinds and the element's
                   q8 value +-127.  A tie row is zero but for one weight of 17 (Q4_K / Q5_K: a
                   sub-block scale of 17 on a quant of 1) on that element, under d = 2^e: its
                   sum is +-2159 * 2^(e-4) * s, an odd 12-bit integer times a power of two,
                   halfway between two f16 values wherever it is an f16 normal.  V is stored
                   unrotated, and so is K at position 0 and at d >= n_rot.
  band weights     one power-of-two scale on every row, chosen against the oracle so that the
                   gate values of family 1 have a standard deviation near 100: they fill the
                   bands between llmi_expf's and x86_v_expf's switch points (88.7228, 103.972,
                   |n| > 126 at about 87.3, |n| > 192 at about 133.1), family 2^4 lies past
                   them, the small families inside
  logit sets       ties that are bit-equal by construction (rows that are byte copies of one
                   another), all-negative logits, and a maximum of zero.  Rows whose fp16
                   scales are all 0x0000 or all 0x8000 give a logit of +0 in both numerics:
                   every accumulation starts from +0 and +0 + -0 = +0, so the oracle never
                   produces a -0 logit here (test_epilogue_inputs.py asserts it) and the zero
                   set holds +0 only; argmax_key's -0 canonicalisation stays unreachable from
                   finite inputs.
  rope table       rope_norm of oracle/ggml_oracle.c: f32 theta by iterated multiplication,
                   cosf / sinf, bases 10000 and 500000

Every builder is deterministic (seeded by its arguments) and cached: a reference is computed
once and shared, read-only, by the tests that need it."""
from __future__ import annotations

import functools

import numpy as np

import pyoracle as po
from helpers import BLOCK_BYTES, BLOCK_ELEMS, Q4_K, Q5_K, Q6_K, Q8_0, SCALE_BYTES, TNAME, pack_k_scales, random_blocks

EPS = 1e-5
FAMILIES = (2.0 ** 4, 1.0, 2.0 ** -8, 2.0 ** -16)
FAMILY_IDS = ("x2^4", "x1", "x2^-8", "x2^-16")
N_CTX = 256
LADDER = tuple(range(-24, 5))
TIE_Q = 17                      # 17 * 127 = 2159: odd, 12 bits
TIE_TARGET = np.float32(127.0 / 16.0)
TIE_ROWS = ((5, 0), (6, 3))     # (row of the k / v segment, e of its d = 2^e)
ROPE_BASES = (10000.0, 500000.0)

# ---- the case matrix (test_gpu_epilogues.py parametrises over these) -----------------------
# (head_dim, n_head, n_head_kv): nq 256, nk 128 either way
HEADS = ((64, 4, 2), (128, 2, 1))
QKV_TYPE_SETS = ((Q4_K, Q4_K, Q4_K), (Q5_K, Q5_K, Q5_K), (Q6_K, Q6_K, Q6_K), (Q8_0, Q8_0, Q8_0),
                 (Q4_K, Q4_K, Q6_K), (Q8_0, Q8_0, Q6_K))
# (head_dim, n_rot, cols): cols 2048 only at head_dim 128 with n_rot = head_dim
QKV_SHAPES = tuple((d, nr, 256) for d, _, _ in HEADS for nr in (d, d // 2)) + ((128, 128, 2048),)
QKV_TOKENS = 70                 # the longest prefill; the batched kernels use the first 8
BATCH_NT = (1, 3, 5, 8)
# distinct positions with 0 and n_ctx - 1, slots 3 and 4 at one position (from nt = 5)
BATCH_POS = {1: (N_CTX - 1,), 3: (0, N_CTX - 1, 1), 5: (0, N_CTX - 1, 1, 17, 17), 8: (0, N_CTX - 1, 1, 17, 17, 100, 254, 3)}
DECODE_POS = (0, 1, N_CTX - 1)
PREFILL_T = (3, 33, 70)
SWIGLU_ROWS = (80, 272)
SWIGLU_COLS = (256, 2048)
SWIGLU_TYPE_SETS = ((Q4_K, Q4_K), (Q5_K, Q5_K), (Q6_K, Q6_K), (Q8_0, Q8_0), (Q4_K, Q6_K))
SWIGLU_TOKENS = 8
LOGIT_TOKENS = 8
LOGIT_COLS = 256
LOGIT_SETS = ("first_last", "pair", "boundary", "last", "negative", "zero_max")


def tset_id(ts):
    return TNAME[ts[0]] if len(set(ts)) == 1 else "+".join(TNAME[t] for t in sorted(set(ts), key=ts.index))


def x86_flags(num):
    return po.X86_ALL if num else 0


# ---- weights -------------------------------------------------------------------------------
def _set_scales(blocks, value):
    """Every fp16 scale of these blocks ([n][block bytes]) = value."""
    qtype = {v: k for k, v in BLOCK_BYTES.items()}[blocks.shape[-1]]
    b = np.array([value], dtype=np.float16).view(np.uint8)
    for sl in SCALE_BYTES[qtype]:
        blocks[..., sl] = b


def ladder_blocks(qtype, rows, cols, rng):
    """random_blocks with row r's fp16 scales = +-2^e, e = LADDER[r % 29], the sign flipping
    every cycle."""
    raw = random_blocks(qtype, rows, cols, rng).reshape(rows, -1, BLOCK_BYTES[qtype]).copy()
    for r in range(rows):
        sign = -1.0 if (r // len(LADDER)) & 1 else 1.0
        _set_scales(raw[r], sign * 2.0 ** LADDER[r % len(LADDER)])
    return raw.reshape(-1)


def tie_row(qtype, cols, e):
    """One row (raw bytes) that is zero but for a weight of TIE_Q on element 0, d = 2^e."""
    nb = cols // BLOCK_ELEMS[qtype]
    row = np.zeros((nb, BLOCK_BYTES[qtype]), dtype=np.uint8)
    d = np.array([2.0 ** e], dtype=np.float16).view(np.uint8)
    if qtype in (Q4_K, Q5_K):
        row[0, 0:2] = d                                   # dmin stays 0
        sc = np.zeros((1, 8), dtype=np.uint8)
        sc[0, 0] = TIE_Q
        row[0, 4:16] = pack_k_scales(sc, np.zeros((1, 8), dtype=np.uint8))
        row[0, 16 if qtype == Q4_K else 48] = 1           # element 0: the low nibble of qs[0]
    elif qtype == Q6_K:
        row[:, 128:192] = 0xAA                            # every q = 32: q - 32 = 0
        row[0, 0] = (32 + TIE_Q) & 15                     # element 0: low nibble of ql[0] ...
        row[0, 128] = 0xA8 | ((32 + TIE_Q) >> 4)          # ... and bits 0-1 of qh[0]
        row[0, 192] = 1                                   # the scale of elements 0..15
        row[0, 208:210] = d
    else:
        row[0, 0:2] = d
        row[0, 2] = TIE_Q
    return row.reshape(-1)


def with_tie_rows(qtype, raw, rows, cols):
    raw = raw.reshape(rows, -1).copy()
    for r, e in TIE_ROWS:
        raw[r] = tie_row(qtype, cols, e)
    return raw.reshape(-1)


# ---- activations and norm weights ----------------------------------------------------------
def norm_base(cols, rng):
    """uniform(0.5, 1.5); element 0 is 1, so that the tuned element's second product is exact
    (with another weight the two roundings skip the tie target about every other time)."""
    base = rng.uniform(0.5, 1.5, cols).astype(np.float32)
    base[0] = 1.0
    return base


def family_nw(base, s):
    return (base * np.float32(s)).astype(np.float32)     # exact: s is a power of two


def tuned_x(x, base):
    """x with element 0 changed until rms_norm_mul(x, base)[0] == TIE_TARGET exactly (a few
    steps of one ulp around the first estimate), the largest magnitude of the row."""
    x = x.copy()
    x[0] = np.float32(abs(x[0]) + 1.0)
    for attempt in range(1, 40):
        for _ in range(60):
            xn = po.rms_norm_mul(x, base, EPS)
            if xn[0] == TIE_TARGET:
                break
            step = x[0] * TIE_TARGET / xn[0] if abs(xn[0] / TIE_TARGET - 1) > 1e-5 else \
                np.nextafter(x[0], np.float32(np.inf if xn[0] < TIE_TARGET else -np.inf))
            x[0] = np.float32(step)
        if xn[0] == TIE_TARGET:
            break
        x[attempt] *= np.float32(1.001)  # the two roundings skip the target: another row scale
    assert xn[0] == TIE_TARGET, "no activation gives the tie target through this norm weight"
    assert np.abs(xn[1:]).max() < TIE_TARGET
    return x


def activations(n, cols, rng, base):
    return np.stack([tuned_x(rng.standard_normal(cols).astype(np.float32), base) for _ in range(n)])


def row_sums(qtype, raw, rows, cols, X, base, num):
    """[family][token][row] f32: po.matvec of the oracle's fused RMSNorm, finite."""
    out = np.empty((len(FAMILIES), X.shape[0], rows), dtype=np.float32)
    for f, s in enumerate(FAMILIES):
        nw = family_nw(base, s)
        for t in range(X.shape[0]):
            out[f, t] = po.matvec(qtype, raw, rows, cols, po.rms_norm_mul(X[t], nw, EPS), x86=x86_flags(num))
    assert np.isfinite(out).all(), "non-finite reference row sum"
    return out


# ---- rope ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rope_table(n_rot, base, n_ctx=N_CTX):
    """[n_ctx][n_rot/2][cos, sin] as rope_norm builds it: theta = pos, times theta_scale =
    powf(base, -2 / n_rot) per pair, all f32; cosf / sinf."""
    import ctypes
    import ctypes.util

    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (m.cosf, m.sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    m.powf.restype, m.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    ts = np.float32(m.powf(np.float32(base), np.float32(-2.0) / np.float32(n_rot)))
    tab = np.empty((n_ctx, n_rot // 2, 2), dtype=np.float32)
    for p in range(n_ctx):
        theta = np.float32(p)
        for i in range(n_rot // 2):
            tab[p, i, 0] = m.cosf(theta)
            tab[p, i, 1] = m.sinf(theta)
            theta = np.float32(theta * ts)
    tab.setflags(write=False)
    return tab


def rope_apply(v, tab, pos, head_dim, n_rot):
    """v [heads * head_dim] f32 rotated at `pos` (NORM mode: pairs (d, d + 1), d < n_rot), one
    f32 rounding per operation."""
    o = v.reshape(-1, head_dim).astype(np.float32).copy()
    a, b = o[:, 0:n_rot:2].copy(), o[:, 1:n_rot:2].copy()
    c, s = tab[pos, :, 0][None, :], tab[pos, :, 1][None, :]
    o[:, 0:n_rot:2] = (a * c).astype(np.float32) - (b * s).astype(np.float32)
    o[:, 1:n_rot:2] = (a * s).astype(np.float32) + (b * c).astype(np.float32)
    return o.reshape(-1)


# ---- QKV -----------------------------------------------------------------------------------
class QkvCase:
    """Weights, activations and row sums of one (type set, head shape, n_rot, cols, numerics)."""

    def __init__(self, tset, head_dim, n_rot, cols, num):
        d, h, hk = next(s for s in HEADS if s[0] == head_dim)
        self.tset, self.D, self.H, self.HK, self.n_rot, self.cols, self.num = tset, d, h, hk, n_rot, cols, num
        self.nq, self.nk = h * d, hk * d
        self.rows = (self.nq, self.nk, self.nk)
        rng = np.random.default_rng(1000 * d + n_rot + cols + sum(tset))
        self.raw = [ladder_blocks(tset[0], self.nq, cols, rng)]
        for i in (1, 2):
            self.raw.append(with_tie_rows(tset[i], ladder_blocks(tset[i], self.nk, cols, rng), self.nk, cols))
        self.base = norm_base(cols, rng)
        self.X = activations(QKV_TOKENS, cols, rng, self.base)
        self.rope_base = ROPE_BASES[(d // 64 + n_rot // 32) % 2]
        self.rope = rope_table(n_rot, self.rope_base)
        # [segment][family][token][row]
        self.sums = [row_sums(tset[i], self.raw[i], self.rows[i], cols, self.X, self.base, num) for i in range(3)]
        for a in (self.X, self.base, *self.raw, *self.sums):
            a.setflags(write=False)

    def token(self, f, t, pos):
        """(q f32 [nq], k f16 [HK][D], v f16 [HK][D]) of token t of family f at `pos`."""
        q = rope_apply(self.sums[0][f, t], self.rope, pos, self.D, self.n_rot)
        with np.errstate(over="ignore"):
            k = rope_apply(self.sums[1][f, t], self.rope, pos, self.D, self.n_rot).astype(np.float16)
            v = self.sums[2][f, t].astype(np.float16)
        return q, k.reshape(self.HK, self.D), v.reshape(self.HK, self.D)

    def kv_f32(self, f, t, pos):
        """The f32 values that become K and V (before the f16 conversion)."""
        return rope_apply(self.sums[1][f, t], self.rope, pos, self.D, self.n_rot), self.sums[2][f, t]


@functools.lru_cache(maxsize=None)
def qkv_case(tset, head_dim, n_rot, cols, num):
    return QkvCase(tset, head_dim, n_rot, cols, num)


def f16_class_counts(v):
    """(overflow to inf, normal, subnormal, rounds to zero) counts of f32 values under the
    f16 conversion."""
    a = np.abs(v.astype(np.float64))
    return (int((a >= 65520.0).sum()), int(((a >= 2.0 ** -14) & (a < 65520.0)).sum()),
            int(((a > 2.0 ** -25) & (a < 2.0 ** -14)).sum()), int((a <= 2.0 ** -25).sum()))


def f16_ties(v):
    """How many f32 values lie exactly halfway between two adjacent finite f16 values."""
    v = v.astype(np.float32).reshape(-1)
    v = v[np.abs(v) < 65504.0]
    h = v.astype(np.float16)
    toward = np.where(v.astype(np.float64) > h.astype(np.float64), np.float16(np.inf), np.float16(-np.inf))
    other = np.nextafter(h, toward)
    d1 = np.abs(v.astype(np.float64) - h.astype(np.float64))
    d2 = np.abs(v.astype(np.float64) - other.astype(np.float64))
    return int(((d1 == d2) & (d1 > 0)).sum())


# ---- SwiGLU --------------------------------------------------------------------------------
def band_blocks(qtype, rows, cols, X, base, num, rng):
    """Random payload under one power-of-two scale per type and column count: the gate
    values of family 1 get a standard deviation near 100."""
    raw = random_blocks(qtype, rows, cols, rng).reshape(rows, -1, BLOCK_BYTES[qtype]).copy()
    _set_scales(raw, 1.0)
    g = np.stack([po.matvec(qtype, raw.reshape(-1), rows, cols, po.rms_norm_mul(x, base, EPS), x86=x86_flags(num))
                  for x in X])
    e = int(np.clip(np.round(np.log2(100.0 / g.std())), -24, 15))
    _set_scales(raw, 2.0 ** e)
    return raw.reshape(-1)


def silu_mul(g, u, num):
    """g / (1 + expf(-g)) * u in f32, expf the oracle's in these numerics."""
    g, u = g.astype(np.float32), u.astype(np.float32)
    with po.x86_mode(x86_flags(num)):
        e = np.array([po.expf(float(-x)) for x in g.reshape(-1)], dtype=np.float32).reshape(g.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((g / (np.float32(1) + e)).astype(np.float32) * u).astype(np.float32)


class SwigluCase:
    def __init__(self, tset, rows, cols, num):
        self.tset, self.rows, self.cols, self.num = tset, rows, cols, num
        rng = np.random.default_rng(77 * rows + cols + sum(tset))
        self.base = norm_base(cols, rng)
        self.X = activations(SWIGLU_TOKENS, cols, rng, self.base)
        self.raw = [band_blocks(tset[0], rows, cols, self.X, self.base, num, rng), ladder_blocks(tset[1], rows, cols, rng)]
        self.gate = row_sums(tset[0], self.raw[0], rows, cols, self.X, self.base, num)   # [family][token][row]
        self.up = row_sums(tset[1], self.raw[1], rows, cols, self.X, self.base, num)
        self.h = silu_mul(self.gate, self.up, num)
        for a in (self.X, self.base, *self.raw, self.gate, self.up, self.h):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def swiglu_case(tset, rows, cols, num):
    return SwigluCase(tset, rows, cols, num)


BANDS = ((0.0, 88.0), (88.73, 103.97), (104.0, 133.0), (133.1, np.inf))


def band_counts(g):
    """[(values > 0, values < 0)] per band of |g|."""
    g = g.astype(np.float64).reshape(-1)
    return [(int(((g > lo) & (g < hi)).sum()), int(((-g > lo) & (-g < hi)).sum())) for lo, hi in BANDS]


# ---- logits --------------------------------------------------------------------------------
class LogitCase:
    """One tie set over `rows` rows of `qtype`: raw weights, LOGIT_TOKENS activations, the
    reference logits [family][token][row] and the rows that tie at token 0's maximum (in family
    1; bit-equal to one another in every family and slot)."""

    def __init__(self, qtype, rows, lset, num):
        cols = LOGIT_COLS
        self.qtype, self.rows, self.cols, self.lset, self.num = qtype, rows, cols, lset, num
        rng = np.random.default_rng(31 * rows + qtype + LOGIT_SETS.index(lset))
        self.base = norm_base(cols, rng)
        x0 = rng.standard_normal(cols).astype(np.float32)
        if lset in ("negative", "zero_max"):  # related activations: the pool rows are negative in every slot
            X = [x0 + np.float32(0.25) * rng.standard_normal(cols).astype(np.float32) for _ in range(LOGIT_TOKENS)]
        else:
            X = [x0] + [rng.standard_normal(cols).astype(np.float32) for _ in range(LOGIT_TOKENS - 1)]
        self.X = np.stack([tuned_x(x, self.base) for x in X])
        raw = random_blocks(qtype, rows, cols, rng).reshape(rows, -1).copy()
        ref_all = row_sums(qtype, raw.reshape(-1), rows, cols, self.X, self.base, num)
        ref = ref_all[1]   # family 1: [token][row]
        self.tied = ()
        if lset in ("negative", "zero_max"):
            pool = np.flatnonzero((ref_all < 0).all(axis=(0, 1)))
            assert pool.size >= 2, "fewer than two rows are negative in every slot and family"
            raw = raw[pool[np.arange(rows) % pool.size]]
            if lset == "zero_max":
                zr = raw.reshape(rows, -1, BLOCK_BYTES[qtype])
                for r, bits in ((rows // 3, 0x8000), (rows // 2, 0x0000), (rows - 2, 0x8000)):
                    for sl in SCALE_BYTES[qtype]:
                        zr[r, :, sl] = np.array([bits], dtype=np.uint16).view(np.uint8)
                self.tied = (rows // 3, rows // 2, rows - 2)
            else:
                self.tied = tuple(int(i) for i in np.arange(rows) if i % pool.size == int(np.argmax(ref[0][pool])))
        else:
            a = int(np.argmax(ref[0]))
            k = 2 * ((rows // 2) // 2)
            edge = (63, 64) if rows > 64 else (15, 16)
            tied = {"first_last": (0, rows - 1), "pair": (k, k + 1), "boundary": edge, "last": (rows - 1,)}[lset]
            src = raw[a].copy()
            if a not in tied:  # the former winner becomes a copy of the lowest row
                raw[a] = raw[int(np.argmin(ref[0]))]
            for r in tied:
                raw[r] = src
            self.tied = tied
        self.raw = raw.reshape(-1)
        self.logits = row_sums(qtype, self.raw, rows, cols, self.X, self.base, num)
        for a in (self.X, self.base, self.raw, self.logits):
            a.setflags(write=False)

    def winner(self, f, t):
        """First index of the maximum under float compare (-0 == +0)."""
        return int(np.argmax(self.logits[f, t]))


@functools.lru_cache(maxsize=None)
def logit_case(qtype, rows, lset, num):
    return LogitCase(qtype, rows, lset, num)
