"""Test helpers: random quantized blocks with sane fp16 scales, device buffers."""
from __future__ import annotations

import numpy as np

F32, F16, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 8, 12, 13, 14
BLOCK_ELEMS = {Q8_0: 32, Q4_K: 256, Q5_K: 256, Q6_K: 256}
BLOCK_BYTES = {Q8_0: 34, Q4_K: 144, Q5_K: 176, Q6_K: 210}
QTYPES = (Q4_K, Q5_K, Q6_K, Q8_0)
TNAME = {Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K", Q8_0: "q8_0"}


def f16_bytes(v: np.ndarray) -> np.ndarray:
    return np.asarray(v, dtype=np.float16).view(np.uint8).reshape(-1, 2)


def random_blocks(qtype: int, rows: int, cols: int, rng: np.random.Generator) -> np.ndarray:
    """Uniform random payload bytes with fp16 block scales of realistic magnitude."""
    nb = rows * (cols // BLOCK_ELEMS[qtype])
    bb = BLOCK_BYTES[qtype]
    raw = rng.integers(0, 256, size=(nb, bb), dtype=np.uint8)
    if qtype in (Q4_K, Q5_K):
        d = rng.uniform(2e-5, 1.2e-4, nb).astype(np.float32)
        raw[:, 0:2] = f16_bytes(d)
        raw[:, 2:4] = f16_bytes(d * 7.5)
    elif qtype == Q6_K:
        raw[:, 208:210] = f16_bytes(rng.uniform(1e-5, 5e-5, nb))
    else:
        raw[:, 0:2] = f16_bytes(rng.uniform(1e-4, 5e-4, nb))
    return raw.reshape(-1)


# ---- edge inputs: blocks and activations at the bounds of the kernels' exactness argument ----
# (prefill.hip header, mv_device.h unit_terms).  Every builder returns (raw, acts): raw
# ggml blocks and the activation families that go with them, acts = [(name, make)], where
# make(rng) draws one f32[cols] vector of the family.
SAT_VARIANTS = {Q4_K: (0,), Q5_K: (0,), Q6_K: (0, 1), Q8_0: (0, 1)}
# byte ranges of the fp16 scales of a block: d, then dmin
SCALE_BYTES = {Q4_K: (slice(0, 2), slice(2, 4)), Q5_K: (slice(0, 2), slice(2, 4)), Q6_K: (slice(208, 210),),
               Q8_0: (slice(0, 2),)}
# fp16 bit patterns of the scale edges: +-0, +-2^-24 (smallest subnormal), the largest
# subnormal, 2^-14 (smallest normal), +-65504 (largest finite)
F16_EDGE_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF)


def pack_k_scales(sc: np.ndarray, mn: np.ndarray) -> np.ndarray:
    """The 12 scale bytes of a Q4_K / Q5_K block from its eight 6-bit scales and mins
    ([nb][8] each), the inverse of ggml's get_scale_min_k4."""
    sc, mn = sc.astype(np.uint8), mn.astype(np.uint8)
    q = np.empty((sc.shape[0], 12), dtype=np.uint8)
    q[:, 0:4] = (sc[:, 0:4] & 63) | ((sc[:, 4:8] >> 4) << 6)
    q[:, 4:8] = (mn[:, 0:4] & 63) | ((mn[:, 4:8] >> 4) << 6)
    q[:, 8:12] = (sc[:, 4:8] & 15) | ((mn[:, 4:8] & 15) << 4)
    return q


def _blank(qtype, rows, cols, rng):
    """random_blocks' fp16 scales around a payload the caller overwrites."""
    return random_blocks(qtype, rows, cols, rng).reshape(-1, BLOCK_BYTES[qtype]).copy()


def _payload(qtype):
    """Byte range of a block that is not an fp16 scale."""
    return {Q4_K: slice(4, 144), Q5_K: slice(4, 176), Q6_K: slice(0, 208), Q8_0: slice(2, 34)}[qtype]


def _signed_const(cols, sign):
    """x = s * c with one |c| per vector: every q8 value is +-127.  sign: +1, -1, or 0 for
    a random sign per element."""
    def make(rng):
        c = np.float32(rng.uniform(0.5, 2.0))
        s = np.float32(sign) if sign else rng.choice(np.array([-1.0, 1.0], dtype=np.float32), cols)
        return (s * c * np.ones(cols, dtype=np.float32)).astype(np.float32)
    return make


def saturated_acts(cols):
    return [("all_plus", _signed_const(cols, 1)), ("all_minus", _signed_const(cols, -1)),
            ("mixed_signs", _signed_const(cols, 0))]


def saturated_blocks(qtype, rows, cols, variant, rng):
    """Every element at the type's extreme: Q4_K / Q5_K q = 15 / 31 with every 6-bit scale
    and min 63; Q6_K variant 0 q - 32 = -32 with scales -128, variant 1 q - 32 = +31 with
    scales +127; Q8_0 quants -128 (variant 0) or +127 (variant 1).  The fp16 d / dmin are
    random_blocks'.  With the activations (every q8 value +-127) each integer block sum of
    the uniform sign patterns sits on its bound."""
    assert variant in SAT_VARIANTS[qtype]
    raw = _blank(qtype, rows, cols, rng)
    if qtype in (Q4_K, Q5_K):
        raw[:, _payload(qtype)] = 0xFF
    elif qtype == Q6_K:
        raw[:, 0:192] = 0x00 if variant == 0 else 0xFF
        raw[:, 192:208] = 0x80 if variant == 0 else 0x7F
    else:
        raw[:, 2:34] = 0x80 if variant == 0 else 0x7F
    return raw.reshape(-1), saturated_acts(cols)


def near_saturated_acts(cols, sig=None, blk=256):
    """|a| in 120..127.  sig None: a random sign per element.  Else the sign of element e is
    sig[e] times one random sign per `blk` elements (the aligned form below)."""
    def make(rng):
        # one 127 in every 32 elements, so that the block maximum (q8_K: per 256, q8_0: per
        # 32) is the same c, and a = 127 x / c
        mag = rng.integers(120, 128, cols).astype(np.float32)
        mag[np.arange(0, cols, 32) + rng.integers(0, 32, cols // 32)] = 127.0
        pm = np.array([-1.0, 1.0], dtype=np.float32)
        s = rng.choice(pm, cols) if sig is None else sig.astype(np.float32) * np.repeat(rng.choice(pm, cols // blk), blk)
        return (s * mag * np.float32(rng.uniform(0.5, 2.0) / 127.0)).astype(np.float32)
    return [("near_sat" if sig is None else "near_sat_aligned", make)]


def near_saturated_blocks(qtype, rows, cols, rng, aligned=False):
    """Quants from the top two and bottom two values of the type, scales from the top four
    (Q6_K: also -128..-125), activations with |a| in 120..127 and random signs.

    With random signs the products cancel, and the block sums stay a few times below
    their bound.  aligned=True removes the cancellation: one sign per column, sig[e], shared
    by every row, is the sign of every weight value scale(e) * q(e) in that column (Q4_K /
    Q5_K: +, with quants from the top two values only), and the activations take sig[e]
    times one random sign per block.  Every product of a block then has the same sign, and
    every integer block sum is within 86 % .. 100 % of the bound (Q6_K: above 2^23) with
    varied low bits, which is what an inexact accumulation would corrupt."""
    raw = _blank(qtype, rows, cols, rng)
    nb = raw.shape[0]
    be = BLOCK_ELEMS[qtype]
    sig = rng.choice(np.array([-1, 1]), cols) if aligned and qtype in (Q6_K, Q8_0) else np.ones(cols, dtype=np.int64)
    sig_b = np.tile(sig.reshape(cols // be, be), (rows, 1))  # [nb][block elements]
    if qtype in (Q4_K, Q5_K):
        hi = 15 if qtype == Q4_K else 31
        q = rng.choice(np.array([hi - 1, hi] if aligned else [0, 1, hi - 1, hi]), (nb, 256))
        # element 64 j + 32 h + l: nibble h of byte 32 j + l, fifth bit 2 j + h of qh[l]
        q4 = q.reshape(nb, 4, 2, 32)
        qs = ((q4[:, :, 0, :] & 15) | ((q4[:, :, 1, :] & 15) << 4)).astype(np.uint8).reshape(nb, 128)
        raw[:, 4:16] = pack_k_scales(rng.integers(60, 64, (nb, 8)), rng.integers(60, 64, (nb, 8)))
        if qtype == Q4_K:
            raw[:, 16:144] = qs
        else:
            qh = np.zeros((nb, 32), dtype=np.uint8)
            for j in range(4):
                for h in range(2):
                    qh |= ((q4[:, j, h, :] >> 4) & 1).astype(np.uint8) << (2 * j + h)
            raw[:, 16:48] = qh
            raw[:, 48:176] = qs
    elif qtype == Q6_K:
        sc = rng.choice(np.array([124, 125, 126, 127, -128, -127, -126, -125], dtype=np.int8), (nb, 16))
        q = rng.choice(np.array([0, 1, 62, 63]), (nb, 256))  # q - 32: -32, -31, 30, 31
        if aligned:  # the sign of q - 32 is sig[e] times the sign of its sub-block's scale
            pos = np.repeat(np.sign(sc.astype(np.int64)), 16, axis=1) * sig_b > 0
            q = np.where(pos, rng.choice(np.array([62, 63]), (nb, 256)), rng.choice(np.array([0, 1]), (nb, 256)))
        # element 128 n + 32 k + l: k = 0, 1 low nibbles of ql[64 n + 32 k + l], k = 2, 3 the
        # high nibbles of ql[64 n + 32 (k - 2) + l]; bits 2 k of qh[32 n + l]
        q6 = q.reshape(nb, 2, 4, 32)
        ql = ((q6[:, :, 0:2, :] & 15) | ((q6[:, :, 2:4, :] & 15) << 4)).astype(np.uint8).reshape(nb, 128)
        qh = np.zeros((nb, 2, 32), dtype=np.uint8)
        for k in range(4):
            qh |= ((q6[:, :, k, :] >> 4) & 3).astype(np.uint8) << (2 * k)
        raw[:, 0:128] = ql
        raw[:, 128:192] = qh.reshape(nb, 64)
        raw[:, 192:208] = sc.view(np.uint8)
    else:
        q = rng.choice(np.array([-128, -127, 126, 127], dtype=np.int8), (nb, 32))
        if aligned:
            q = np.where(sig_b > 0, rng.choice(np.array([126, 127], dtype=np.int8), (nb, 32)),
                         rng.choice(np.array([-128, -127], dtype=np.int8), (nb, 32)))
        raw[:, 2:34] = q.astype(np.int8).view(np.uint8)
    return raw.reshape(-1), near_saturated_acts(cols, sig if aligned else None, be)


def general_acts(qtype, cols, huge=True):
    """Activation families for weights of ordinary magnitude: normal; one all-zero
    256-block; an all-zero vector; x * 1e-35 (d_a normal, d_w * d_a an f32 subnormal, the
    result normal again); x * 3e-5 (a q8_0 activation d that is an fp16 subnormal); and with
    `huge` x * 1e30 for K-quants, x * 1e5 for Q8_0 (whose reference is NaN at 1e30: d_a
    overflows fp16)."""
    def normal(rng):
        return rng.standard_normal(cols).astype(np.float32)

    def zero_block(rng):
        x = normal(rng)
        b = int(rng.integers(0, cols // 256))
        x[256 * b: 256 * (b + 1)] = 0.0
        return x

    def scaled(f):
        return lambda rng: (rng.standard_normal(cols) * f).astype(np.float32)

    acts = [("normal", normal), ("zero_block", zero_block), ("all_zero", lambda rng: np.zeros(cols, dtype=np.float32)),
            ("x1e-35", scaled(1e-35)), ("x3e-5", scaled(3e-5))]
    if huge:
        acts.append(("x1e5", scaled(1e5)) if qtype == Q8_0 else ("x1e30", scaled(1e30)))
    return acts


def scale_edge_blocks(qtype, rows, cols, rng):
    """A random payload whose fp16 d (and, independently, the dmin of Q4_K / Q5_K) is drawn
    per block from: +- a value of random_blocks' magnitude, +-0, +-2^-24, the largest
    subnormal, 2^-14, +-65504.  The activation families leave out the huge one (65504 * d_a
    * the block sum overflows f32)."""
    raw = _blank(qtype, rows, cols, rng)
    nb = raw.shape[0]
    for sl in SCALE_BYTES[qtype]:
        bits = raw[:, sl].copy().view(np.uint16).reshape(nb)
        pick = rng.integers(0, len(F16_EDGE_BITS) + 2, nb)  # the last two: + / - the normal value
        edge = np.array(F16_EDGE_BITS + (0, 0), dtype=np.uint16)[pick]
        out = np.where(pick < len(F16_EDGE_BITS), edge, bits | np.where(pick == len(F16_EDGE_BITS) + 1, 0x8000, 0))
        raw[:, sl] = out.astype(np.uint16).view(np.uint8).reshape(nb, 2)
    return raw.reshape(-1), general_acts(qtype, cols, huge=False)


def pick_acts(acts, *names):
    """The families of `acts` with these names, in this order."""
    by = dict(acts)
    return [(n, by[n]) for n in names]


def edge_weight_sets(qtype, rows, cols, rng):
    """Every weight set of the edge matrix with its activation families:
    [(name, raw, acts)]."""
    sets = [("random", random_blocks(qtype, rows, cols, rng), general_acts(qtype, cols))]
    for v in SAT_VARIANTS[qtype]:
        raw, acts = saturated_blocks(qtype, rows, cols, v, rng)
        # (a saturated token beside a zero and an ordinary one in the batched kernels' tiles)
        sets.append((f"saturated{v}", raw, acts + pick_acts(general_acts(qtype, cols), "normal", "zero_block", "all_zero")))
    raw, acts = near_saturated_blocks(qtype, rows, cols, rng)
    sets.append(("near_saturated", raw, acts + pick_acts(saturated_acts(cols), "mixed_signs")))
    raw, acts = near_saturated_blocks(qtype, rows, cols, rng, aligned=True)
    sets.append(("near_saturated_aligned", raw, acts + pick_acts(general_acts(qtype, cols), "zero_block", "all_zero")))
    raw, acts = scale_edge_blocks(qtype, rows, cols, rng)
    sets.append(("scale_edge", raw, acts))
    return sets


def first_diff(got: np.ndarray, ref: np.ndarray) -> str:
    """'' when got and ref are bit-identical (uint32 views: signed zeros and NaN payloads
    count), else the first differing (row, value, reference)."""
    g, r = np.ascontiguousarray(got, dtype=np.float32).reshape(-1), np.ascontiguousarray(ref, dtype=np.float32).reshape(-1)
    assert g.shape == r.shape
    bad = np.flatnonzero(g.view(np.uint32) != r.view(np.uint32))
    if bad.size == 0:
        return ""
    i = int(bad[0])
    return (f"{bad.size} of {g.size} values differ, first at row {i}: got {g[i]!r} (0x{int(g.view(np.uint32)[i]):08x}), "
            f"reference {r[i]!r} (0x{int(r.view(np.uint32)[i]):08x})")


def to_dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def empty_dev(nbytes: int):
    import torch

    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
