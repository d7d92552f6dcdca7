"""The arithmetic behind the split-unit matvec geometry (mv_device.h "Split units"), on the
CPU with the numpy block decode of tests/test_matvec_edge_inputs.py: a 256-weight unit is
shared by two lanes, the even one taking parts 0-3 (chunks 0, 1: elements 0..127, sub-blocks
0..3 of Q4_K / Q5_K) and the odd one parts 4-7 (elements 128..255, sub-blocks 4..7).  For
saturated, sign-aligned near-saturated and random blocks:

  - the two halves' integer partials add up to the whole unit's sums: the eight residue sums
    aux32[l] (l = e % 8) of ggml's generic order, the eight lane sums (l = (e % 32) / 4) of
    the x86 order, the min sum sumi and the x86 order's four prod[k], of which the even lane
    holds k = 0, 1 and the odd lane k = 2, 3;
  - every half stays inside the bounds the kernels' comments state: dot operands of the
    24-bit multiplies, the products, and partials no larger than the whole's bound;
  - the 6-bit scales and mins of sub-blocks 0..3 are the bytes of the FIRST word scales_mins
    forms from the 12-byte header and those of sub-blocks 4..7 the bytes of the SECOND, which
    is how a lane picks its half of them."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import BLOCK_BYTES, Q4_K, Q5_K, Q6_K, TNAME, near_saturated_blocks, random_blocks, saturated_blocks
from helpers import SAT_VARIANTS, general_acts
from test_matvec_edge_inputs import BOUND, act_int, block_sums, decode_int, k_scale_min

KTYPES = (Q4_K, Q5_K, Q6_K)
IDS = [TNAME[t] for t in KTYPES]
ROWS, COLS = 3, 1024
QMAX = {Q4_K: 15, Q5_K: 31, Q6_K: 32}
SMAX = {Q4_K: 63, Q5_K: 63, Q6_K: 128}


def block_sets(qtype, rng):
    """[(name, raw, activation vectors)]"""
    out = []
    for v in SAT_VARIANTS[qtype]:
        raw, acts = saturated_blocks(qtype, ROWS, COLS, v, rng)
        out.append((f"saturated{v}", raw, [make(rng) for _, make in acts]))
    raw, acts = near_saturated_blocks(qtype, ROWS, COLS, rng, aligned=True)
    out.append(("near_saturated_aligned", raw, [acts[0][1](rng) for _ in range(3)]))
    raw = random_blocks(qtype, ROWS, COLS, rng)
    out.append(("random", raw, [make(rng) for name, make in general_acts(qtype, COLS) if name in ("normal", "zero_block")]))
    return out


def products(qtype, raw, x):
    """scale(e) * q(e) * a(e) and a(e), [rows][blocks][256]"""
    q, s = decode_int(qtype, raw)
    a = act_int(qtype, x).reshape(1, COLS // 256, 256)
    return (q * s).reshape(ROWS, COLS // 256, 256) * a, np.broadcast_to(a, (ROWS, COLS // 256, 256))


@pytest.mark.parametrize("qtype", KTYPES, ids=IDS)
def test_half_partials_add_up_to_the_unit(qtype):
    rng = np.random.default_rng(41 + qtype)
    for name, raw, xs in block_sets(qtype, rng):
        for x in xs:
            p, _ = products(qtype, raw, x)
            lo, hi = p[:, :, :128], p[:, :, 128:]
            # generic order: residue l = e % 8 (128 is a multiple of 8: a half keeps the residues)
            g_lo, g_hi = lo.reshape(ROWS, -1, 16, 8).sum(axis=2), hi.reshape(ROWS, -1, 16, 8).sum(axis=2)
            whole = block_sums(qtype, raw, ROWS, COLS, x)
            assert np.array_equal(g_lo + g_hi, whole), name
            # x86 order: lane k = (e % 32) / 4
            x_lo, x_hi = (h.reshape(ROWS, -1, 4, 8, 4).sum(axis=(2, 4)) for h in (lo, hi))
            x_whole = p.reshape(ROWS, -1, 8, 8, 4).sum(axis=(2, 4))
            assert np.array_equal(x_lo + x_hi, x_whole), name
            assert np.array_equal(x_whole.sum(axis=2), whole.sum(axis=2)), name
            # a partial is no larger than the whole's bound (here: half of it), below 2^23
            bound = max(BOUND[qtype, v] for v in SAT_VARIANTS[qtype])
            for h in (g_lo, g_hi, x_lo, x_hi):
                assert np.abs(h).max() <= bound // 2 < 2 ** 23, name
            if name.startswith("saturated") and np.unique(np.sign(x)).size == 1:
                assert (np.abs(g_lo) == np.abs(whole) // 2).all() and (np.abs(g_hi) == np.abs(whole) // 2).all()


@pytest.mark.parametrize("qtype", KTYPES, ids=IDS)
def test_half_dot_operands_stay_in_24_bits(qtype):
    """Each half multiplies dot4 results (four products q * a of one sub-block; Q6_K: two, the
    other two bytes of the dword masked) by that sub-block's scale with a 24-bit multiply."""
    rng = np.random.default_rng(43 + qtype)
    n = 4 if qtype != Q6_K else 2
    for name, raw, xs in block_sets(qtype, rng):
        q, s = decode_int(qtype, raw)
        assert np.abs(q).max() <= QMAX[qtype] and np.abs(s).max() <= SMAX[qtype]
        for x in xs:
            a = act_int(qtype, x).reshape(1, COLS // 256, 256)
            qa = q.reshape(ROWS, COLS // 256, 256) * a
            # generic order: a dot holds the elements l + 8 i of one 32-element sub-block
            # (Q6_K: of one 16-element sub-block, i.e. two of them)
            if qtype == Q6_K:
                dots = qa.reshape(ROWS, -1, 16, 2, 8).sum(axis=3)
            else:
                dots = qa.reshape(ROWS, -1, 8, 4, 8).sum(axis=3)
            assert np.abs(dots).max() <= n * QMAX[qtype] * 127 < 2 ** 23, name
            assert np.abs(dots).max() * SMAX[qtype] < 2 ** 31, name
            # x86 order: four consecutive elements
            dots = qa.reshape(ROWS, -1, 64, 4).sum(axis=3)
            assert np.abs(dots).max() <= 4 * QMAX[qtype] * 127 < 2 ** 23, name


def scales_mins_words(sb):
    """mv_device.h scales_mins on the 12 header bytes [nb][12] as three little-endian words:
    (sc.x, sc.y, mn.x, mn.y), each [nb] uint32."""
    w = sb.astype(np.uint8).copy().view("<u4").astype(np.uint64)
    s0, s1, s2 = w[:, 0], w[:, 1], w[:, 2]
    m4 = 0x0F0F0F0F
    return (s0 & 0x3F3F3F3F, (s2 & m4) | ((s0 >> 2) & 0x30303030), s1 & 0x3F3F3F3F, ((s2 >> 4) & m4) | ((s1 >> 2) & 0x30303030))


@pytest.mark.parametrize("qtype", (Q4_K, Q5_K), ids=IDS[:2])
def test_header_words_split_by_half(qtype):
    rng = np.random.default_rng(47 + qtype)
    for name, raw, _ in block_sets(qtype, rng):
        sb = raw.reshape(-1, BLOCK_BYTES[qtype])[:, 4:16]
        sc, mn = k_scale_min(sb)
        scx, scy, mnx, mny = scales_mins_words(sb)
        for j in range(4):
            assert np.array_equal((scx >> (8 * j)) & 0xFF, sc[:, j]) and np.array_equal((scy >> (8 * j)) & 0xFF, sc[:, 4 + j]), name
            assert np.array_equal((mnx >> (8 * j)) & 0xFF, mn[:, j]) and np.array_equal((mny >> (8 * j)) & 0xFF, mn[:, 4 + j]), name


@pytest.mark.parametrize("qtype", (Q4_K, Q5_K), ids=IDS[:2])
def test_half_min_sums_add_up(qtype):
    rng = np.random.default_rng(53 + qtype)
    for name, raw, xs in block_sets(qtype, rng):
        _, mn = k_scale_min(raw.reshape(-1, BLOCK_BYTES[qtype])[:, 4:16])
        mn = mn.reshape(ROWS, COLS // 256, 8)
        for x in xs:
            a = act_int(qtype, x).reshape(COLS // 256, 256)
            bs16 = a.reshape(-1, 16, 16).sum(axis=2)          # q8_K bsums
            bs32 = bs16.reshape(-1, 8, 2).sum(axis=2)[None]   # per 32-element sub-block
            terms = mn * bs32                                  # m_j (bs[2j] + bs[2j+1])
            sumi = terms.sum(axis=2)
            lo, hi = terms[:, :, :4].sum(axis=2), terms[:, :, 4:].sum(axis=2)
            assert np.array_equal(lo + hi, sumi), name
            prod = terms.reshape(ROWS, -1, 4, 2).sum(axis=3)   # x86 order: prod[k] = pairs 2k, 2k + 1
            assert np.array_equal(np.concatenate([prod[:, :, :2], prod[:, :, 2:]], axis=2).sum(axis=2), sumi), name
            assert np.array_equal(prod[:, :, :2].sum(axis=2), lo) and np.array_equal(prod[:, :, 2:].sum(axis=2), hi), name
            # sdot2 pairs: int16 bsums against 6-bit mins, |sumi| <= 8 * 63 * 32 * 127
            assert np.abs(bs16).max() <= 16 * 127 and np.abs(sumi).max() <= 8 * 63 * 32 * 127 < 2 ** 23, name
            for h in (lo, hi):
                assert np.abs(h).max() <= 4 * 63 * 32 * 127, name
