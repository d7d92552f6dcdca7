"""Inputs and plain references of the step-entry kernel tests (llmi_step_entry: k_embed,
k_bembed, k_pf_embed, k_embed_row and their shared dequant_elem).

get_rows.  The reference of an embedding row is ggml's dequantize_row_* of the row's raw
GGUF bytes, stated twice: pyoracle.dequantize, and dequant_np below (float32 NumPy, one
rounding per multiply and per subtract, ggml's association).  test_step_entry_inputs.py holds
the two to each other bit for bit.  Beside them stands a NumPy model of the DEVICE side --
repack_np restates k_repack_*, layout_get_rows restates dequant_elem over those planes --
which serves one purpose: to apply a deliberately wrong read (MUTANTS_LAYOUT) and show that
the shapes and weight sets below tell it from the right one.

Token selection and state.  entry_ref restates common.h's StepState contract in a few lines;
STATE_CASES are the crafted states, each a (name, state) pair, and MUTANTS_STATE the wrong
variants of entry_ref they must tell apart.
"""
from __future__ import annotations

import functools

import numpy as np

from helpers import (Q4_K, Q5_K, Q6_K, Q8_0, BLOCK_BYTES, BLOCK_ELEMS, SAT_VARIANTS, random_blocks, saturated_blocks,
                     scale_edge_blocks)
from llmi import STEP_STATE

# (vocab, cols): the smallest shapes that reach each layout (rows per group RG = 2^rgs)
SHAPES = [(64, 256), (1001, 256), (1004, 512), (520, 2048), (36, 3072), (516, 4096), (66, 5120), (130, 8192), (40, 16384)]
SMALL, WIDE = (64, 256), (40, 16384)
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def layout_rgs(rows, cols):
    """common.h layout_rgs."""
    U = cols // 256
    lr = max(4, (min(U, 64) + 3) & ~3)
    R, s = 1, 0
    while 2 * R * lr <= 64:
        R, s = R * 2, s + 1
    while s > 0 and rows % R:
        R, s = R >> 1, s - 1
    return s


def weight_sets(qtype, vocab, cols):
    """[(name, raw)]: random blocks, every saturated variant, the fp16 scale edges."""
    rng = np.random.default_rng(qtype * 1000003 + vocab * 131 + cols)
    sets = [("random", random_blocks(qtype, vocab, cols, rng))]
    for v in SAT_VARIANTS[qtype]:
        sets.append((f"saturated{v}", saturated_blocks(qtype, vocab, cols, v, rng)[0]))
    sets.append(("scale_edge", scale_edge_blocks(qtype, vocab, cols, rng)[0]))
    return sets


def row_list(vocab, cols, rng):
    """0, 1, RG-1, RG, RG+1, the last RG+1 rows, V-1 and a few random rows."""
    RG = 1 << layout_rgs(vocab, cols)
    rows = [0, 1, RG - 1, RG, RG + 1] + list(range(vocab - RG - 1, vocab)) + [vocab - 1]
    rows += [int(r) for r in rng.integers(0, vocab, 4)]
    out = []
    for r in rows:
        if 0 <= r < vocab and r not in out:
            out.append(r)
    return out


# ---- get_rows, reference 1: ggml's dequantize_row_* in float32 NumPy --------------------------
def _h2f(b):
    """fp16 bytes [..., 2] -> f32 (exact)."""
    return np.ascontiguousarray(b).view(np.float16)[..., 0].astype(np.float32)


def _scale_min_k4(j, q):
    """ggml's get_scale_min_k4 over scale bytes q [..., 12] -> (sc, m) uint8 [...]."""
    if j < 4:
        return q[..., j] & 63, q[..., j + 4] & 63
    return (q[..., j + 4] & 0xF) | ((q[..., j - 4] >> 6) << 4), (q[..., j + 4] >> 4) | ((q[..., j] >> 6) << 4)


def dequant_np(qtype, raw, rows, cols):
    """f32 [rows][cols]: every product and difference rounded once, as ggml's scalar code
    compiled without contraction."""
    f32 = np.float32
    blk = np.asarray(raw, dtype=np.uint8).reshape(-1, BLOCK_BYTES[qtype])
    nb = blk.shape[0]
    y = np.empty((nb, BLOCK_ELEMS[qtype]), dtype=f32)
    if qtype in (Q4_K, Q5_K):
        d, dmin, sc12 = _h2f(blk[:, 0:2])[:, None], _h2f(blk[:, 2:4])[:, None], blk[:, 4:16]
        qh = blk[:, 16:48] if qtype == Q5_K else None
        qs = blk[:, 48:176] if qtype == Q5_K else blk[:, 16:144]
        for j in range(4):
            q = qs[:, 32 * j: 32 * j + 32]
            for h in range(2):
                sc, m = _scale_min_k4(2 * j + h, sc12)
                d1 = d * sc.astype(f32)[:, None]
                m1 = dmin * m.astype(f32)[:, None]
                v = ((q >> 4) if h else (q & 0xF)).astype(np.int32)
                if qh is not None:
                    v = v + np.where(qh & (1 << (2 * j + h)), 16, 0)
                y[:, 64 * j + 32 * h: 64 * j + 32 * h + 32] = d1 * v.astype(f32) - m1
    elif qtype == Q6_K:
        d = _h2f(blk[:, 208:210])[:, None]
        sc = blk[:, 192:208].view(np.int8)
        for n in range(2):
            ql, qh = blk[:, 64 * n: 64 * n + 64], blk[:, 128 + 32 * n: 128 + 32 * n + 32]
            for quad in range(4):
                lo = ql[:, 32 * (quad & 1): 32 * (quad & 1) + 32]
                lo = (lo >> 4) if quad >> 1 else (lo & 0xF)
                q = (lo | (((qh >> (2 * quad)) & 3) << 4)).astype(np.int32) - 32
                s = np.repeat(sc[:, 8 * n + 2 * quad: 8 * n + 2 * quad + 2], 16, axis=1).astype(f32)  # is = l / 16
                y[:, 128 * n + 32 * quad: 128 * n + 32 * quad + 32] = (d * s) * q.astype(f32)
    else:
        y[:] = blk[:, 2:34].view(np.int8).astype(f32) * _h2f(blk[:, 0:2])[:, None]
    return y.reshape(rows, cols)


@functools.lru_cache(maxsize=2)
def references(qtype, vocab, cols):
    """[(set name, raw, table f32 [vocab][cols])] by the oracle; shared, read-only."""
    import pyoracle as po

    out = []
    for name, raw in weight_sets(qtype, vocab, cols):
        tab = po.dequantize(qtype, raw, vocab * cols).reshape(vocab, cols)
        tab.setflags(write=False)
        raw.setflags(write=False)
        out.append((name, raw, tab))
    return out


# ---- the device side in NumPy: k_repack_* and dequant_elem ------------------------------------
def piece_off(row, p, u, U, nparts, rgs):
    """mv_device.h piece_off."""
    g, r = row >> rgs, row & ((1 << rgs) - 1)
    return ((((g * nparts + p) << rgs) + r) * U + u) * 16


def _el(x86, l, i):
    return 4 * l + i if x86 else l + 8 * i


def _u6(blk):
    """The 6-bit unsigned values of Q6_K blocks [..., 210] -> [..., 256]."""
    out = np.empty(blk.shape[:-1] + (256,), dtype=np.uint8)
    for n in range(2):
        for quad in range(4):
            lo = blk[..., 64 * n + 32 * (quad & 1): 64 * n + 32 * (quad & 1) + 32]
            lo = (lo >> 4) if quad >> 1 else (lo & 0xF)
            hi = (blk[..., 128 + 32 * n: 128 + 32 * n + 32] >> (2 * quad)) & 3
            out[..., 128 * n + 32 * quad: 128 * n + 32 * quad + 32] = lo | (hi << 4)
    return out


def repack_np(qtype, raw, rows, cols, x86):
    """The planes k_repack_kq / k_repack_q80 write: dict(A, H, S, D) of uint8 arrays."""
    U, rgs = cols // 256, layout_rgs(rows, cols)
    row, u = np.arange(rows, dtype=np.int64)[:, None], np.arange(U, dtype=np.int64)[None, :]
    P = dict(A=np.zeros(rows * U * (256 if qtype == Q8_0 else 128), np.uint8), H=np.zeros(1, np.uint8), S=np.zeros(1, np.uint8),
             D=np.zeros(1, np.uint8))
    if qtype == Q8_0:
        blk = np.asarray(raw, np.uint8).reshape(rows, U, 8, 34)
        for b in range(8):
            for h in range(2):
                off = piece_off(row, 2 * b + h, u, U, 16, rgs)
                P["A"][off[..., None] + np.arange(16)] = blk[:, :, b, 2 + 16 * h: 18 + 16 * h]
        P["D"] = blk[:, :, :, 0:2].reshape(-1).copy()
        return P
    blk = np.asarray(raw, np.uint8).reshape(rows, U, BLOCK_BYTES[qtype])
    if qtype in (Q4_K, Q5_K):
        qs = blk[:, :, 48:176] if qtype == Q5_K else blk[:, :, 16:144]
        P["S"] = blk[:, :, 0:16].reshape(-1).copy()
        nib = lambda c, t: qs[:, :, 32 * c + t]  # noqa: E731
    else:
        v6 = _u6(blk)
        P["S"], P["D"] = blk[:, :, 192:208].reshape(-1).copy(), blk[:, :, 208:210].reshape(-1).copy()
        nib = lambda c, t: (v6[:, :, 64 * c + t] & 15) | ((v6[:, :, 64 * c + 32 + t] & 15) << 4)  # noqa: E731
    for c in range(4):
        for k in range(2):
            off = piece_off(row, 2 * c + k, u, U, 8, rgs)
            for m in range(4):
                for i in range(4):
                    P["A"][off + 4 * m + i] = nib(c, _el(x86, 4 * k + m, i))
    if qtype == Q5_K:
        qh = blk[:, :, 16:48]
        P["H"] = np.zeros(rows * U * 32, np.uint8)
        for c in range(4):
            off = piece_off(row, c >> 1, u, U, 2, rgs) + 8 * (c & 1)
            for i in range(4):
                lo, hi = np.zeros((rows, U), np.uint8), np.zeros((rows, U), np.uint8)
                for l in range(8):
                    lo |= ((qh[:, :, _el(x86, l, i)] >> (2 * c)) & 1) << l
                    hi |= ((qh[:, :, _el(x86, l, i)] >> (2 * c + 1)) & 1) << l
                P["H"][off + i], P["H"][off + 4 + i] = lo, hi
    elif qtype == Q6_K:
        P["H"] = np.zeros(rows * U * 64, np.uint8)
        for c in range(4):
            off = piece_off(row, c, u, U, 4, rgs)
            for g in range(4):
                for i in range(4):
                    v = np.zeros((rows, U), np.uint8)
                    for m in range(4):
                        v |= ((v6[:, :, 64 * c + 32 * (g >> 1) + _el(x86, 4 * (g & 1) + m, i)] >> 4) ^ 2) << (2 * m)
                    P["H"][off + 4 * g + i] = v
    return P


# wrong reads of the device layout that the get_rows matrix must tell from the right one
MUTANTS_LAYOUT = ("order_swapped", "rgs_ignored", "rgs_plus_one", "q6_no_xor", "q5_other_half")


def layout_get_rows(qtype, P, vocab, cols, x86, rows, mutant=None):
    """dequant_elem over the planes P for the rows `rows` -> f32 [len(rows)][cols].  mutant:
    one of MUTANTS_LAYOUT (reads outside a plane wrap around)."""
    f32 = np.float32
    U, rgs = cols // 256, layout_rgs(vocab, cols)
    if mutant == "rgs_ignored":
        rgs = 0
    elif mutant == "rgs_plus_one":
        rgs += 1
    if mutant == "order_swapped":
        x86 = not x86
    row = np.asarray(rows, dtype=np.int64)[:, None]
    e = np.arange(cols, dtype=np.int64)[None, :]
    u, t = e >> 8, e & 255
    ru = row * U + u
    take = lambda plane, idx: np.take(P[plane], idx, mode="wrap")  # noqa: E731
    if qtype == Q8_0:
        q = take("A", piece_off(row, t >> 4, u, U, 16, rgs) + (t & 15)).view(np.int8)
        d = _h2f(np.stack([take("D", ru * 16 + 2 * (t >> 5)), take("D", ru * 16 + 2 * (t >> 5) + 1)], axis=-1))
        return q.astype(f32) * d
    c, hi = t >> 6, (t >> 5) & 1
    l = (t & 31) >> 2 if x86 else t & 7
    i = t & 3 if x86 else (t & 31) >> 3
    k, m = l >> 2, l & 3
    qb = take("A", piece_off(row, 2 * c + k, u, U, 8, rgs) + 4 * m + i)
    q = np.where(hi == 1, qb >> 4, qb & 0xF).astype(np.int32)
    if qtype == Q6_K:
        hb = (take("H", piece_off(row, c, u, U, 4, rgs) + (2 * hi + k) * 4 + i) >> (2 * m)) & 3
        q |= (hb if mutant == "q6_no_xor" else hb ^ 2).astype(np.int32) << 4
        d = _h2f(np.stack([take("D", ru * 2), take("D", ru * 2 + 1)], axis=-1))
        sc = take("S", ru * 16 + (t >> 4)).view(np.int8)
        return (d * sc.astype(f32)) * (q - 32).astype(f32)
    hdr = P["S"].reshape(-1, 16)[ru]  # [n][cols][16]
    d, dmin = _h2f(hdr[..., 0:2]), _h2f(hdr[..., 2:4])
    sc, mn = np.zeros(ru.shape, np.uint8), np.zeros(ru.shape, np.uint8)
    for j in range(8):
        s_j, m_j = _scale_min_k4(j, hdr[..., 4:16])
        sel = (2 * c + hi) == j
        sc, mn = np.where(sel, s_j, sc), np.where(sel, m_j, mn)
    if qtype == Q5_K:
        half = 1 - hi if mutant == "q5_other_half" else hi
        hb = take("H", piece_off(row, c >> 1, u, U, 2, rgs) + 8 * (c & 1) + 4 * half + i)
        q += ((hb >> l) & 1).astype(np.int32) << 4
    return (d * sc.astype(f32)) * q.astype(f32) - dmin * mn.astype(f32)


# ---- token selection and state ----------------------------------------------------------------
N_CTX = 24  # of the state cases


def key(hi, tok):
    """An argmax key: the ordered logit `hi` above 0xffffffff - row."""
    return (int(hi) << 32) | ((0xFFFFFFFF - tok) & 0xFFFFFFFF)


# wrong variants of entry_ref that STATE_CASES must tell from the right one
MUTANTS_STATE = (["parity", "signed_compare", "hi_word_only", "no_low_clamp", "no_high_clamp"]
                 + [f"skip_lane_{k}" for k in range(64)])


def _key_max(slots, mutant):
    s = np.asarray(slots, dtype=np.uint64)
    if mutant == "signed_compare":
        return int(s[int(np.argmax(s.view(np.int64)))])
    if mutant == "hi_word_only":
        return int(s[int(np.argmax(s >> np.uint64(32)))])  # the first lane of the largest high word
    if mutant and mutant.startswith("skip_lane_"):
        return int(np.delete(s, int(mutant[10:])).max())
    return int(s.max())


def entry_ref(st, hist, vocab, n_ctx, mutant=None):
    """common.h's contract of k_embed / k_bembed on one state (a STEP_STATE record) and its
    history row: (state after, history after, token, position)."""
    st, hist = np.array(st, dtype=STEP_STATE).reshape(()), np.array(hist, dtype=np.int32)
    pos = int(st["pos_next"])
    if int(st["token_in_pos"]) == pos:
        tok = int(st["token_in"])
    else:
        k = _key_max(st["key"][pos & 1 if mutant == "parity" else (pos + 1) & 1], mutant)
        tok = int(np.uint32(0xFFFFFFFF - (k & 0xFFFFFFFF)).astype(np.int32))
    if (tok < 0 and mutant != "no_low_clamp") or (tok >= vocab and mutant != "no_high_clamp"):
        tok = 0
    st["pos"], st["token"] = pos, tok
    st["seq"] = (int(st["seq"]) + 1) & 0xFFFFFFFF
    st["key"][pos & 1] = 0
    if 0 <= pos < n_ctx:
        hist[pos] = tok
    return st, hist, tok, pos


def init_hist(n_seq, n_ctx):
    """A history no token of a case equals."""
    return (100000 + 1000 * np.arange(n_seq)[:, None] + np.arange(n_ctx)[None, :]).astype(np.int32)


def state_cases(vocab):
    """[(name, state)] over a vocabulary of `vocab` rows and N_CTX positions.  Every state
    starts with a stale pos / token and with both key parities full of live keys below the
    ones the case places, so that a cleared or a kept parity shows."""
    rng = np.random.default_rng(vocab)
    V = vocab
    cases = []

    def add(name, pos_next, token_in=-5, token_in_pos=None, read=(), other=(), seq=41, clear_read=False):
        st = np.zeros((), dtype=STEP_STATE)
        st["token_in"], st["pos_next"], st["seq"] = token_in, pos_next, seq
        st["token_in_pos"] = pos_next + 3 if token_in_pos is None else token_in_pos
        st["pos"], st["token"] = 0x5A5A, -77
        # background keys: high words in [2^28, 2^29), tokens inside the vocabulary and none
        # of them one that the case places (a maximum that misses a lane names another token)
        placed = {0xFFFFFFFF - (kv & 0xFFFFFFFF) for _, kv in list(read) + list(other)}

        def other_token():
            t = int(rng.integers(0, V))
            while t in placed:
                t = (t + 1) % V
            return t

        bg = [[key(int(rng.integers(1 << 28, 1 << 29)), other_token()) for _ in range(64)] for _ in range(2)]
        st["key"][:] = np.array(bg, dtype=np.uint64)
        rp = (pos_next + 1) & 1
        if clear_read:
            st["key"][rp] = 0
        for lane, kv in read:
            st["key"][rp][lane] = kv
        for lane, kv in other:
            st["key"][1 - rp][lane] = kv
        cases.append((name, st))

    BIG = 0xC0000000
    add("host_token", 5, token_in=7 % V, token_in_pos=5, read=[(9, key(BIG, 9 % V + 1))], other=[(3, key(BIG, 11 % V + 2))])
    add("host_token_odd", 6, token_in=V - 1, token_in_pos=6, read=[(9, key(BIG, 2))])
    add("feedback", 6, token_in=7 % V, read=[(17, key(BIG, 9))], other=[(17, key(BIG + 5, 11))])
    add("feedback_odd", 7, token_in=7 % V, read=[(50, key(BIG, 13))], other=[(2, key(0xFFFFFFFF, 12))])
    for k in range(64):
        add(f"max_in_lane_{k}", k % 7, read=[(k, key(BIG + k, (5 * k + 3) % V))])
    # key order
    add("top_bit", 3, read=[(4, key(0xC0123456, 3)), (37, key(0x40123456, 4))])
    add("top_bit_swapped", 4, read=[(4, key(0x40123456, 4)), (37, key(0xC0123456, 3))])
    add("hi_low_bit", 3, read=[(8, key(0x90000001, V - 1)), (41, key(0x90000000, 0))])
    add("hi_low_bit_swapped", 4, read=[(8, key(0x90000000, 0)), (41, key(0x90000001, V - 1))])
    add("equal_hi", 2, read=[(3, key(BIG, 9)), (40, key(BIG, 5))])
    add("equal_hi_swapped", 5, read=[(3, key(BIG, 5)), (40, key(BIG, 9))])
    add("id_zero", 1, read=[(63, key(BIG, 0)), (0, key(BIG, 1))])
    add("id_last", 2, read=[(0, key(BIG, V - 1))])
    add("negative_logits_only", 2, read=[(l, key(0x10000000 + l, l % 8 + 2)) for l in range(64)])
    add("empty_keys", 4, clear_read=True)
    # clamps
    for name, t in (("m1", -1), ("vocab", V), ("int_max", I32_MAX), ("int_min", I32_MIN)):
        add(f"clamp_token_in_{name}", 3, token_in=t, token_in_pos=3, read=[(5, key(BIG, 6))])
    add("clamp_key_vocab", 3, read=[(5, key(BIG, V))])
    add("clamp_key_negative", 4, read=[(60, key(BIG, 0x80000005))])
    # positions
    for p in (0, N_CTX - 1, N_CTX, N_CTX + 5, -1):
        add(f"pos_{p}_host", p, token_in=(p + 9) % V, token_in_pos=p)
        add(f"pos_{p}_feedback", p, read=[(p & 63, key(BIG, (p + 17) % V))])
    add("seq_wraps", 3, seq=0xFFFFFFFF, read=[(1, key(BIG, 2))])
    add("seq_zero", 3, seq=0, token_in=1, token_in_pos=3)
    return cases


# ---- k_pf_embed -------------------------------------------------------------------------------
def pf_ref(table, tokens, hist, pos0, n_ctx):
    """(x rows, history after) of k_pf_embed: ids outside the vocabulary read row 0, and the
    history records the clamped id, up to n_ctx - 1."""
    V = table.shape[0]
    tok = np.asarray(tokens, dtype=np.int64)
    tok = np.where((tok < 0) | (tok >= V), 0, tok)
    hist = np.array(hist, dtype=np.int32)
    n = max(0, min(len(tok), n_ctx - pos0))
    hist[0, pos0: pos0 + n] = tok[:n]
    return table[tok], hist


def pf_token_cases(vocab):
    """[(name, tokens, pos0, n_ctx)]: T in 1, 33, 600, ids outside the vocabulary among the
    tokens, pos0 + T inside, ending on and crossing n_ctx."""
    rng = np.random.default_rng(7)
    out = []
    for T in (1, 33, 600):
        tok = rng.integers(0, vocab, T).astype(np.int64)
        for j, bad in enumerate((-1, vocab, I32_MAX, I32_MIN)):
            if T > 1:
                tok[(7 * j + 2) % T] = bad
        out.append((f"T{T}-inside", tok.copy(), 2, T + 5))
        out.append((f"T{T}-to-the-end", tok.copy(), 3, T + 3))
        out.append((f"T{T}-crossing", tok.copy(), 4, T + 4 - (T + 1) // 2))
        out.append((f"T{T}-past", tok.copy(), T + 9, T + 9))
    out.append(("T1-bad-id", np.array([vocab]), 0, 4))
    return out
