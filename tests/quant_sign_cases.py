"""Inputs for the signed maximum of the q8_K activation quantization (mv_device.h quant_sub).

ggml keeps the SIGNED value of the first element whose |y| is the block's largest.  The kernel
finds it from two order-free maxima per 256-block, P = max y and N = max -y: the sign is + when
P > N, - when N > P, and only P == N > 0 (+a and -a both present) needs the first index, which a
wave-uniform slow branch then computes for the whole wave.  Each case below is named for the
branch its planted blocks take; tests/test_quant_sign_inputs.py checks on the CPU that they do.

cases(cols) -> [(name, x, planted, idx)]: x is f32[cols]; planted maps a block index to the
branch it must take ("pos", "neg", "tie", "zero") and, for "tie", the sign of the first of the
two; idx lists the planted element indices (a fused-RMSNorm test gives these one common norm
weight, so that a tie stays a tie).  Everything outside the planted elements is |x| <= 1."""
from __future__ import annotations

import numpy as np

A = np.float32(4.0)  # the planted magnitude: above 1.5 * |base| whatever the norm weight


def _base(cols, rng):
    return rng.uniform(-1.0, 1.0, cols).astype(np.float32)


def _blocks(cols):
    """The blocks a pattern is planted in: the first and the last (one thread's first and, in
    a wide row, second sub-block)."""
    nb = cols // 256
    return sorted({0, nb - 1})


def cases(cols: int, seed: int = 0):
    rng = np.random.default_rng(1000 + cols + seed)
    nb = cols // 256
    out = []

    def plant(name, pairs, branch, blocks=None):
        """pairs: [(offset in the block, value)]"""
        x = _base(cols, rng)
        planted, idx = {}, []
        for b in (_blocks(cols) if blocks is None else blocks):
            for off, val in pairs:
                x[256 * b + off] = val
                idx.append(256 * b + off)
            planted[b] = branch
        out.append((name, x, planted, idx))

    plant("positive_only", [(77, A)], ("pos", +1))
    plant("negative_only", [(77, -A)], ("neg", -1))
    plant("plus_before_minus", [(5, A), (200, -A)], ("tie", +1))
    plant("minus_before_plus", [(5, -A), (200, A)], ("tie", -1))
    plant("tie_in_one_sub_block", [(16 * 3 + 2, A), (16 * 3 + 9, -A)], ("tie", +1))
    plant("tie_across_sub_blocks", [(16 * 2 + 1, -A), (16 * 11 + 4, A)], ("tie", -1))
    plant("tie_first_and_last_sub_block", [(3, A), (253, -A)], ("tie", +1))
    # one tied block among untied ones: the wave takes the slow branch with mixed lanes
    plant("tie_in_one_block_of_the_row", [(40, -A), (41, A)], ("tie", -1), blocks=[1 if nb > 1 else 0])

    x = _base(cols, rng)
    planted = {}
    for b in _blocks(cols):
        x[256 * b:256 * b + 256] = -np.abs(x[256 * b:256 * b + 256]) - np.float32(0.125)
        planted[b] = ("neg", -1)
    out.append(("all_negative_block", x, planted, []))

    x = _base(cols, rng)
    planted, idx = {}, []
    for k, b in enumerate(_blocks(cols)):  # +a in the first block, -a in the last
        x[256 * b:256 * b + 256] = 0.0
        x[256 * b + 255] = A if k == 0 else -A
        planted[b] = ("pos", +1) if k == 0 else ("neg", -1)
        idx.append(256 * b + 255)
    out.append(("one_nonzero_placed_last", x, planted, idx))

    # a +0 block, a block of mixed +0 / -0 (both the zero-block path), -0 entries in a live block
    x = _base(cols, rng)
    x[0:256] = 0.0
    x[0:256:3] = -0.0
    planted = {0: ("zero", 0)}
    if nb > 1:
        x[256:512] = 0.0
        planted[1] = ("zero", 0)
    if nb > 2:
        x[512:768:5] = -0.0
    out.append(("negative_zeros_beside_a_zero_block", x, planted, []))
    return out


def norm_weight(cols, idx, rng):
    """Random RMSNorm weights with one common value on the planted elements."""
    w = rng.uniform(0.5, 1.5, cols).astype(np.float32)
    w[idx] = np.float32(1.25)
    return w


def branch_of(block: np.ndarray):
    """(branch, sign of ggml's signed maximum) of one 256-element block, from P and N."""
    P, N = np.float32(block.max()), np.float32((-block).max())
    am = max(P, N, np.float32(0.0))
    if am == 0:
        return ("zero", 0)
    if P > N:
        return ("pos", +1)
    if N > P:
        return ("neg", -1)
    first = int(np.argmax(np.abs(block) == am))
    return ("tie", +1 if block[first] > 0 else -1)


def q8k_ref(x: np.ndarray) -> np.ndarray:
    """NumPy restatement of ggml's quantize_row_q8_K_ref: per 256-block {f32 d, int8 qs[256],
    int16 bsums[16]} (292 bytes), every operation in f32 as the C code has it."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 256)
    out = np.zeros((x.shape[0], 292), dtype=np.uint8)
    for b, xb in enumerate(x):
        ax = np.abs(xb)
        first = int(np.argmax(ax))  # 'if (ax > amax)': the first of the largest
        if ax[first] == 0:
            continue  # d = 0, qs = 0, bsums = 0
        iscale = np.float32(-127.0) / xb[first]
        v = (iscale * xb).astype(np.float32) + np.float32(12582912.0)  # nearest_int's magic constant
        q = np.minimum(127, (v.view(np.int32) & 0x007FFFFF) - 0x00400000).astype(np.int32)
        d = np.float32(1.0) / iscale
        out[b, 0:4] = np.array([d], dtype=np.float32).view(np.uint8)
        out[b, 4:260] = q.astype(np.int8).view(np.uint8)
        out[b, 260:292] = q.reshape(16, 16).sum(axis=1).astype(np.int16).view(np.uint8)
    return out.reshape(-1)
