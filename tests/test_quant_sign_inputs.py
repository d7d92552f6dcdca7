"""The inputs of tests/test_gpu_quant_sign.py do what their names say (CPU).

For every case of quant_sign_cases.cases(), at every column count the GPU tests use, plain and
through the RMSNorm: the oracle's q8_K image equals an independent NumPy restatement of
quantize_row_q8_K_ref and its block scales are finite; every planted block takes the branch of
the kernel's sign logic it is named for (P > N, N > P, P == N, or the zero block), with the
sign ggml's first-index scan keeps; and the mixed-lanes case has exactly one tied block."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as po
from helpers import Q4_K
from quant_sign_cases import branch_of, cases, norm_weight, q8k_ref

COLS = [256, 512, 2048, 4096, 14336]


def _inputs(cols, norm):
    rng = np.random.default_rng(5 + cols)
    for name, x, planted, idx in cases(cols):
        y = po.rms_norm_mul(x, norm_weight(cols, idx, rng), 1e-5) if norm else x
        yield name, y, planted


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("cols", COLS)
def test_oracle_matches_numpy_restatement(cols, norm):
    for name, y, _ in _inputs(cols, norm):
        ref = po.quantize_act(Q4_K, y)
        d = ref.reshape(-1, 292)[:, 0:4].copy().view(np.float32)
        assert np.isfinite(d).all(), f"{name}: non-finite block scale in the oracle's image"
        assert np.array_equal(ref, q8k_ref(y)), f"{name}: oracle and NumPy restatement differ"


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("cols", COLS)
def test_cases_take_their_branch(cols, norm):
    seen = set()
    for name, y, planted in _inputs(cols, norm):
        blocks = y.reshape(-1, 256)
        ref = po.quantize_act(Q4_K, y).reshape(-1, 292)
        for b, want in planted.items():
            got = branch_of(blocks[b])
            assert got == want, f"{name}: block {b} takes {got}, meant {want}"
            seen.add(got[0])
            # the sign ggml kept: d = 1 / (-127 / max) has the sign of -max
            d = float(ref[b, 0:4].copy().view(np.float32)[0])
            assert np.sign(d) == -want[1], f"{name}: block {b} scale {d}, meant sign {-want[1]}"
        if name == "tie_in_one_block_of_the_row":
            ties = [b for b in range(blocks.shape[0]) if branch_of(blocks[b])[0] == "tie"]
            assert ties == list(planted), f"{name}: tied blocks {ties}"
    assert seen == {"pos", "neg", "tie", "zero"}
