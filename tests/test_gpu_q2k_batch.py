"""Q2_K in the batched decode kernels: k_mvn, k_bmd (LLMI_BMM_DMA=1), k_bmm (=0) and the
two-group QKV launch k_bmd2, through llmi_mv_epilogue.  The oracle has no Q2_K: the logits rows
are held to q2k_cases.dot_f32 bit for bit, the QKV and SwiGLU epilogues to the same hook's
single-token kernel (k_matvec, pinned to dot_f32 by test_gpu_q2k.py), and one float64 reference
written from the block layout guards against a shared misreading of it."""
from __future__ import annotations

import numpy as np
import pytest

import epilogue_cases as ec
import llmi
import pyoracle as po
from helpers import Q4_K, first_diff, random_blocks
from llmi._lib import EPI_LOGITS, EPI_QKV, EPI_SWIGLU
from q2k_cases import Q2_K, act_image, dequant_f64, dot_f32, extreme_q2k, random_q2k, unpack
from q3k_cases import Q3_K, random_q3k
from test_gpu_batch import _batched, _prompts, _single_reference
from test_gpu_q3k_batch import hook  # llmi_mv_epilogue over sentinel-filled outputs

pytestmark = pytest.mark.gpu

CONTENTS = {"random": random_q2k, "extremes": extreme_q2k}
KERNELS = {"k_mvn": (1, 1), "k_bmd": (2, 1), "k_bmm": (2, 0)}  # (llmi_mv_epilogue kernel, LLMI_BMM_DMA)
# U = 1 (a one-stage round); U = 3; a full round and a one-stage tail; two full rounds; 17 tiles
# (the persistent tile loop); odd rows (k_mvn only: the matrix-core kernels take rows % 16 == 0)
SHAPES = [(16, 256), (48, 768), (32, 2304), (16, 4096), (272, 2048)]
POS = [0, ec.N_CTX - 1, 5, 6, 17, 17, 100, 3]


def logits_rows(kernel, raw, rows, cols, X, nw):
    return hook(kernel, EPI_LOGITS, (Q2_K,), [raw], (rows,), cols, X, nw, POS[:X.shape[0]])[0].view(np.float32)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("kname,rows,cols", [(k, *s) for k in KERNELS for s in SHAPES] + [("k_mvn", 7, 512)])
def test_logits_store_bit_equal_to_dot_f32(gpu, monkeypatch, kname, rows, cols, content):
    kernel, dma = KERNELS[kname]
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(rows * 131 + cols)
    raw = CONTENTS[content](rows, cols, rng)
    nw = rng.uniform(0.8, 1.2, cols).astype(np.float32)
    for nt in (1, 2, 3, 5, 8):
        X = (rng.standard_normal((nt, cols)) * 3).astype(np.float32)
        got = logits_rows(kernel, raw, rows, cols, X, nw)
        for t in range(nt):
            diff = first_diff(got[t], dot_f32(raw, po.quantize_act(Q4_K, po.rms_norm_mul(X[t], nw, 1e-5)), rows, cols))
            assert not diff, f"nt {nt}, token {t}: {diff}"


def same_as_single_token(kernel, epi, types, raws, rows, cols, rng, qkv=None):
    """Every batched token carries the bits of kernel 0 (k_matvec, nt = 1) on that token alone:
    q or h, and for QKV that token's K / V cache rows."""
    nw = rng.uniform(0.8, 1.2, cols).astype(np.float32)
    for nt in (3, 8):
        X = (rng.standard_normal((nt, cols)) * 3).astype(np.float32)
        got = hook(kernel, epi, types, raws, rows, cols, X, nw, POS[:nt], qkv)[:-1]
        for t in range(nt):
            ref = hook(0, epi, types, raws, rows, cols, X[t:t + 1], nw, POS[t:t + 1], qkv)[:-1]
            for i, (g, r) in enumerate(zip(got, ref)):
                assert np.array_equal(g[t], r[0]), f"nt {nt}, token {t}, output {i}: {first_diff(g[t].ravel(), r[0].ravel())}"


@pytest.mark.parametrize("cols", [256, 2048])
@pytest.mark.parametrize("vt", [Q3_K, Q4_K])
@pytest.mark.parametrize("kernel", [4, 1], ids=["k_bmd2", "k_mvn"])
def test_qkv_bit_equal_to_single_token(gpu, kernel, vt, cols):
    D, H, HK = 64, 4, 2
    rng = np.random.default_rng(cols + vt)
    rows = (D * H, D * HK, D * HK)
    v = random_q3k(rows[2], cols, rng) if vt == Q3_K else random_blocks(vt, rows[2], cols, rng)
    raws = [extreme_q2k(rows[0], cols, rng), random_q2k(rows[1], cols, rng), v]
    same_as_single_token(kernel, EPI_QKV, (Q2_K, Q2_K, vt), raws, rows, cols, rng, (D, HK))


@pytest.mark.parametrize("cols", [256, 2048])
@pytest.mark.parametrize("kernel", [1, 2], ids=["k_mvn", "k_bmd"])
def test_swiglu_bit_equal_to_single_token(gpu, kernel, cols):
    rows, rng = 272, np.random.default_rng(272 + cols)
    raws = [extreme_q2k(rows, cols, rng), random_q2k(rows, cols, rng)]
    same_as_single_token(kernel, EPI_SWIGLU, (Q2_K, Q2_K), raws, (rows, rows), cols, rng)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(48, 768), (32, 2304)])
def test_bmd_against_float64(gpu, rows, cols, content):
    """k_bmd, 8 tokens, against the float64 dequantized weights dotted with the float64 q8_K
    image; the bound derived in test_gpu_q2k.test_matvec_against_float64 (the operations and their
    order are the same): (U + 3) 2^-23 sum (|p1| + |p2|) per row.  The norm weight is all ones; the
    fused RMSNorm still divides by the RMS, so the image is that of rms_norm_mul(x)."""
    rng = np.random.default_rng(rows + cols)
    raw, nw = CONTENTS[content](rows, cols, rng), np.ones(cols, np.float32)
    X = rng.standard_normal((8, cols)).astype(np.float32)
    got = logits_rows(2, raw, rows, cols, X, nw)
    U = cols // 256
    q, sc, mn, d, dmin = unpack(raw)
    for t in range(8):
        da, a, bs = act_image(po.quantize_act(Q4_K, po.rms_norm_mul(X[t], nw, 1e-5)), U)
        isum = (np.repeat(sc, 16, axis=1) * q).reshape(rows, U, 256) * a[None]
        p1 = np.abs(da[None].astype(np.float64) * d.reshape(rows, U) * isum.sum(axis=2))
        p2 = np.abs(da[None].astype(np.float64) * dmin.reshape(rows, U) * (mn.reshape(rows, U, 16) * bs[None]).sum(axis=2))
        ref = np.einsum("rue,ue->r", dequant_f64(raw).reshape(rows, U, 256), da[:, None].astype(np.float64) * a)
        tol = (U + 3) * 2.0 ** -23 * (p1 + p2).sum(axis=1)
        err = np.abs(got[t].astype(np.float64) - ref)
        worst = int(np.argmax(err - tol))
        assert (err <= tol).all(), f"token {t}, row {worst}: |err| {err[worst]:.3g} > {tol[worst]:.3g}"


@pytest.fixture(scope="module")
def q2k_path(synth_dir):
    path = str(synth_dir / "tiny-q2k.gguf")
    llmi.write_synthetic_gguf(path, "tiny-q2k", seed=1)
    return path


@pytest.mark.parametrize("k,dma", [(2, 1), (3, 1), (8, 1), (8, 0)])
def test_model_batched_greedy_matches_single(gpu, monkeypatch, q2k_path, k, dma):
    """generate_greedy_batch raises where the model has no batched step, so passing also shows
    that the batched step ran: k = 2 through k_mvn, 3 and 8 on the matrix cores."""
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    prompts = _prompts(np.random.default_rng(40 + k), k)
    want, want_lg = _single_reference(q2k_path, prompts, 12, 256)
    got, got_lg, _ = _batched(q2k_path, prompts, 12, 256)
    assert got == want and all(np.array_equal(g, w) for g, w in zip(got_lg, want_lg))
