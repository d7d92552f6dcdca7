"""Q3_K in the batched decode kernels: k_mvn, k_bmd (LLMI_BMM_DMA=1) and k_bmm (=0), and the
mixed QKV launch k_bmd2.  A Q3_K block is its Q6_K twin (test_gpu_q3k.py), so every token's
result carries the oracle's bits for the twin; the epilogues are compared with the twin through
the same hook (its path is pinned to the oracle by test_gpu_epilogues.py); one float64
reference written from the block layout alone guards against a shared misreading of it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import epilogue_cases as ec
import llmi
import pyoracle as po
from helpers import Q4_K, Q5_K, Q6_K, first_diff, random_blocks, to_dev
from llmi._lib import EPI_LOGITS, EPI_QKV, EPI_SWIGLU, llmi_epilogue_args
from q3k_cases import Q3_K, dequant_f64, extreme_q3k, random_q3k, twin_q6k, unpack
from test_gpu_batch import _batched, _prompts, _single_reference
from test_gpu_epilogues import _i32, call, sentinel16, sentinel32
from test_gpu_matvec_edges import gpu_bmv
from test_gpu_q3k import repacked

pytestmark = pytest.mark.gpu

CONTENTS = {"random": random_q3k, "extremes": extreme_q3k}
KERNELS = {"k_mvn": (0, 1), "k_bmd": (1, 1), "k_bmm": (1, 0)}  # (llmi_bmv kernel, LLMI_BMM_DMA)
# U = 1 (a 12-B scale row, a one-stage round); U = 3 (scale rows never 16-B aligned past row 0);
# U = 9 (a full round and a one-stage tail); two full rounds; 17 tiles (the persistent loop)
SHAPES = [(16, 256), (48, 768), (32, 2304), (16, 4096), (272, 2048)]


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("kname,rows,cols", [(k, *s) for k in KERNELS for s in SHAPES] + [("k_mvn", 7, 512)])
def test_store_bit_equal_to_the_oracle_through_the_twin(gpu, monkeypatch, kname, rows, cols, content):
    kernel, dma = KERNELS[kname]
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(rows * 131 + cols)
    raw = CONTENTS[content](rows, cols, rng)
    wd, twin = repacked(Q3_K, raw, rows, cols), twin_q6k(raw)
    nw = rng.uniform(0.8, 1.2, cols).astype(np.float32)
    for nt in (1, 2, 3, 5, 8):
        X = (rng.standard_normal((nt, cols)) * 3).astype(np.float32)
        got = gpu_bmv(Q3_K, wd, rows, cols, X, kernel, nw)
        for t in range(nt):
            diff = first_diff(got[t], po.matvec(Q6_K, twin, rows, cols, po.rms_norm_mul(X[t], nw, 1e-5)))
            assert not diff, f"nt {nt}, token {t}: {diff}"


def hook(kernel, epi, types, raws, rows, cols, X, nw, pos, qkv=None):
    """llmi_mv_epilogue over sentinel-filled outputs; returns every output as host arrays."""
    nt, a = X.shape[0], llmi_epilogue_args()
    keep = [repacked(t, r, n, cols) for t, r, n in zip(types, raws, rows)] + [to_dev(X), to_dev(nw)]
    a.kernel, a.epi, a.cols, a.eps, a.nt, a.pos = kernel, epi, cols, 1e-5, nt, _i32(pos)
    for i, (t, n) in enumerate(zip(types, rows)):
        a.type[i], a.w_dev[i], a.rows[i] = t, keep[i].data_ptr(), n
    a.x_dev, a.norm_w_dev = keep[-2].data_ptr(), keep[-1].data_ptr()
    tok, nxt = _i32([-7] * nt), _i32([-7] * nt)
    a.token_out, a.pos_next_out = tok, nxt
    if qkv:
        D, HK = qkv
        out = [sentinel32(nt, rows[0]), sentinel16(nt, HK, ec.N_CTX, D), sentinel16(nt, HK, D, ec.N_CTX)]
        keep.append(to_dev(np.array(ec.rope_table(D, 10000.0))))
        a.head_dim, a.n_rot, a.n_ctx, a.rope_dev = D, D, ec.N_CTX, keep[-1].data_ptr()
        a.q_dev, a.kc_dev, a.vc_dev = (o.data_ptr() for o in out)
    else:
        out = [sentinel32(nt, rows[0])]
        a.y_dev = out[0].data_ptr()
    call(a)
    return [o.cpu().numpy() for o in out] + [np.array(list(tok) + list(nxt))]


def same_as_twin(kernel, epi, types, raws, rows, cols, rng, qkv=None):
    """The Q3_K call and the call with every Q3_K tensor replaced by its Q6_K twin: same bits."""
    nw = rng.uniform(0.8, 1.2, cols).astype(np.float32)
    twin_t = [Q6_K if t == Q3_K else t for t in types]
    twin_r = [twin_q6k(r) if t == Q3_K else r for t, r in zip(types, raws)]
    for nt in (3, 8):
        X = (rng.standard_normal((nt, cols)) * 3).astype(np.float32)
        pos = ([0, ec.N_CTX - 1, 5, 6, 17, 17, 100, 3])[:nt]
        got = hook(kernel, epi, types, raws, rows, cols, X, nw, pos, qkv)
        # (k_bmd2 has no (Q6_K, Q4_K / Q5_K) pair: the twin's QKV runs as two launches)
        ref = hook(2 if kernel == 4 else kernel, epi, twin_t, twin_r, rows, cols, X, nw, pos, qkv)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert np.array_equal(g.view(np.uint8), r.view(np.uint8)), f"nt {nt}, output {i}: {first_diff(g.ravel(), r.ravel())}"


@pytest.mark.parametrize("cols", [256, 2048])
@pytest.mark.parametrize("D,H,HK", [(64, 4, 2), (128, 2, 1)])
@pytest.mark.parametrize("vt", [Q4_K, Q5_K])
@pytest.mark.parametrize("kernel", [4, 2, 1], ids=["k_bmd2", "two-launches", "k_mvn"])
def test_qkv_bit_equal_to_the_twin(gpu, kernel, vt, D, H, HK, cols):
    rng = np.random.default_rng(cols + D + vt)
    rows = (D * H, D * HK, D * HK)
    raws = [extreme_q3k(rows[0], cols, rng), random_q3k(rows[1], cols, rng), random_blocks(vt, rows[2], cols, rng)]
    same_as_twin(kernel, EPI_QKV, (Q3_K, Q3_K, vt), raws, rows, cols, rng, (D, HK))


@pytest.mark.parametrize("cols", [256, 2048])
@pytest.mark.parametrize("kernel,dma,rows", [(1, 1, 80), (2, 1, 272), (2, 0, 272)], ids=["k_mvn", "k_bmd", "k_bmm"])
def test_swiglu_bit_equal_to_the_twin(gpu, monkeypatch, kernel, dma, rows, cols):
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(rows + cols)
    raws = [extreme_q3k(rows, cols, rng), random_q3k(rows, cols, rng)]
    same_as_twin(kernel, EPI_SWIGLU, (Q3_K, Q3_K), raws, (rows, rows), cols, rng)


@pytest.mark.parametrize("kernel,dma", [(1, 1), (2, 1), (2, 0)], ids=["k_mvn", "k_bmd", "k_bmm"])
def test_logits_bit_equal_to_the_twin(gpu, monkeypatch, kernel, dma):
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(3)
    same_as_twin(kernel, EPI_LOGITS, (Q3_K,), [random_q3k(1008, 768, rng)], (1008,), 768, rng)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(48, 768), (32, 2304)])
def test_bmd_against_float64(gpu, rows, cols, content):
    """k_bmd, 8 tokens, against the float64 dequantized weights dotted with the float64
    dequantized q8_K image; the bound derived in test_gpu_q3k.test_matvec_against_float64
    (the operations and their order are the same): (U + 8) 2^-23 sum |t| per row."""
    rng = np.random.default_rng(rows + cols)
    raw = CONTENTS[content](rows, cols, rng)
    X = rng.standard_normal((8, cols)).astype(np.float32)
    got = gpu_bmv(Q3_K, repacked(Q3_K, raw, rows, cols), rows, cols, X, 1)
    U = cols // 256
    q, sc, dw = unpack(raw)
    for t in range(8):
        img = po.quantize_act(Q4_K, X[t]).reshape(U, 292)  # block_q8_K: f32 d, int8 qs[256], int16 bsums[16]
        da = img[:, 0:4].copy().view(np.float32).reshape(U).astype(np.float64)
        a = img[:, 4:260].copy().view(np.int8).astype(np.int64)
        aux = ((np.repeat(sc, 16, axis=1) * q).reshape(rows, U, 256) * a[None]).reshape(rows, U, 32, 8).sum(axis=2)
        terms = (dw.reshape(rows, U) * da[None])[:, :, None] * aux
        ref = np.einsum("rue,ue->r", dequant_f64(raw).reshape(rows, U, 256), da[:, None] * a)
        tol = (U + 8) * 2.0 ** -23 * np.abs(terms).sum(axis=(1, 2))
        err = np.abs(got[t].astype(np.float64) - ref)
        worst = int(np.argmax(err - tol))
        assert (err <= tol).all(), f"token {t}, row {worst}: |err| {err[worst]:.3g} > {tol[worst]:.3g}"


@pytest.fixture(scope="module")
def q3km_path(synth_dir):
    path = str(synth_dir / "tiny-q3km.gguf")
    llmi.write_synthetic_gguf(path, "tiny-q3km", seed=1)
    return path


@pytest.mark.parametrize("k,dma", [(2, 1), (3, 1), (8, 1), (8, 0)])
def test_model_batched_greedy_matches_single(gpu, monkeypatch, q3km_path, k, dma):
    """generate_greedy_batch raises where the model has no batched step, so passing also shows
    that the batched step ran: k = 2 through k_mvn, 3 and 8 on the matrix cores."""
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    prompts = _prompts(np.random.default_rng(40 + k), k)
    want, want_lg = _single_reference(q3km_path, prompts, 12, 256)
    got, got_lg, c = _batched(q3km_path, prompts, 12, 256)
    assert got == want and all(np.array_equal(g, w) for g, w in zip(got_lg, want_lg))
    # one llama_decode of k sequences: each sequence's logits are its single decode's bits
    toks = [w[-1] for w in want]
    assert c.decode(toks, pos=[len(p) + 12 for p in prompts], seq=list(range(k)), logits_all=True) == 0
    m = llmi.Model(q3km_path)
    for s, p in enumerate(prompts):
        c1 = llmi.Context(m, n_ctx=256)
        assert c1.decode(p) == 0 and c1.generate_greedy(want[s][0], len(p), 12) == want[s][1:]
        assert c1.decode([toks[s]], pos=[len(p) + 12]) == 0
        assert np.array_equal(c.logits(s), c1.logits(-1)), f"sequence {s}"
        c1.close()
