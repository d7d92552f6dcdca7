"""Q2_K weights on the GPU (generic numerics): decode matvec, get_rows, prefill GEMM and a
Q2_K-mix model.  The oracle has no Q2_K; the references are q2k_cases.py's NumPy restatements
of ggml's generic vec_dot_q2_K_q8_K and dequantize_row_q2_K, written from the block layout."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gguf_variants as gv
import llmi
import pyoracle as po
from helpers import Q4_K, Q6_K, empty_dev, first_diff, random_blocks, to_dev
from llmi._lib import STEP_PF_EMBED
from q2k_cases import Q2_K, act_image, dequant_f32, dequant_f64, dot_f32, extreme_q2k, random_q2k, unpack
from q3k_cases import Q3_K, random_q3k

pytestmark = pytest.mark.gpu
CONTENTS = {"random": random_q2k, "extremes": extreme_q2k}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def repacked(raw, rows, cols):
    import torch

    L = llmi._lib.lib()
    nbytes = L.llmi_device_layout_bytes(Q2_K, rows, cols)
    assert nbytes > 0, llmi.last_error()
    rd, wd = to_dev(raw), empty_dev(nbytes)
    torch.cuda.synchronize()
    assert L.llmi_repack(Q2_K, _p(rd), _p(wd), rows, cols) == 0, llmi.last_error()
    return wd


def gpu_matvec(wd, rows, cols, x, nw=None, y0=None):
    """llmi_matvec: y = W x, or with y0 the residual-add epilogue y = y0 + W x (mode 1)."""
    import torch

    xd, nd = to_dev(x), to_dev(nw) if nw is not None else None
    yd = to_dev(y0) if y0 is not None else torch.zeros(rows, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert llmi._lib.lib().llmi_matvec(Q2_K, _p(wd), rows, cols, _p(xd), _p(nd), 1e-5, _p(yd), int(y0 is not None)) == 0, llmi.last_error()
    return yd.cpu().numpy()


# one unit; odd rows; a ragged last row group; sub-items with a carried chain; the 8-wave wide
# launch under add; the 4-wave kernel with several tasks per wave
@pytest.mark.parametrize("epi", ["store", "add"])
@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(2, 256), (7, 512), (130, 1024), (64, 8192), (333, 14336), (16384, 4096)])
def test_matvec_bit_equal_to_dot_f32(gpu, rows, cols, content, epi):
    rng = np.random.default_rng(rows * 131 + cols)
    raw = CONTENTS[content](rows, cols, rng)
    x = rng.standard_normal(cols).astype(np.float32)
    y0 = rng.standard_normal(rows).astype(np.float32) if epi == "add" else None
    ref = dot_f32(raw, po.quantize_act(Q4_K, x), rows, cols)
    diff = first_diff(gpu_matvec(repacked(raw, rows, cols), rows, cols, x, y0=y0), ref if y0 is None else y0 + ref)
    assert not diff, diff


def test_matvec_fused_rmsnorm_bit_equal_to_dot_f32(gpu):
    rows, cols = 96, 2048
    rng = np.random.default_rng(17)
    raw = random_q2k(rows, cols, rng)
    x, w = (rng.standard_normal(cols) * 4).astype(np.float32), rng.uniform(0.8, 1.2, cols).astype(np.float32)
    ref = dot_f32(raw, po.quantize_act(Q4_K, po.rms_norm_mul(x, w, 1e-5)), rows, cols)
    diff = first_diff(gpu_matvec(repacked(raw, rows, cols), rows, cols, x, w), ref)
    assert not diff, diff


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(7, 512), (64, 8192)])
def test_matvec_against_float64(gpu, rows, cols, content):
    """Reference: the float64 dequantized weights dotted with the float64 q8_K image.  Per row,
    block u adds p1 - p2 (p1 = d_a d isum, p2 = d_a dmin summs) onto the chain: two roundings per
    product, one for the subtraction, one for the chain add, so with e = 2^-24 its first-order
    error is e (2 |p1| + 2 |p2| + |p1 - p2| + |partial sum|) <= e (3 (|p1| + |p2|) + S), S = the
    sum of |p1| + |p2| over the row.  Over U = cols / 256 blocks: (U + 3) e S; twice that is allowed."""
    rng = np.random.default_rng(rows + cols)
    raw = CONTENTS[content](rows, cols, rng)
    x = rng.standard_normal(cols).astype(np.float32)
    got = gpu_matvec(repacked(raw, rows, cols), rows, cols, x)
    U = cols // 256
    da, a, bs = act_image(po.quantize_act(Q4_K, x), U)
    q, sc, mn, d, dmin = unpack(raw)
    isum = (np.repeat(sc, 16, axis=1) * q).reshape(rows, U, 256) * a[None]
    p1 = np.abs(da[None].astype(np.float64) * d.reshape(rows, U) * isum.sum(axis=2))
    p2 = np.abs(da[None].astype(np.float64) * dmin.reshape(rows, U) * (mn.reshape(rows, U, 16) * bs[None]).sum(axis=2))
    ref = np.einsum("rue,ue->r", dequant_f64(raw).reshape(rows, U, 256), da[:, None].astype(np.float64) * a)
    tol = (U + 3) * 2.0 ** -23 * (p1 + p2).sum(axis=1)
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"row {worst}: |err| {err[worst]:.3g} > {tol[worst]:.3g}"


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(37, 256), (130, 1024)])
def test_get_rows_equal_dequantize_row(gpu, rows, cols, content):
    import torch

    rng = np.random.default_rng(rows)
    raw = CONTENTS[content](rows, cols, rng)
    wd, toks = repacked(raw, rows, cols), rng.permutation(rows)
    torch.cuda.synchronize()
    x, _, _, _, bad = llmi.step_entry(STEP_PF_EMBED, Q2_K, wd.data_ptr(), rows, cols, rows + 4,
                                      hist=np.zeros((1, rows + 4), dtype=np.int32), tokens=toks, pos0=0)
    diff = first_diff(x.view(np.float32), dequant_f32(raw).reshape(rows, cols)[toks])
    assert not diff and bad == [0, 0, 0], diff


@pytest.mark.parametrize("n_tok", [64, 65])
@pytest.mark.parametrize("rows,cols", [(256, 512), (128, 4096)])
def test_pf_gemm_bit_equal_to_matvec(gpu, rows, cols, n_tok):
    import torch

    rng = np.random.default_rng(rows + cols + n_tok)
    wd = repacked(extreme_q2k(rows, cols, rng), rows, cols)
    x = rng.standard_normal((n_tok, cols)).astype(np.float32)
    y = torch.zeros((n_tok, rows), dtype=torch.float32, device="cuda")
    xd = to_dev(x)
    torch.cuda.synchronize()
    assert llmi._lib.lib().llmi_pf_gemm(Q2_K, _p(wd), rows, cols, _p(xd), None, 1e-5, n_tok, _p(y), None) == 0, llmi.last_error()
    diff = first_diff(y.cpu().numpy(), np.stack([gpu_matvec(wd, rows, cols, x[t]) for t in range(n_tok)]))
    assert not diff, diff


@pytest.mark.parametrize("kernel", [0, 1])
def test_bmv_declines(gpu, kernel):
    rows, cols = 32, 512
    wd, x, y = repacked(random_q2k(rows, cols, np.random.default_rng(1)), rows, cols), to_dev(np.ones((2, cols), np.float32)), empty_dev(2 * rows * 4)
    assert llmi._lib.lib().llmi_bmv(Q2_K, _p(wd), rows, cols, _p(x), None, 1e-5, 2, _p(y), kernel) < 0
    assert "llmi_bmv" in llmi.last_error()


@pytest.fixture(scope="module")
def q2k_model(tiny_models, synth_dir):
    """tiny-mixed (two layers) with upstream's Q2_K mix; attn_v is Q3_K in layer 0 and Q4_K in
    layer 1, so both two-group QKV launches occur."""
    def edit(g):
        for i, t in enumerate(g.tensors):
            if t.type == 0:  # norms stay f32
                continue
            (cols, rows), kind, rng = t.ne, t.name.split(".")[-2], np.random.default_rng(700 + i)
            if kind in ("token_embd", "attn_q", "attn_k", "ffn_gate", "ffn_up"):
                qt, raw = Q2_K, random_q2k(rows, cols, rng)
            elif kind == "output" or (kind == "attn_v" and t.name.startswith("blk.1.")):
                qt = Q6_K if kind == "output" else Q4_K
                raw = random_blocks(qt, rows, cols, rng)
            else:
                qt, raw = Q3_K, random_q3k(rows, cols, rng)
            g.replace_tensor(t.name, t.ne, qt, raw.tobytes())
        g.set_kv("general.file_type", gv.U32, 10)
    for t, v in ((Q2_K, ("Q2_K", 256, 84)), (Q3_K, ("Q3_K", 256, 110))):  # gguf_reader.py predates both types
        gv.gr.GGML_TYPES.setdefault(t, v)
    path = gv._variant(tiny_models["tiny-mixed"], synth_dir, "q2k", edit)
    m = llmi.Model(path)
    yield path, m
    m.close()


def test_model_prefill_equals_decode_and_two_sequences_equal_single(gpu, q2k_model):
    m = q2k_model[1]
    assert ("ftype 10" in m.desc) and m.prefill_supported
    prompt = [1] + [int(t) for t in np.random.default_rng(5).integers(3, 700, 69)]
    lg = []
    for batched in (False, True):  # 70 decode steps, then the 70-token prefill
        c = llmi.Context(m, n_ctx=128)
        if batched:
            assert c.decode(prompt) == 0 and c.prefill_tokens == len(prompt) - 1
        else:
            for pos, t in enumerate(prompt):
                assert c.decode([t], pos=[pos]) == 0
        lg.append(c.logits(-1))
        c.close()
    diff = first_diff(lg[1], lg[0])
    assert not diff, diff
    # one llama_decode step of two sequences (no batched kernels: one at a time) = the single steps
    heads = ([1, 42, 7], [1, 9, 300, 5])
    c = llmi.Context(m, n_ctx=64, n_seq=2)
    for s, h in enumerate(heads):
        assert c.decode(h, seq=[s] * len(h)) == 0
    assert c.decode([11, 12], pos=[3, 4], seq=[0, 1], logits_all=True) == 0
    both = [c.logits(0), c.logits(1)]
    c.close()
    for s, h in enumerate(heads):
        c = llmi.Context(m, n_ctx=64)
        assert c.decode(h) == 0 and c.decode([11 + s], pos=[len(h)]) == 0
        diff = first_diff(both[s], c.logits(-1))
        c.close()
        assert not diff, (s, diff)


def test_model_refused_in_x86_numerics(gpu, q2k_model):
    with pytest.raises(llmi.LlmiError, match="q2_K"):
        llmi.Model(q2k_model[0], numerics=llmi.NUMERICS_X86)
