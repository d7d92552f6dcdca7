"""Q3_K weights on the GPU (generic numerics): the native decode matvec, get_rows, the prefill
GEMM and a Q3_K_M-shaped model end to end.

The oracle has no Q3_K, but it needs none: a Q3_K block is exactly a Q6_K block (the same d,
int8 scales scale - 32, quants q + 32), and ggml's generic vec_dot_q3_K_q8_K and
vec_dot_q6_K_q8_K run the same integer sums and the same fp32 operations in the same order.
So every Q3_K result must carry the bits of its Q6_K twin, whose path is pinned to the oracle.
A float64 dequantization written from the block layout alone (q3k_cases.py) guards the twin
converter and the kernels against a shared misreading of that layout.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import gguf_variants as gv
import llmi
import pyoracle as po
from helpers import Q4_K, Q5_K, Q6_K, empty_dev, first_diff, random_blocks, to_dev
from llmi._lib import STEP_PF_EMBED
from q3k_cases import Q3_K, dequant_f64, extreme_q3k, random_q3k, twin_q6k, unpack

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def repacked(qtype, raw, rows, cols):
    import torch

    L = llmi._lib.lib()
    nbytes = L.llmi_device_layout_bytes(qtype, rows, cols)
    assert nbytes > 0, llmi.last_error()
    rd, wd = to_dev(raw), empty_dev(nbytes)
    torch.cuda.synchronize()
    assert L.llmi_repack(qtype, _p(rd), _p(wd), rows, cols) == 0, llmi.last_error()
    return wd


def gpu_matvec(qtype, raw, rows, cols, x, nw=None, y0=None):
    """llmi_matvec: y = W x, or with y0 the residual-add epilogue y = y0 + W x (mode 1)."""
    import torch

    wd = repacked(qtype, raw, rows, cols)
    xd = to_dev(x.astype(np.float32))
    nd = to_dev(nw.astype(np.float32)) if nw is not None else None
    yd = to_dev(y0) if y0 is not None else torch.zeros(rows, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mode = 0 if y0 is None else 1
    assert llmi._lib.lib().llmi_matvec(qtype, _p(wd), rows, cols, _p(xd), _p(nd), 1e-5, _p(yd), mode) == 0, llmi.last_error()
    return yd.cpu().numpy()


CONTENTS = {"random": random_q3k, "extremes": extreme_q3k}
# one unit; odd rows; several row groups and a ragged last one; 4 rows per task; 32 units; 56
# units, which the add epilogue runs as the 8-wave wide launch (a plain store never goes wide);
# 112 units: sub-items with carried chains and the prologue's tail.  All of these have fewer
# than four tasks per CU and run as one-wave workgroups, one task each; (16384, 4096) has 4096
# tasks: the 4-wave kernel, several tasks per wave with the prefetch running across them.
SHAPES = [(2, 256), (7, 512), (130, 1024), (1024, 4096), (64, 8192), (333, 14336), (5, 28672), (16384, 4096)]


@pytest.mark.parametrize("epi", ["store", "add"])
@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_matvec_bit_equal_to_the_q6k_twin(gpu, rows, cols, content, epi):
    rng = np.random.default_rng(rows * 131 + cols)
    raw = CONTENTS[content](rows, cols, rng)
    x = rng.standard_normal(cols).astype(np.float32)
    y0 = rng.standard_normal(rows).astype(np.float32) if epi == "add" else None
    got = gpu_matvec(Q3_K, raw, rows, cols, x, y0=y0)
    ref = po.matvec(Q6_K, twin_q6k(raw), rows, cols, x)
    diff = first_diff(got, ref if y0 is None else y0 + ref)  # one f32 add per row, as the epilogue's
    assert not diff, diff


def test_matvec_fused_rmsnorm_bit_equal_to_the_twin(gpu):
    rows, cols = 96, 2048
    rng = np.random.default_rng(17)
    raw = random_q3k(rows, cols, rng)
    x = (rng.standard_normal(cols) * 4).astype(np.float32)
    w = rng.uniform(0.8, 1.2, cols).astype(np.float32)
    got = gpu_matvec(Q3_K, raw, rows, cols, x, w)
    diff = first_diff(got, po.matvec(Q6_K, twin_q6k(raw), rows, cols, po.rms_norm_mul(x, w, 1e-5)))
    assert not diff, diff


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(7, 512), (64, 8192)])
def test_matvec_against_float64(gpu, rows, cols, content):
    """Reference: the float64 dequantized weights dotted with the float64 dequantized q8_K
    image of the activation.  Tolerance per row, derived: a row is U = cols / 256 blocks of
    eight terms t = d_w d_a aux32[l], summed by eight U-step fp32 chains and eight final adds;
    each term is rounded twice (the product d_w d_a, then times aux32) and each add once, so
    the first-order bound is (U + 8) 2^-24 sum |t|; twice that is allowed."""
    rng = np.random.default_rng(rows + cols)
    raw = CONTENTS[content](rows, cols, rng)
    x = rng.standard_normal(cols).astype(np.float32)
    got = gpu_matvec(Q3_K, raw, rows, cols, x)
    U = cols // 256
    img = po.quantize_act(Q4_K, x).reshape(U, 292)  # block_q8_K: f32 d, int8 qs[256], int16 bsums[16]
    da = img[:, 0:4].copy().view(np.float32).reshape(U).astype(np.float64)
    a = img[:, 4:260].copy().view(np.int8).astype(np.int64)
    q, sc, dw = unpack(raw)
    prod = (np.repeat(sc, 16, axis=1) * q).reshape(rows, U, 256) * a[None]       # scale q a, exact
    aux = prod.reshape(rows, U, 32, 8).sum(axis=2)                               # aux32[l]: elements e % 8 == l
    terms = (dw.reshape(rows, U) * da[None])[:, :, None] * aux
    ref = np.einsum("rue,ue->r", dequant_f64(raw).reshape(rows, U, 256), da[:, None] * a)
    tol = (U + 8) * 2.0 ** -23 * np.abs(terms).sum(axis=(1, 2))
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(np.argmax(err - tol))
    assert (err <= tol).all(), f"row {worst}: |err| {err[worst]:.3g} > {tol[worst]:.3g}"


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("rows,cols", [(37, 256), (130, 1024)])
def test_get_rows_equal_the_float64_dequantization(gpu, rows, cols, content):
    """Every row through k_pf_embed's dequantization.  d (11 bits) * scale (6) * q (3) is
    exact in f32, so the rows equal the float64 dequantization bit for bit."""
    import torch

    rng = np.random.default_rng(rows)
    raw = CONTENTS[content](rows, cols, rng)
    wd = repacked(Q3_K, raw, rows, cols)
    toks = rng.permutation(rows)
    torch.cuda.synchronize()
    x, _, _, _, bad = llmi.step_entry(STEP_PF_EMBED, Q3_K, wd.data_ptr(), rows, cols, rows + 4,
                                      hist=np.zeros((1, rows + 4), dtype=np.int32), tokens=toks, pos0=0)
    ref = dequant_f64(raw).reshape(rows, cols)[toks].astype(np.float32)
    diff = first_diff(x.view(np.float32), ref)
    assert not diff and bad == [0, 0, 0], diff


@pytest.mark.parametrize("n_tok", [64, 65])
@pytest.mark.parametrize("rows,cols", [(256, 512), (128, 4096)])
def test_pf_gemm_bit_equal_to_the_q6k_twin(gpu, rows, cols, n_tok):
    import torch

    rng = np.random.default_rng(rows + cols + n_tok)
    raw = extreme_q3k(rows, cols, rng)
    xd = to_dev(rng.standard_normal((n_tok, cols)).astype(np.float32))
    out = []
    for qtype, blocks in ((Q3_K, raw), (Q6_K, twin_q6k(raw))):
        wd = repacked(qtype, blocks, rows, cols)
        y = torch.zeros((n_tok, rows), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert llmi._lib.lib().llmi_pf_gemm(qtype, _p(wd), rows, cols, _p(xd), None, 1e-5, n_tok, _p(y), None) == 0, llmi.last_error()
        out.append(y.cpu().numpy())
    diff = first_diff(out[0], out[1])
    assert not diff, diff


# ---- end to end: a Q3_K_M-shaped tiny model and its Q6_K twin -------------------------------
def _q3km_type(name, layer):
    """The Q3_K_M table (csrc/synth_writer.cpp) on the two-layer tiny preset: attn_v and ffn_down
    take Q5_K in layer 0 and Q4_K in layer 1, so both mixed QKV launches occur."""
    kind = name.split(".")[-2]
    if kind in ("token_embd", "attn_q", "attn_k", "ffn_gate", "ffn_up"):
        return Q3_K
    if kind in ("attn_v", "ffn_down"):
        return Q5_K if layer == 0 else Q4_K
    return Q4_K if kind == "attn_output" else Q6_K


def _q3km_files(base, out_dir):
    """(Q3_K_M file, the file with every Q3_K tensor replaced by its Q6_K twin)."""
    def edit(twin):
        def apply(g):
            for i, t in enumerate(g.tensors):
                if t.type == 0:  # norms stay f32
                    continue
                cols, rows = t.ne
                qt = _q3km_type(t.name, int(t.name.split(".")[1]) if t.name.startswith("blk.") else 0)
                rng = np.random.default_rng(900 + i)
                if qt != Q3_K:
                    g.replace_tensor(t.name, t.ne, qt, random_blocks(qt, rows, cols, rng).tobytes())
                else:
                    raw = random_q3k(rows, cols, rng)
                    g.replace_tensor(t.name, t.ne, Q6_K if twin else Q3_K, (twin_q6k(raw) if twin else raw).tobytes())
            g.set_kv("general.file_type", gv.U32, 12)
        return apply
    # gguf_reader.py and gguf_variants.py predate Q3_K and may not be edited: the reader's type
    # table learns the type here, and the files go through the module's own cached writer
    gv.gr.GGML_TYPES.setdefault(Q3_K, ("Q3_K", 256, 110))
    return gv._variant(base, out_dir, "q3km", edit(False)), gv._variant(base, out_dir, "q3km-twin", edit(True))


@pytest.fixture(scope="module")
def q3km(tiny_models, synth_dir):
    return _q3km_files(tiny_models["tiny-mixed"], synth_dir)


def _both(q3km, run):
    out = []
    for path in q3km:
        m = llmi.Model(path)
        out.append(run(m))
        m.close()
    return out


def test_model_decode_steps_bit_equal_to_the_twin(gpu, q3km):
    def run(m):
        assert ("ftype 12" in m.desc) and m.prefill_supported
        c = llmi.Context(m, n_ctx=64)
        lg, ids = [], []
        for pos, t in enumerate([1, 42, 7, 300]):
            assert c.decode([t], pos=[pos]) == 0
        for pos in range(4, 12):
            lg.append(c.logits(-1))
            ids.append(c.greedy(-1))
            assert c.decode([ids[-1]], pos=[pos]) == 0
        c.close()
        return np.stack(lg), ids
    (lq, iq), (lt, it) = _both(q3km, run)
    diff = first_diff(lq, lt)
    assert not diff and iq == it, (diff, iq, it)


def test_model_prefill_bit_equal_to_the_twin(gpu, q3km):
    rng = np.random.default_rng(5)
    prompt = [1] + [int(t) for t in rng.integers(3, 700, 69)]

    def run(m):
        assert m.prefill_supported
        c = llmi.Context(m, n_ctx=128)
        assert c.decode(prompt) == 0 and c.prefill_tokens == len(prompt) - 1
        lg = c.logits(-1)
        c.close()
        return lg
    lq, lt = _both(q3km, run)
    diff = first_diff(lq, lt)
    assert not diff, diff


def test_model_two_sequences_bit_equal_to_the_twin(gpu, q3km):
    """A step of two sequences in one llama_decode: the twin takes the batched kernels, the
    Q3_K file (which has none) the per-sequence path; the logits are the same bits."""
    def run(m):
        c = llmi.Context(m, n_ctx=64, n_seq=2)
        assert c.decode([1, 42, 7], seq=[0, 0, 0]) == 0 and c.decode([1, 9, 300, 5], seq=[1, 1, 1, 1]) == 0
        assert c.decode([11, 12], pos=[3, 4], seq=[0, 1], logits_all=True) == 0
        lg = np.stack([c.logits(0), c.logits(1)])
        c.close()
        return lg
    lq, lt = _both(q3km, run)
    diff = first_diff(lq, lt)
    assert not diff, diff


def test_model_refused_in_x86_numerics(gpu, q3km):
    with pytest.raises(llmi.LlmiError, match="q3_K"):
        llmi.Model(q3km[0], numerics=llmi.NUMERICS_X86)
