"""Matvec and GEMM parity at the bounds of the exactness argument.

Every quantized linear kernel claims bit-equality with ggml's generic order (and with the
x86 order in x86 numerics) on the strength of magnitude bounds stated in comments
(prefill.hip header, batch.hip, mv_device.h unit_terms).  These tests feed the inputs
that sit ON those bounds (tests/helpers.py; checked on the CPU by
tests/test_matvec_edge_inputs.py) through every such kernel:

  weights      random | saturated (every quant and scale at the type's extreme, integer
               block sums equal to the bound) | near-saturated (the top and bottom two quants,
               the top four scales, |a| in 120..127; with random signs, and sign-aligned so
               that the sums sit within 14 % of the bound, Q6_K above 2^23, with varied low
               bits) | scale edges (fp16 d / dmin of +-0, +-2^-24, the largest
               subnormal, 2^-14, +-65504, +- a normal value)
  activations  normal | one all-zero 256-block | all zero | x * 1e-35 (d_w * d_a an f32
               subnormal) | x * 3e-5 (fp16-subnormal q8_0 d) | x * 1e30 (Q8_0: x * 1e5) |
               +-c constant (every q8 value +-127: all plus, all minus, random signs) |
               |a| in 120..127
  kernels      llmi_matvec (k_matvec at row-task geometries of 4, 8, 24, 32 and 64 lanes per
               row, the last with the unit loop; fused RMSNorm; the accumulate epilogue),
               llmi_pf_gemm (k_pf_gemm: the 32-token workgroups at small shapes, and both the
               64- and the 32-token workgroups on a grid that fills the chip; different
               families side by side in one MFMA tile),
               llmi_bmv kernel 0 (k_mvn) and kernel 1 (k_bmd, and k_bmm under
               LLMI_BMM_DMA=0)

Every comparison is bit-exact against the CPU oracle (po.matvec; x86 = X86_ALL in x86
numerics) on the uint32 views, so signed zeros count; every reference value is asserted
finite first, which keeps NaN out.  No family had to leave the matrix for a non-finite
reference: the huge family is simply not paired with the saturated and the scale-edge
weights (65504 * d_a * a block sum overflows f32 there by construction)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import llmi
import pyoracle as po
from helpers import (Q4_K, Q5_K, Q6_K, Q8_0, QTYPES, TNAME, edge_weight_sets, empty_dev, first_diff, random_blocks,
                     to_dev)

pytestmark = pytest.mark.gpu

IDS = [TNAME[t] for t in QTYPES]
KQUANTS = (Q4_K, Q5_K, Q6_K)
NUMERICS = [0, 1]
NUM_IDS = ["generic", "x86"]
EPS = 1e-5


class numerics:
    """llmi_test_option("numerics"): this thread's kernel-level hooks in generic (0) or
    x86 (1) numerics; llmi_repack's byte order follows it."""

    def __init__(self, num):
        self.num = num

    def __enter__(self):
        self.old = llmi.test_option("numerics", self.num)

    def __exit__(self, *exc):
        llmi.test_option("numerics", self.old)
        return False


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def oracle(qtype, raw, rows, cols, x, num, nw=None):
    """The reference of one row of activations: finite, or the comparison means nothing."""
    if nw is not None:
        x = po.rms_norm_mul(x, nw, EPS)
    y = po.matvec(qtype, raw, rows, cols, x, x86=po.X86_ALL if num else 0)
    assert np.isfinite(y).all(), "non-finite reference: this input does not belong in the matrix"
    return y


def repack(qtype, raw, rows, cols):
    import torch

    L = llmi.lib()
    nbytes = L.llmi_device_layout_bytes(qtype, rows, cols)
    assert nbytes > 0
    rd, wd = to_dev(raw), empty_dev(nbytes)
    torch.cuda.synchronize()
    assert L.llmi_repack(qtype, _p(rd), _p(wd), rows, cols) == 0, llmi.last_error()
    return wd


def norm_weight(wname, cols, rng):
    """Unit weights for the sets whose activations must stay (near-)saturated through the
    RMSNorm (a uniform scale keeps every q8 value), random ones otherwise."""
    if wname.startswith(("saturated", "near_saturated")):
        return np.ones(cols, dtype=np.float32)
    return rng.uniform(0.5, 1.5, cols).astype(np.float32)


def token_rows(acts, n, rng):
    """n activation rows, row t of family t mod len(acts): different families side by side
    in one launch."""
    names = [acts[t % len(acts)][0] for t in range(n)]
    return names, np.stack([acts[t % len(acts)][1](rng) for t in range(n)])


def check(got, ref, what):
    d = first_diff(got, ref)
    assert not d, f"{what}: {d}"


# ---- llmi_matvec (k_matvec) -----------------------------------------------------------------
def gpu_matvec(qtype, wd, rows, cols, x, nw=None, y0=None):
    import torch

    xd = to_dev(x)
    nd = to_dev(nw) if nw is not None else None
    yd = to_dev(y0) if y0 is not None else torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = llmi.lib().llmi_matvec(qtype, _p(wd), rows, cols, _p(xd), _p(nd), EPS, _p(yd), 1 if y0 is not None else 0)
    assert rc == 0, llmi.last_error()
    return yd.cpu().numpy()


# row-task geometry (kernels.hip mv_geometry: Lr lanes per row, R = 64 / Lr rows per task):
# Lr = 4 at 256 and 512 columns (one- and two-block rows), 4 at 1024, 32 at 8192, 24 at 5632,
# 64 with more than one unit per lane at 28672 (which also runs the prologue's tail loop)
MV_SHAPES = [(2, 256), (7, 512), (130, 1024), (64, 8192), (130, 5632), (5, 28672)]


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", MV_SHAPES)
def test_matvec_edges(gpu, qtype, rows, cols, num):
    rng = np.random.default_rng(rows * 131 + cols + qtype)
    with numerics(num):
        for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
            wd = repack(qtype, raw, rows, cols)
            for aname, make in acts:
                x = make(rng)
                ref = oracle(qtype, raw, rows, cols, x, num)
                check(gpu_matvec(qtype, wd, rows, cols, x), ref, f"{wname} x {aname}")


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
def test_matvec_edges_rmsnorm(gpu, qtype, norm, num):
    rows, cols = 96, 2048
    rng = np.random.default_rng(11 + qtype)
    with numerics(num):
        for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
            wd = repack(qtype, raw, rows, cols)
            nw = norm_weight(wname, cols, rng) if norm else None
            for aname, make in acts:
                x = make(rng)
                ref = oracle(qtype, raw, rows, cols, x, num, nw)
                check(gpu_matvec(qtype, wd, rows, cols, x, nw), ref, f"{wname} x {aname}")


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
def test_matvec_edges_accumulate(gpu, qtype, num):
    """mode 1: y += W . q(x) onto a non-zero y, one f32 add per row after the row's sum."""
    rows, cols = 130, 1024
    rng = np.random.default_rng(29 + qtype)
    with numerics(num):
        for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
            wd = repack(qtype, raw, rows, cols)
            for aname, make in acts:
                x = make(rng)
                y0 = rng.standard_normal(rows).astype(np.float32)
                y0[::7] = 0.0
                ref = y0 + oracle(qtype, raw, rows, cols, x, num)
                assert np.isfinite(ref).all()
                check(gpu_matvec(qtype, wd, rows, cols, x, y0=y0), ref, f"{wname} x {aname}")


# ---- llmi_pf_gemm (k_pf_gemm) --------------------------------------------------------------
# The launcher (prefill.hip pf_gemm_launch) takes the 64-token-workgroup kernel
# k_pf_gemm<.., NG = 2> only in generic numerics, with the pf_gemm_ng option at 2, above 32
# tokens, and when ceil(rows / 64) * ceil(T / 64) workgroups fill every CU; else the 32-token
# kernel (NG = 1), which x86 numerics always takes.  At PF_SHAPES the grid never fills the
# chip, so every case there is an NG = 1 launch whatever the option says (the two settings
# are kept as cases all the same); PF_NG2 is the shape at which the gate opens.
PF_SHAPES = [(32, 256), (96, 512), (160, 4096), (64, 14336)]
PF_CASES = [(n_tok, ng) for n_tok in (5, 33, 70) for ng in (2, 1) if ng == 2 or n_tok >= 33]
# 128 row blocks x 3 token groups (64 + 64 + 2 tokens) = 384 workgroups, two K stages
PF_NG2 = (8192, 512, 130)


def _pf_gemm_edges(qtype, rows, cols, n_tok, ng, num):
    import torch

    L = llmi.lib()
    rng = np.random.default_rng(rows + cols + n_tok + qtype)
    old = L.llmi_test_option(b"pf_gemm_ng", ng)
    try:
        with numerics(num):
            for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
                wd = repack(qtype, raw, rows, cols)
                names, X = token_rows(acts, n_tok, rng)
                ref = np.stack([oracle(qtype, raw, rows, cols, X[t], num) for t in range(n_tok)])
                xd = to_dev(X)
                yd = torch.full((n_tok, rows), float("nan"), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                rc = L.llmi_pf_gemm(qtype, _p(wd), rows, cols, _p(xd), None, EPS, n_tok, _p(yd), None)
                assert rc == 0, llmi.last_error()
                got = yd.cpu().numpy()
                for t in range(n_tok):
                    check(got[t], ref[t], f"{wname}, token {t} ({names[t]})")
    finally:
        L.llmi_test_option(b"pf_gemm_ng", old)


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", PF_SHAPES)
@pytest.mark.parametrize("n_tok,ng", PF_CASES)
def test_pf_gemm_edges(gpu, qtype, rows, cols, n_tok, ng, num):
    """The 32-token-workgroup kernel (NG = 1; x86: its x86 form) at the small shapes."""
    _pf_gemm_edges(qtype, rows, cols, n_tok, ng, num)


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("ng,num", [(2, 0), (1, 0), (2, 1)], ids=["ng2-generic", "ng1-generic", "x86"])
def test_pf_gemm_edges_full_grid(gpu, qtype, ng, num):
    """A grid that fills the chip: generic numerics with pf_gemm_ng 2 runs the 64-token
    workgroups (NG = 2, what a prompt above 64 tokens runs on a real model's wide weights),
    pf_gemm_ng 1 the 32-token ones on the same inputs; x86 its one kernel, with a ragged last
    token group in each."""
    import torch

    rows, cols, n_tok = PF_NG2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_tok > 32 and -(-rows // 64) * -(-n_tok // 64) >= cus, "the NG = 2 gate of pf_gemm_launch is not open here"
    _pf_gemm_edges(qtype, rows, cols, n_tok, ng, num)


# ---- llmi_bmv (k_mvn; k_bmd / k_bmm) -------------------------------------------------------
def gpu_bmv(qtype, wd, rows, cols, X, kernel, nw=None):
    import torch

    nt = X.shape[0]
    xd = to_dev(X)
    nd = to_dev(nw) if nw is not None else None
    yd = torch.full((nt, rows), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rc = llmi.lib().llmi_bmv(qtype, _p(wd), rows, cols, _p(xd), _p(nd), EPS, nt, _p(yd), kernel)
    assert rc == 0, llmi.last_error()
    return yd.cpu().numpy()


BMV_CASES = [(0, 1, t, s) for t in QTYPES for s in [(7, 512), (130, 1024), (64, 8192)]] + \
            [(1, dma, t, s) for dma in (1, 0) for t in KQUANTS for s in [(32, 256), (96, 4096), (64, 14336)]]
BMV_NT = {0: (1, 3, 5, 8), 1: (3, 5, 8)}
BMV_KNAME = {(0, 1): "k_mvn", (1, 1): "k_bmd", (1, 0): "k_bmm"}


def _bmv_id(c):
    kernel, dma, t, (rows, cols) = c
    return f"{BMV_KNAME[kernel, dma]}-{TNAME[t]}-{rows}x{cols}"


def _bmv_numerics(dma):
    return NUMERICS if dma else [0]  # the x86 fold is k_bmd's only: bmm_ok refuses x86 for k_bmm


BMV_PARAMS = [pytest.param(c, num, id=f"{_bmv_id(c)}-{NUM_IDS[num]}") for c in BMV_CASES for num in _bmv_numerics(c[1])]


@pytest.mark.parametrize("case,num", BMV_PARAMS)
def test_bmv_edges(gpu, monkeypatch, case, num):
    kernel, dma, qtype, (rows, cols) = case
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(rows * 17 + cols + qtype + kernel)
    with numerics(num):
        for wname, raw, acts in edge_weight_sets(qtype, rows, cols, rng):
            wd = repack(qtype, raw, rows, cols)
            for nt in BMV_NT[kernel]:
                # (rotate the families so that every one runs at some token count)
                names, X = token_rows(acts[nt % len(acts):] + acts[:nt % len(acts)], nt, rng)
                ref = np.stack([oracle(qtype, raw, rows, cols, X[t], num) for t in range(nt)])
                got = gpu_bmv(qtype, wd, rows, cols, X, kernel)
                for t in range(nt):
                    check(got[t], ref[t], f"{wname}, nt {nt}, token {t} ({names[t]})")


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("case,num", BMV_PARAMS)
def test_bmv_ordinary_inputs(gpu, monkeypatch, case, num, norm):
    """The batched kernels' first kernel-level oracle comparison: ordinary random blocks and
    normal activations at the same shapes, with and without the fused RMSNorm."""
    kernel, dma, qtype, (rows, cols) = case
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    rng = np.random.default_rng(rows + cols * 3 + qtype + kernel)
    raw = random_blocks(qtype, rows, cols, rng)
    nw = rng.uniform(0.5, 1.5, cols).astype(np.float32) if norm else None
    with numerics(num):
        wd = repack(qtype, raw, rows, cols)
        for nt in BMV_NT[kernel]:
            X = (rng.standard_normal((nt, cols)) * 3).astype(np.float32)
            ref = np.stack([oracle(qtype, raw, rows, cols, X[t], num, nw) for t in range(nt)])
            got = gpu_bmv(qtype, wd, rows, cols, X, kernel, nw)
            for t in range(nt):
                check(got[t], ref[t], f"nt {nt}, token {t}")
