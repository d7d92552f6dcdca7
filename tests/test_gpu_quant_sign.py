"""The q8_K activation quantization's signed maximum on the GPU, bit for bit (quant_sub).

The inputs of tests/quant_sign_cases.py (largest magnitude positive only, negative only, +a
before -a, -a before +a, ties inside one sub-block, across the sub-blocks of one DPP row, in the
first and last sub-block, in one block of an otherwise untied row, an all-negative block, one
nonzero element placed last, -0.0 beside a zero block) go, in generic and in x86 numerics
(quant_sub<0, 1>: the same sign logic, another store path), through
  llmi_quantize_act   plain and with the fused RMSNorm, at 256, 512 and 4096 columns, against
                      pyoracle.quantize_act (k_quant_dump: one 4-wave workgroup);
  llmi_matvec         Q4_K, so that the prologue of every workgroup shape k_matvec is launched
                      with runs them (mv_kernels.h mv_launch_np), against the oracle matvec:
                        64 x 2048, store      fewer than 4 tasks per CU: one-wave workgroups
                                              (mv_try_narrow), 2 register-held sub-blocks
                        8192 x 4096, store    2048 tasks of 4 rows, at least 4 per CU on a chip
                                              of up to 512 CUs: 4-wave workgroups (mv_launch)
                        16 x 14336, add       >= 12288 columns with the residual-add epilogue
                                              (mv_try_wide takes no plain store): 8-wave
                                              workgroups, 2 register-held sub-blocks per thread;
                                              y is preset and the reference is y + W x in f32
tests/test_quant_sign_inputs.py checks on the CPU that each input takes the branch it is named
for."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import llmi
import pyoracle as po
from helpers import Q4_K, empty_dev, first_diff, random_blocks, to_dev
from quant_sign_cases import cases, norm_weight

pytestmark = pytest.mark.gpu
EPS = 1e-5
NUMERICS = [0, 1]
NUM_IDS = ["generic", "x86"]


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


def gpu_quant(x, nw=None):
    import torch

    cols = x.size
    out = torch.zeros(cols // 256 * 292, dtype=torch.uint8, device="cuda")
    xd = to_dev(x)
    nd = to_dev(nw) if nw is not None else None
    torch.cuda.synchronize()
    assert llmi.lib().llmi_quantize_act(Q4_K, cols, _p(xd), _p(nd), EPS, _p(out)) == 0, llmi.last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("cols", [256, 512, 4096])
def test_quantize_act_signed_max(gpu, cols, norm, num):
    rng = np.random.default_rng(5 + cols)
    with numerics(num):
        for name, x, _, idx in cases(cols):
            nw = norm_weight(cols, idx, rng) if norm else None
            ref = po.quantize_act(Q4_K, po.rms_norm_mul(x, nw, EPS) if norm else x, x86=po.X86_ALL if num else 0)
            got = gpu_quant(x, nw)
            bad = np.flatnonzero(ref != got)
            assert bad.size == 0, (f"{name}: {bad.size} bytes differ, first in block {int(bad[0]) // 292} at byte "
                                   f"{int(bad[0]) % 292}: got {int(got[bad[0]])}, reference {int(ref[bad[0]])}")


# (rows, cols, accumulate): the one-wave, 4-wave and 8-wave workgroups (module docstring)
MV_SHAPES = [(64, 2048, False), (8192, 4096, False), (16, 14336, True)]


@pytest.mark.parametrize("num", NUMERICS, ids=NUM_IDS)
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "rmsnorm"])
@pytest.mark.parametrize("rows,cols,add", MV_SHAPES, ids=["narrow-64x2048", "wg4-8192x4096", "wide-16x14336-add"])
def test_matvec_signed_max(gpu, rows, cols, add, norm, num):
    import torch

    L = llmi.lib()
    rng = np.random.default_rng(rows * 131 + cols)
    raw = random_blocks(Q4_K, rows, cols, rng)
    y0 = rng.standard_normal(rows).astype(np.float32) if add else None
    with numerics(num):
        wd = empty_dev(L.llmi_device_layout_bytes(Q4_K, rows, cols))
        rd = to_dev(raw)
        torch.cuda.synchronize()
        assert L.llmi_repack(Q4_K, _p(rd), _p(wd), rows, cols) == 0, llmi.last_error()
        for name, x, _, idx in cases(cols):
            nw = norm_weight(cols, idx, rng) if norm else None
            ref = po.matvec(Q4_K, raw, rows, cols, po.rms_norm_mul(x, nw, EPS) if norm else x,
                            x86=po.X86_ALL if num else 0)
            if add:
                ref = (y0 + ref).astype(np.float32)  # the epilogue's one f32 add onto the residual
            assert np.isfinite(ref).all(), f"{name}: non-finite reference"
            xd, nd = to_dev(x), to_dev(nw) if norm else None
            yd = to_dev(y0) if add else torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rc = L.llmi_matvec(Q4_K, _p(wd), rows, cols, _p(xd), _p(nd), EPS, _p(yd), 1 if add else 0)
            assert rc == 0, llmi.last_error()
            d = first_diff(yd.cpu().numpy(), ref)
            assert not d, f"{name}: {d}"
