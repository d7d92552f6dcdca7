"""The batched-matvec hook's C surface without a GPU: llmi_bmv is exported, and every bad
argument is rejected before any device call (the pointers are never dereferenced), as is
kernel 1 on arguments the matrix-core kernels do not take: never a fall-back to k_mvn."""
from __future__ import annotations

import pytest

import llmi
from helpers import Q4_K, Q6_K, Q8_0


def call(type=Q4_K, w=1, rows=32, cols=512, x=1, nw=None, eps=1e-5, nt=3, y=1, kernel=0):
    return llmi.lib().llmi_bmv(type, w, rows, cols, x, nw, eps, nt, y, kernel)


def test_bmv_symbol_is_exported():
    assert hasattr(llmi.lib(), "llmi_bmv")


@pytest.mark.parametrize("bad", [dict(nt=0), dict(nt=9), dict(nt=-1), dict(cols=300), dict(cols=0), dict(cols=-256),
                                 dict(rows=0), dict(rows=-16), dict(type=2), dict(type=-1), dict(type=15), dict(w=None),
                                 dict(x=None), dict(y=None), dict(kernel=-1), dict(kernel=2)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bmv_rejects_bad_arguments(bad):
    for kernel in (0, 1):
        args = dict(kernel=kernel)
        args.update(bad)
        assert call(**args) < 0, args
        assert "llmi_bmv" in llmi.last_error(), args


@pytest.mark.parametrize("bad", [dict(type=Q8_0), dict(rows=24), dict(rows=7)], ids=["q8_0", "rows24", "rows7"])
def test_bmv_matrix_core_kernel_never_falls_back(bad):
    """kernel 1 on what bmm_ok refuses (a Q8_0 weight, rows no multiple of 16) is an error,
    not a k_mvn launch."""
    assert call(kernel=1, **bad) < 0
    assert "llmi_bmv" in llmi.last_error()


def test_bmv_matrix_core_kernel_refuses_x86_without_dma(monkeypatch):
    """The x86 fold is k_bmd's only: under LLMI_BMM_DMA=0 (k_bmm, read per launch) kernel 1
    refuses x86 numerics."""
    monkeypatch.setenv("LLMI_BMM_DMA", "0")
    old = llmi.test_option("numerics", 1)
    try:
        assert call(type=Q6_K, kernel=1) < 0
        assert "llmi_bmv" in llmi.last_error()
    finally:
        llmi.test_option("numerics", old)
