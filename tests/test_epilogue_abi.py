"""The epilogue hook's C surface without a GPU: llmi_mv_epilogue is exported, every bad
argument is rejected before any device call (the device pointers are never dereferenced),
and a kernel asked for on arguments it does not take is an error, never another kernel."""
from __future__ import annotations

import ctypes as C

import pytest

import llmi
from helpers import Q4_K, Q5_K, Q6_K, Q8_0
from llmi._lib import EPI_LOGITS, EPI_QKV, EPI_SWIGLU, llmi_epilogue_args

DEV = 0x1000  # a non-null "device pointer": no valid call gets as far as using it


def make(epi, kernel=1, types=None, rows=None, cols=256, nt=3, pos=(0, 5, 255), **over):
    n = {EPI_QKV: 3, EPI_SWIGLU: 2, EPI_LOGITS: 1}.get(epi, 1)
    types = types or (Q4_K,) * n
    rows = rows or {EPI_QKV: (256, 128, 128), EPI_SWIGLU: (80, 80)}.get(epi, (96,))
    a = llmi_epilogue_args()
    a.kernel, a.epi, a.cols, a.eps, a.nt = kernel, epi, cols, 1e-5, nt
    for i in range(n):
        a.type[i], a.w_dev[i], a.rows[i] = types[i], DEV, rows[i]
    a.x_dev = a.norm_w_dev = a.rope_dev = a.q_dev = a.kc_dev = a.vc_dev = a.y_dev = DEV
    a.head_dim, a.n_rot, a.n_ctx = 64, 64, 256
    keep = [(C.c_int32 * 8)(*(list(pos) + [0] * 8)[:8]), (C.c_int32 * 8)(), (C.c_int32 * 8)()]
    a.pos, a.token_out, a.pos_next_out = keep
    for k, v in over.items():
        if k.startswith("w_dev") or k.startswith("type") or k.startswith("rows"):
            name, i = k[:-1], int(k[-1])
            getattr(a, name)[i] = v
        else:
            setattr(a, k, v)
    return a, keep


def refused(a):
    rc = llmi.lib().llmi_mv_epilogue(C.byref(a[0]))
    return rc < 0 and "llmi_mv_epilogue" in llmi.last_error()


def test_symbol_is_exported():
    assert hasattr(llmi.lib(), "llmi_mv_epilogue")
    assert llmi.lib().llmi_mv_epilogue(None) < 0


COMMON_BAD = [dict(kernel=-1), dict(kernel=5), dict(cols=300), dict(cols=0), dict(cols=-256), dict(nt=0), dict(nt=9),
              dict(nt=-1), dict(type0=2), dict(type0=-1), dict(type0=15), dict(w_dev0=None), dict(rows0=0), dict(rows0=-16),
              dict(x_dev=None), dict(norm_w_dev=None)]
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())  # noqa: E731


@pytest.mark.parametrize("epi", [EPI_QKV, EPI_SWIGLU, EPI_LOGITS], ids=["qkv", "swiglu", "logits"])
@pytest.mark.parametrize("bad", COMMON_BAD, ids=_ids)
def test_rejects_bad_common_arguments(epi, bad):
    for kernel in (1, 2):
        args = dict(kernel=kernel)
        args.update(bad)
        assert refused(make(epi, **args)), args


@pytest.mark.parametrize("epi", [0, 1, 5, -1])
def test_rejects_other_epilogues(epi):
    assert refused(make(epi))


@pytest.mark.parametrize("bad", [dict(n_rot=63), dict(n_rot=66), dict(n_rot=-2), dict(head_dim=0), dict(head_dim=63),
                                 dict(rows0=250), dict(rows1=100, rows2=100), dict(rows2=64), dict(n_ctx=0),
                                 dict(pos=(0, 5, 256)), dict(pos=(-1, 5, 255)), dict(rope_dev=None), dict(q_dev=None),
                                 dict(kc_dev=None), dict(vc_dev=None), dict(w_dev2=None), dict(type2=3), dict(rows2=0)],
                         ids=_ids)
def test_rejects_bad_qkv_arguments(bad):
    for kernel in (1, 2):
        args = dict(kernel=kernel)
        args.update(bad)
        assert refused(make(EPI_QKV, **args)), bad


def test_rejects_null_positions():
    a = make(EPI_QKV)
    a[0].pos = None
    assert refused(a)
    b = make(EPI_LOGITS)
    b[0].pos = None
    assert refused(b)


@pytest.mark.parametrize("T,pos0", [(3, 254), (70, 187), (1, 256), (3, -1)])
def test_prefill_positions_must_fit_the_context(T, pos0):
    assert refused(make(EPI_QKV, kernel=3, nt=T, pos=(pos0,)))


def test_token_counts_per_kernel():
    assert refused(make(EPI_SWIGLU, kernel=0, nt=2))          # launch_matvec: one token
    assert refused(make(EPI_SWIGLU, kernel=3, nt=0))
    assert refused(make(EPI_QKV, kernel=4, nt=9, types=(Q4_K, Q4_K, Q6_K)))


@pytest.mark.parametrize("bad", [dict(rows1=96), dict(y_dev=None), dict(w_dev1=None), dict(type1=7)], ids=_ids)
def test_rejects_bad_swiglu_arguments(bad):
    assert refused(make(EPI_SWIGLU, **bad))


def test_rejects_bad_logits_arguments():
    assert refused(make(EPI_LOGITS, y_dev=None))
    assert refused(make(EPI_LOGITS, pos=(0, -1, 3)))
    for f in ("token_out", "pos_next_out"):
        a = make(EPI_LOGITS)
        setattr(a[0], f, None)
        assert refused(a), f


def test_a_kernel_never_stands_in_for_another():
    """What the requested kernel does not take is an error on the host."""
    assert refused(make(EPI_LOGITS, kernel=3))                                    # the prefill GEMM has no LOGITS
    assert refused(make(EPI_SWIGLU, kernel=4))                                    # launch_bmm_qkv2: QKV only
    assert refused(make(EPI_QKV, kernel=4))                                       # ... of two type groups
    assert refused(make(EPI_QKV, kernel=4, types=(Q4_K, Q6_K, Q5_K)))             # three groups
    assert refused(make(EPI_QKV, kernel=4, types=(Q8_0, Q8_0, Q6_K)))             # bmm_ok: K-quants only
    assert refused(make(EPI_QKV, kernel=2, types=(Q8_0, Q8_0, Q8_0)))
    assert refused(make(EPI_QKV, kernel=2, types=(Q8_0, Q8_0, Q6_K)))             # no k_mvn for the Q8_0 group
    assert refused(make(EPI_LOGITS, kernel=2, rows=(33,)))                        # rows % 16
    assert refused(make(EPI_LOGITS, kernel=2, types=(Q8_0,)))
    assert refused(make(EPI_SWIGLU, kernel=2, types=(Q4_K, Q6_K)))                # one type per launch
    assert refused(make(EPI_SWIGLU, kernel=1, types=(Q4_K, Q6_K)))
    assert refused(make(EPI_SWIGLU, kernel=0, nt=1, types=(Q4_K, Q8_0)))          # two activation kinds
    assert refused(make(EPI_SWIGLU, kernel=3, types=(Q4_K, Q8_0)))
    assert refused(make(EPI_SWIGLU, kernel=3, rows=(40, 40)))                     # pf_gemm_ok: rows % 16
    assert refused(make(EPI_QKV, kernel=0, nt=1, rows=(258, 129, 129), head_dim=129, n_rot=0))  # odd head_dim


def test_matrix_core_kernels_refuse_x86_without_dma(monkeypatch):
    """The x86 fold is k_bmd's only: under LLMI_BMM_DMA=0 kernels 2 and 4 refuse x86 numerics."""
    monkeypatch.setenv("LLMI_BMM_DMA", "0")
    old = llmi.test_option("numerics", 1)
    try:
        assert refused(make(EPI_LOGITS, kernel=2))
        assert refused(make(EPI_QKV, kernel=4, types=(Q4_K, Q4_K, Q6_K)))
    finally:
        llmi.test_option("numerics", old)
