"""The embeddings surface of the C ABI without a GPU: the entry points exist and agree with
the header and the ctypes table, llmi_embd_pool refuses every bad argument before any device
call and names it, and the getters and setters fail loudly on a NULL context."""
from __future__ import annotations

import ctypes as C

import pytest

import llmi
from llmi._lib import SIGNATURES, last_error, lib
from test_abi import declared_functions, exported_symbols

NAMES = ("llama_set_embeddings", "llmi_set_pooling_type", "llama_pooling_type", "llmi_model_pooling_type",
         "llama_get_embeddings_seq", "llama_get_embeddings_ith", "llama_get_embeddings", "llmi_embd_pool")


def test_exports_signatures_and_header_agree():
    decl, exp = declared_functions(), exported_symbols()
    for n in NAMES:
        assert n in decl, f"{n} is not declared in include/llmi.h"
        assert n in exp, f"{n} is not exported"
        assert n in SIGNATURES, f"{n} has no ctypes signature"
    res, args = SIGNATURES["llmi_embd_pool"]
    assert res is C.c_int32 and len(args) == 12
    assert SIGNATURES["llama_get_embeddings_seq"][0] == C.POINTER(C.c_float)


def test_pooling_constants_match_the_header():
    src = open(__import__("test_abi").HDR).read()
    for name, v in (("UNSPECIFIED", -1), ("NONE", 0), ("MEAN", 1), ("CLS", 2), ("LAST", 3), ("RANK", 4)):
        assert f"#define LLMI_POOLING_TYPE_{name} {v}\n" in src
        assert getattr(llmi, f"POOLING_{name}") == v


# a valid call's arguments (the pointers are never followed: every refusal comes first)
P = 0x1000
GOOD = dict(x_dev=P, ldx=512, n_tok=4, n_embd=256, norm_w_dev=P, eps=1e-5, pooling=llmi.POOLING_MEAN, n_total=8, t0=2,
            acc_dev=P, out_dev=P)
REFUSALS = [
    ("x_dev", dict(x_dev=0)),
    ("norm_w_dev", dict(norm_w_dev=0)),
    ("out_dev", dict(out_dev=0)),
    ("acc_dev", dict(acc_dev=0)),
    ("n_embd", dict(n_embd=0)),
    ("n_embd", dict(n_embd=-256)),
    ("n_embd", dict(n_embd=384, ldx=512)),
    ("ldx", dict(ldx=255)),
    ("n_tok", dict(n_tok=0)),
    ("n_tok", dict(n_tok=-1)),
    ("t0", dict(t0=-1)),
    ("n_total", dict(n_total=5)),
    ("pooling", dict(pooling=-1)),
    ("pooling", dict(pooling=4)),
]


@pytest.mark.parametrize("field,change", REFUSALS, ids=[f"{f}-{i}" for i, (f, _) in enumerate(REFUSALS)])
def test_embd_pool_refuses_before_any_device_call(field, change):
    a = {**GOOD, **change}
    with pytest.raises(llmi.LlmiError) as e:
        llmi.embd_pool(**a)
    msg = str(e.value)
    assert "returned -1" in msg and "llmi_embd_pool: " in msg and field in msg, msg


def test_acc_may_be_null_unless_mean():
    """NONE / CLS / LAST with a null acc pass the argument checks: the refusal that follows
    names another argument (ldx), so acc was accepted."""
    for pooling in (llmi.POOLING_NONE, llmi.POOLING_CLS, llmi.POOLING_LAST):
        with pytest.raises(llmi.LlmiError) as e:
            llmi.embd_pool(**{**GOOD, "pooling": pooling, "acc_dev": 0, "ldx": 8})
        assert "ldx" in str(e.value) and "acc_dev" not in str(e.value)


def test_null_context():
    L = lib()
    assert L.llmi_set_pooling_type(None, llmi.POOLING_MEAN) == -1 and "ctx" in last_error()
    assert L.llama_pooling_type(None) == llmi.POOLING_UNSPECIFIED and "ctx" in last_error()
    assert L.llmi_model_pooling_type(None) == -1 and "model" in last_error()
    for get in (lambda: L.llama_get_embeddings_seq(None, 0), lambda: L.llama_get_embeddings_ith(None, 0),
                lambda: L.llama_get_embeddings(None)):
        assert not get() and "ctx" in last_error()
    L.llama_set_embeddings(None, True)  # no crash
    assert "ctx" in last_error()


@pytest.mark.parametrize("bad", [4, 7, -1])
def test_set_pooling_type_refuses_rank_and_unknown_values(bad):
    """RANK (4) and values that are no pooling type are refused with `type` named.  The value
    is checked before the context, so the refusal can be asked for without a GPU (the same
    on a real context: tests/test_gpu_embeddings.py)."""
    L = lib()
    assert L.llmi_set_pooling_type(None, bad) == -1
    err = last_error()
    assert err.startswith("llmi_set_pooling_type: type ") and str(bad) in err and "ctx" not in err
