"""The sequence-copy C ABI without a GPU: llama_kv_self_seq_cp and llmi_kv_seq_copy exist with
the declared signatures, llmi_kv_seq_copy refuses every bad argument with < 0 before any
device call, each refusal naming its argument, and llama_kv_self_seq_cp(NULL, ...) is false."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

import llmi
from llmi._lib import SIGNATURES

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "llmi.h")
POINTERS = ("kc_src", "vc_src", "hist_src", "kc_dst", "vc_dst", "hist_dst")
_P = C.c_void_p


def test_exports_and_signatures():
    L = llmi.lib()
    for name in ("llama_kv_self_seq_cp", "llmi_kv_seq_copy"):
        assert name in SIGNATURES and getattr(L, name) is not None
    assert SIGNATURES["llama_kv_self_seq_cp"] == (C.c_bool, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32])
    assert SIGNATURES["llmi_kv_seq_copy"] == (C.c_int32, [C.c_int32] * 5 + [_P] * 6 + [C.POINTER(C.c_double)])
    text = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("bool llama_kv_self_seq_cp(struct llama_context* ctx, llama_seq_id seq_src, llama_seq_id seq_dst, "
            "llama_pos p0, llama_pos p1);") in text
    assert ("int32_t llmi_kv_seq_copy(int32_t n_planes, int32_t head_dim, int32_t n_ctx, int32_t p0, int32_t p1, "
            "const uint16_t* kc_src, const uint16_t* vc_src, const int32_t* hist_src, uint16_t* kc_dst, "
            "uint16_t* vc_dst, int32_t* hist_dst, double* usec);") in text
    assert hasattr(llmi.Context, "seq_cp") and callable(llmi.kv_seq_copy)


def _copy(n_planes=3, head_dim=64, n_ctx=256, p0=0, p1=8, nulls=()):
    """The call with host addresses that are never dereferenced: every case here must be
    refused before the first device call."""
    fake = {name: None if name in nulls else _P(0x1000 * (i + 1)) for i, name in enumerate(POINTERS)}
    return llmi.lib().llmi_kv_seq_copy(n_planes, head_dim, n_ctx, p0, p1, *[fake[n] for n in POINTERS], None)


def test_null_pointers_are_refused_by_name():
    for name in POINTERS:
        assert _copy(nulls=(name,)) < 0, name
        assert name in llmi.last_error() and "null" in llmi.last_error(), (name, llmi.last_error())


@pytest.mark.parametrize("kw,word", [
    (dict(n_planes=0), "n_planes"), (dict(n_planes=-3), "n_planes"),
    (dict(head_dim=0), "head_dim"), (dict(head_dim=-8), "head_dim"), (dict(head_dim=60), "head_dim"),
    (dict(n_ctx=0), "n_ctx"), (dict(n_ctx=-256), "n_ctx"), (dict(n_ctx=200), "n_ctx"), (dict(n_ctx=264), "n_ctx"),
    (dict(p0=-1), "p0"), (dict(p0=8, p1=8), "p0"), (dict(p0=9, p1=8), "p0"), (dict(p0=0, p1=0), "p0"),
    (dict(p0=0, p1=-1), "p0"), (dict(p0=250, p1=257), "p1"), (dict(p0=256, p1=257), "p1"),
])
def test_bad_shapes_and_ranges_are_refused_by_name(kw, word):
    assert _copy(**kw) < 0, kw
    err = llmi.last_error()
    assert err.startswith("llmi_kv_seq_copy") and word in err, (kw, err)


def test_python_wrapper_raises_on_refusal():
    with pytest.raises(llmi.LlmiError, match="head_dim"):
        llmi.kv_seq_copy(3, 12, 256, 0, 8, 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000)
    with pytest.raises(llmi.LlmiError, match="vc_dst"):
        llmi.kv_seq_copy(3, 64, 256, 0, 8, 0x1000, 0x2000, 0x3000, 0x4000, 0, 0x6000)


def test_seq_cp_null_context_is_false():
    assert llmi.lib().llama_kv_self_seq_cp(None, 0, 1, 0, -1) is False
    assert "llama_kv_self_seq_cp" in llmi.last_error() and "ctx" in llmi.last_error()
