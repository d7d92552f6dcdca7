"""The log-probability C ABI without a GPU: the exports exist, LLMI_LOGPROBS_MAX_TOP is 20 in
the header and the binding, and llmi_generate_logprobs_batch / llmi_logprob_rows refuse bad
arguments with -1 before any device work, each refusal naming its field."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import llmi
from llmi._lib import LOGPROBS_MAX_TOP, SIGNATURES
from llmi.sampling import SamplingParams

OK = SamplingParams()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "llmi.h")
FIELDS = ("seqs", "first", "pos0", "params", "uniforms", "n_top", "out", "tok_logprob", "top_id", "top_logprob")


def test_exports_and_limit():
    L = llmi.lib()
    for name in ("llmi_generate_logprobs_batch", "llmi_logprob_rows"):
        assert name in SIGNATURES and getattr(L, name) is not None
    assert LOGPROBS_MAX_TOP == 20
    text = open(HEADER).read()
    assert re.search(r"#define\s+LLMI_LOGPROBS_MAX_TOP\s+20\b", text)
    assert "llmi_generate_logprobs_batch(" in text and "llmi_logprob_rows(" in text
    assert hasattr(llmi.Context, "generate_logprobs_batch") and callable(llmi.logprob_rows)


def _generate(n_top, seqs, n_gen=4, nulls=(), params=None):
    k = len(seqs)
    T = LOGPROBS_MAX_TOP
    arr = lambda name, v: None if name in nulls else (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    dbl = lambda name, n: None if name in nulls else (C.c_double * max(n, 1))()  # noqa: E731
    i32 = lambda name, n: None if name in nulls else (C.c_int32 * max(n, 1))()  # noqa: E731
    pa = None if "params" in nulls else llmi.sampler_params(params or [OK] * k)
    return llmi.lib().llmi_generate_logprobs_batch(
        None, k, arr("seqs", seqs), arr("first", [1] * k), arr("pos0", [0] * k), n_gen, pa, dbl("uniforms", k * n_gen),
        arr("n_top", n_top), i32("out", k * n_gen), dbl("tok_logprob", k * n_gen), i32("top_id", k * n_gen * T),
        dbl("top_logprob", k * n_gen * T))


def _hook(n_top, nulls=(), V=16):
    n, m = len(n_top), max(len(n_top), 1)
    T = LOGPROBS_MAX_TOP
    bufs = dict(logits=np.zeros((m, V), np.float32), uniforms=np.zeros(m), n_top=np.asarray(list(n_top) or [0], np.int32),
                token_out=np.zeros(m, np.int32), tok_logprob_out=np.zeros(m), lse_out=np.zeros(m),
                top_id_out=np.zeros((m, T), np.int32), top_logprob_out=np.zeros((m, T)))
    p = lambda name: None if name in nulls else bufs[name].ctypes.data_as(C.c_void_p)  # noqa: E731
    return llmi.lib().llmi_logprob_rows(p("logits"), n, V, None, 0, None if "params" in nulls else llmi.sampler_params([OK] * m),
                                        p("uniforms"), p("n_top"), p("token_out"), p("tok_logprob_out"), p("lse_out"),
                                        p("top_id_out"), p("top_logprob_out"), None, None)


@pytest.mark.parametrize("bad", [-2, 21])
def test_n_top_outside_the_limits_is_refused(bad):
    assert _generate([0, bad, 5], [0, 1, 2]) == -1
    assert "n_top[1]" in llmi.last_error() and str(bad) in llmi.last_error()
    assert _hook([20, -1, bad]) == -1 and "n_top[2]" in llmi.last_error()


def test_limits_themselves_are_taken():
    """-1, 0 and 20 pass the argument checks: what is missing then is the context."""
    assert _generate([-1, 0, 20], [0, 1, 2]) == -1 and "ctx" in llmi.last_error()


def test_null_pointers_are_refused_by_name():
    for name in FIELDS:
        assert _generate([5], [0], nulls=(name,)) == -1, name
        assert name in llmi.last_error() and "null" in llmi.last_error(), (name, llmi.last_error())
    for name in ("logits", "params", "uniforms", "n_top", "token_out", "tok_logprob_out", "lse_out", "top_id_out",
                 "top_logprob_out"):
        assert _hook([5], nulls=(name,)) == -1 and "null" in llmi.last_error(), name


def test_repeated_sequences_and_counts_are_refused():
    assert _generate([5, 5, 5], [0, 2, 0]) == -1 and "seqs" in llmi.last_error() and "repeated sequence" in llmi.last_error()
    for n in (0, 9):
        assert _generate([5] * n, list(range(n))) == -1 and "1..8" in llmi.last_error()
    assert _hook([]) == -1 and "n_rows" in llmi.last_error()


def test_sampler_limits_are_refused_as_in_the_sampled_call():
    assert _generate([5, 5], [0, 1], params=[OK, SamplingParams(top_k=0)]) == -1
    assert "params[1]" in llmi.last_error() and "top_k" in llmi.last_error()
