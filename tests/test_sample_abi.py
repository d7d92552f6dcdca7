"""The device sampler's C ABI without a GPU: llmi_sample_logits and
llmi_generate_sampled_batch refuse what the device path does not take before any device
work, each refusal naming its field; and the kernel-level cases of tests/sample_cases.py are
decided by the host reference with a margin of at least 1e-9, so the GPU tests set none
aside."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import llmi
import sample_cases as SC
from llmi._lib import SAMPLE_MAX_LAST_N, SAMPLE_MAX_TOP_K
from llmi.sampling import DEVICE_MAX_LAST_N, DEVICE_MAX_TOP_K, SamplingParams

OK = SamplingParams()
BAD = [
    (dict(top_k=0), "top_k"), (dict(top_k=-1), "top_k"), (dict(top_k=SAMPLE_MAX_TOP_K + 1), "top_k"),
    (dict(repeat_last_n=-1), "repeat_last_n"), (dict(repeat_last_n=SAMPLE_MAX_LAST_N + 1), "repeat_last_n"),
    (dict(temperature=float("nan")), "temperature"), (dict(temperature=float("inf")), "temperature"),
]


def test_limits_agree():
    assert (DEVICE_MAX_TOP_K, DEVICE_MAX_LAST_N) == (SAMPLE_MAX_TOP_K, SAMPLE_MAX_LAST_N)
    assert SAMPLE_MAX_TOP_K >= 256 and SAMPLE_MAX_LAST_N >= 256


def _hook(params, rows=None, V=16, nulls=()):
    rows = len(params) if rows is None else rows
    n = max(rows, 1)
    lg, un = np.zeros((n, V), np.float32), np.zeros(n)
    tok, cand, nc = np.zeros(n, np.int32), np.zeros((n, SAMPLE_MAX_TOP_K), np.int32), np.zeros(n, np.int32)
    vp = lambda name, a: None if name in nulls else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return llmi.lib().llmi_sample_logits(vp("logits", lg), rows, V, None, 0, None if "params" in nulls else llmi.sampler_params(params),
                                         vp("uniforms", un), vp("token_out", tok), vp("cand_out", cand), vp("n_cand_out", nc),
                                         None, None)


def _generate(params, seqs, n_gen=4, nulls=(), uniforms=True):
    k = len(seqs)
    arr = lambda name, v: None if name in nulls else (C.c_int32 * max(len(v), 1))(*v)  # noqa: E731
    un = None if "uniforms" in nulls else (C.c_double * max(k * n_gen, 1))()
    out = None if "out" in nulls else (C.c_int32 * max(k * n_gen, 1))()
    pa = None if "params" in nulls else llmi.sampler_params(params)
    return llmi.lib().llmi_generate_sampled_batch(None, k, arr("seqs", seqs), arr("first", [1] * k), arr("pos0", [0] * k), n_gen,
                                                  pa, un, out)


@pytest.mark.parametrize("kw,field", BAD, ids=[f"{list(kw)[0]}={list(kw.values())[0]}" for kw, _ in BAD])
def test_parameters_outside_the_device_limits_are_refused(kw, field):
    bad = SamplingParams(**kw)
    assert _hook([OK, bad]) == -1
    assert field in llmi.last_error() and "params[1]" in llmi.last_error()
    assert _generate([OK, OK, bad], [0, 1, 2]) == -1
    assert field in llmi.last_error() and "params[2]" in llmi.last_error()


@pytest.mark.parametrize("n", [0, 9])
def test_row_and_sequence_counts_are_refused(n):
    assert _hook([OK] * n, rows=n) == -1 and "n_rows" in llmi.last_error()
    assert _generate([OK] * n, list(range(n))) == -1 and "1..8" in llmi.last_error()


def test_repeated_sequences_are_refused():
    assert _generate([OK] * 3, [0, 2, 0]) == -1 and "repeated sequence" in llmi.last_error()


def test_null_pointers_are_refused():
    for name in ("logits", "params", "uniforms", "token_out", "cand_out", "n_cand_out"):
        assert _hook([OK], nulls=(name,)) == -1 and "null" in llmi.last_error(), name
    for name in ("seqs", "first", "pos0", "params", "uniforms", "out"):
        assert _generate([OK], [0], nulls=(name,)) == -1 and "null" in llmi.last_error(), name
    # everything else in order: the context is what is missing
    assert _generate([OK], [0]) == -1 and "context" in llmi.last_error()
    # a history length without a history
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lg, un, i32 = np.zeros((1, 4), np.float32), np.zeros(1), np.zeros(SAMPLE_MAX_TOP_K, np.int32)
    assert llmi.lib().llmi_sample_logits(p(lg), 1, 4, None, 3, llmi.sampler_params([OK]), p(un), p(i32), p(i32), p(i32), None,
                                         None) == -1 and "null" in llmi.last_error()


CASES = SC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_no_kernel_case_needs_setting_aside(case):
    """The comparison rule lets a case be set aside only when the reference's own decision
    margin is below 1e-9; the seeds are chosen so that none is."""
    for r, (tok, cand, margin, _) in enumerate(SC.reference(case)):
        assert margin >= SC.MARGIN, f"row {r}: margin {margin:.3g}"
        assert 0 <= tok < case[1].shape[1]


def test_cases_cover_what_they_claim():
    names = [c[0] for c in CASES]
    for V in SC.VS:
        assert f"shape-V{V}" in names
    by = dict((c[0], c) for c in CASES)
    # the straddling run resolves to its 30 lowest ids
    for V in (777, 2000, 128256):
        _, lg, _, _, _ = by[f"ties-straddle-V{V}"]
        cand = SC.reference(by[f"ties-straddle-V{V}"])[0][1]
        run = np.flatnonzero(lg[0] == 12.0)
        assert len(cand) == 40 and sorted(cand[10:]) == list(run[:30])
        assert len(SC.reference(by[f"ties-max-minp1-V{V}"])[0][1]) == 5
        assert SC.reference(by[f"ties-all-equal-V{V}"])[1][1] == tuple(range(256))
    # the penalty moves a token out of and into the top 4
    for V in (257, 1500):
        c = by[f"pen-cross-k-V{V}"]
        ref = SC.reference(c)
        assert int(c[2][0, 0]) not in ref[0][1] and int(c[2][1, 0]) in ref[1][1]
        # and dethrones the maximum
        c = by[f"pen-argmax-V{V}"]
        assert SC.reference(c)[0][0] != int(np.argmax(c[1][0]))
    # the uniforms pick the first, a middle and the last candidate
    ref = SC.reference(by["uniforms"])
    picks = [r[1].index(r[0]) for r in ref]
    assert picks == [0, 15, 0, 7, 15]
    # flat cdf runs: the tail underflows to probability 0
    assert SC.final_cdf(by["range-V257"][3][0], by["range-V257"][1][0], [], 0.5)[0] == 1.0
