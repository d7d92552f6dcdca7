"""k_sample alone (llmi.sample_logits, no model) against the host definition,
llmi.sampling.sample_with_uniform, on the crafted rows of tests/sample_cases.py.

Comparison rule: tokens and final candidate ids are compared exactly, penalized values bit
for bit.  A case could be set aside only if the reference's own decision margin were below
1e-9 (at most 256 FP64 terms of about 1e-16 each accumulate about 1e-13; four orders of
slack); the cases are seeded so that none is, which every test asserts."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
import sample_cases as SC

pytestmark = pytest.mark.gpu

CASES = SC.all_cases()


def _run(case):
    _, lg, hist, params, us = case
    return llmi.sample_logits(lg, hist, params, us)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_host_definition(gpu, case):
    name, lg, hist, params, us = case
    toks, cands, pen, usec = _run(case)
    V = lg.shape[1]
    for r, (tok, cand, margin, row) in enumerate(SC.reference(case)):
        assert margin >= SC.MARGIN, f"{name} row {r}: reference margin {margin:.3g}: the case must be reseeded"
        print(f"{name} row {r}: token {toks[r]} (host {tok}), {len(cands[r])} candidates (host {len(cand)}), margin {margin:.3g}")
        assert tuple(cands[r]) == tuple(cand), f"{name} row {r}: candidates"
        assert toks[r] == tok, f"{name} row {r}: token"
        for j, t in enumerate(hist[r]):
            want = row[t] if 0 <= t < V else np.float32(0)
            assert pen[r, j].view(np.uint32) == np.float32(want).view(np.uint32), f"{name} row {r}: penalized value of token {t}"
    assert usec >= 0.0


def test_greedy_rows_keep_the_plain_argmax(gpu):
    """A record that says greedy leaves the row's argmax keys alone, whatever its neighbours do."""
    case = dict((c[0], c) for c in CASES)["rows-8"]
    toks, cands, _, _ = _run(case)
    for r, p in enumerate(case[3]):
        if p.greedy:
            assert toks[r] == int(np.argmax(case[1][r])) and cands[r] == []


def test_same_inputs_same_outputs(gpu):
    for name in ("rows-8", "shape-V128256", "pen-h100-w16-V1500"):
        case = dict((c[0], c) for c in CASES)[name]
        a, b = _run(case), _run(case)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
