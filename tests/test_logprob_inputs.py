"""The crafted rows of tests/logprob_cases.py against the host definition,
llmi.sampling.token_logprobs, on the CPU: the definition's own properties hold on every case,
and the condition under which the GPU tests' tolerance was derived holds, so no case is set
aside there."""
from __future__ import annotations

import math

import numpy as np
import pytest

import logprob_cases as LC
from llmi.sampling import token_logprobs

CASES = LC.all_cases()


def _rows(case):
    _, lg, _, _, _, n_top = case
    return [(r, lg[r], n_top[r]) for r in range(lg.shape[0])]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_definition_on_every_case(case):
    for r, row, n in _rows(case):
        assert not np.isnan(row).any() and np.isfinite(row.max()), f"row {r} is outside the definition"
        lse, ids, lp = token_logprobs(row, max(n, 0))
        V = row.size
        # exp(logprobs) over the whole row sums to 1
        assert abs(math.fsum(np.exp(lp)) - 1.0) <= (V + 64) * LC.EPS * 4, f"row {r}"
        # the ids are in lexsort order: logit descending, lower id first on ties
        order = np.lexsort((np.arange(V), -row.astype(np.float64)))
        assert list(ids) == list(order[:min(max(n, 0), V)]), f"row {r}"
        # x - lse, never log(p): finite wherever the logit is
        assert np.array_equal(np.isfinite(lp), np.isfinite(row)), f"row {r}"
        assert np.all(lp[np.isneginf(row)] == -np.inf)
        # the tolerance's condition: the definition's lse against an exactly rounded sum
        x = row.astype(np.float64)
        m = float(x.max())
        exact = m + math.log(math.fsum(math.exp(v - m) for v in x))
        err, tol = abs(lse - exact), LC.tolerance(V, exact, exact)
        assert err <= tol / 4, f"row {r}: |lse - fsum lse| {err:.3g} above a quarter of {tol:.3g}"


def test_reference_covers_every_row():
    """No case is set aside: every row has a reference, a row with n_top -1 a token only."""
    for case in CASES:
        ref = LC.reference(case)
        assert len(ref) == case[1].shape[0]
        for (tok, lse, lp, ids), n in zip(ref, case[5]):
            assert 0 <= tok < case[1].shape[1]
            assert (lse is None) == (n < 0)
            if n >= 0:
                assert len(ids) == min(n, case[1].shape[1]) and math.isfinite(lse)


def test_cases_cover_what_they_claim():
    by = dict((c[0], c) for c in CASES)
    for V in LC.VS:
        c = by[f"shape-V{V}"]
        assert sorted(set(c[5])) == list(LC.N_TOPS)
    assert any(n > c[1].shape[1] for c in CASES for n in c[5])
    assert {c[1].shape[0] for c in CASES} >= {1, 3, 8}
    assert any(-1 in c[5] and c[5][0] >= 0 and c[5][-1] >= 0 for c in CASES)
    for V in (777, 2000, 128256):
        # all equal: every logprob is -log V, the ids 0 .. n-1
        _, lse, lp, ids = LC.reference(by[f"ties-all-equal-V{V}"])[0]
        assert ids == list(range(20)) and np.allclose(lp, -math.log(V), rtol=0, atol=1e-12)
        # the straddling run resolves to its lowest ids
        c = by[f"ties-straddle-V{V}"]
        run = np.flatnonzero(c[1][1] == 12.0)
        assert LC.reference(c)[1][3][3:] == list(run[:17]) and LC.reference(c)[0][3][3:] == list(run[:2])
    for V in (257, 1500):
        c = by[f"range-V{V}"]
        ref = LC.reference(c)
        # gaps above 745: finite log-probabilities below -745
        assert all(math.isfinite(ref[0][2][i]) for i in ref[0][3]) and ref[0][2][ref[0][3][1]] < -745.0
        # one finite entry: logprob 0, the alternatives -inf in id order
        tok, lse, lp, ids = ref[2]
        assert lp[tok] == 0.0 and all(lp[i] == -np.inf for i in ids[1:]) and ids[1:] == sorted(ids[1:])
        assert np.isneginf(c[1][3]).sum() == V // 2
        # the penalty moves the chosen token's logit: the sampler picks the token whose raw
        # logit is 7 and whose penalized logit is 8.5
        c = by[f"pen-chosen-V{V}"]
        for r, (tok, lse, lp, ids) in enumerate(LC.reference(c)):
            assert tok == int(c[2][r, 0]) and c[1][r, tok] == 7.0
            assert abs(lp[tok] - (7.0 - lse)) == 0.0
        # the penalized argmax is not the raw argmax, which stays alternative 0
        c = by[f"pen-argmax-V{V}"]
        ref = LC.reference(c)
        assert ref[0][0] != int(np.argmax(c[1][0])) and ref[0][3][0] == int(np.argmax(c[1][0]))
        assert ref[1][0] == int(np.argmax(c[1][1]))
    c = by["scales-V777"]
    assert [round(float(np.std(c[1][r])) / s, 0) for r, s in enumerate(LC.SCALES)] == [1.0] * 4
    assert any(p.greedy for c in CASES for p in c[3])


def test_strided_partial_sums_stay_far_inside_the_bound():
    """The device sums one partial per thread (1024 of them) and then those: that order against
    the definition's, on the CPU, for every V and scale listed."""
    worst = 0.0
    for V in LC.VS:
        for s in LC.SCALES:
            row = (np.random.default_rng(V).standard_normal(V) * s).astype(np.float32)
            lse, _, _ = token_logprobs(row, 0)
            x = row.astype(np.float64)
            m = x.max()
            e = np.exp(x - m)
            parts = np.array([e[t::1024].sum() for t in range(min(1024, V))])
            strided = float(m + np.log(parts.sum()))
            worst = max(worst, abs(strided - lse) / LC.tolerance(V, lse, lse))
    print(f"strided 1024-partial sum against the definition: at most {worst:.3%} of the bound")
    assert worst < 0.02
