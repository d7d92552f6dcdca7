"""k_logprob, k_sample and k_logprob_pick in step order (llmi.logprob_rows, no model) against the
host definition, llmi.sampling.token_logprobs, on the crafted rows of tests/logprob_cases.py.

Comparison rule: the token equals k_sample's alone on the same inputs (llmi.sample_logits);
the alternatives' ids equal the reference's exactly; lse, the token's log-probability and
the alternatives' are within the derived tolerance of logprob_cases (-inf exactly); and the
row read back is what k_sample alone leaves, bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
import logprob_cases as LC
from llmi.sampling import token_logprobs

pytestmark = pytest.mark.gpu

CASES = LC.all_cases()
T = LC.MAX_TOP


def _close(dev, ref, V, lse_ref, what):
    if np.isneginf(ref):
        assert np.isneginf(dev), f"{what}: {dev} where the reference has -inf"
        return 0.0
    err, tol = abs(float(dev) - float(ref)), LC.tolerance(V, lse_ref, ref)
    assert err <= tol, f"{what}: |{dev!r} - {ref!r}| = {err:.3g} above {tol:.3g}"
    return err / tol


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernels_equal_host_definition(gpu, case):
    name, lg, hist, params, us, n_top = case
    V = lg.shape[1]
    got = llmi.logprob_rows(lg, hist, params, us, n_top)
    toks, _, pen, _ = llmi.sample_logits(lg, hist, params, us)
    assert got["tokens"] == toks, f"{name}: tokens differ from k_sample alone"
    worst = 0.0
    for r in range(lg.shape[0]):
        # the row after the three kernels: the input, but for k_sample's penalized entries
        want = lg[r].copy()
        for j, t in enumerate(hist[r]):
            if 0 <= t < V:
                want[t] = pen[r, j]
        assert np.array_equal(got["rows"][r].view(np.uint32), want.view(np.uint32)), f"{name} row {r}: the row changed"
        if n_top[r] < 0:  # the kernels returned at once: the caller's values stand
            assert np.isnan(got["lse"][r]) and np.isnan(got["tok_logprob"][r])
            assert np.all(got["top_ids"][r] == -2) and np.all(np.isnan(got["top_logprobs"][r]))
            continue
        lse, ids, lp = token_logprobs(lg[r], n_top[r])
        worst = max(worst, _close(got["lse"][r], lse, V, lse, f"{name} row {r} lse"))
        worst = max(worst, _close(got["tok_logprob"][r], lp[toks[r]], V, lse, f"{name} row {r} token {toks[r]}"))
        n = len(ids)
        assert list(got["top_ids"][r, :n]) == [int(i) for i in ids], f"{name} row {r}: alternatives"
        assert np.all(got["top_ids"][r, n:] == -1) and np.all(np.isneginf(got["top_logprobs"][r, n:])), f"{name} row {r}: unused entries"
        for i, t in enumerate(ids):
            worst = max(worst, _close(got["top_logprobs"][r, i], lp[t], V, lse, f"{name} row {r} alternative {i}"))
    print(f"{name}: worst error {worst:.3%} of the tolerance; k_logprob {got['usec'][0]:.1f} us, k_sample "
          f"{got['usec'][1]:.1f} us, k_logprob_pick {got['usec'][2]:.1f} us")


def test_penalized_token_reports_its_raw_logit(gpu):
    """The sampler leaves 8.5 where the raw row has 7: the reported value is 7 - lse."""
    by = dict((c[0], c) for c in CASES)
    for V in (257, 1500):
        name, lg, hist, params, us, n_top = by[f"pen-chosen-V{V}"]
        got = llmi.logprob_rows(lg, hist, params, us, n_top)
        for r in range(2):
            tok = got["tokens"][r]
            assert tok == int(hist[r, 0]) and got["rows"][r, tok] == np.float32(8.5) and lg[r, tok] == np.float32(7.0)
            lse, _, lp = token_logprobs(lg[r], 0)
            _close(got["tok_logprob"][r], 7.0 - lse, V, lse, f"{name} row {r}")
            assert abs(got["tok_logprob"][r] - (8.5 - lse)) > 1.0


def test_same_inputs_same_outputs(gpu):
    for name in ("rows-8", "shape-V128256", "pen-window-V1500"):
        _, lg, hist, params, us, n_top = dict((c[0], c) for c in CASES)[name]
        a, b = llmi.logprob_rows(lg, hist, params, us, n_top), llmi.logprob_rows(lg, hist, params, us, n_top)
        assert a["tokens"] == b["tokens"] and np.array_equal(a["top_ids"], b["top_ids"])
        # (the FP64 sum's order is fixed by the launch: the same bits)
        for k in ("lse", "tok_logprob", "top_logprobs"):
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
