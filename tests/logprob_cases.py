"""Crafted inputs of the device log-probability tests (llmi.logprob_rows: k_logprob, k_sample,
k_logprob_pick in step order): the smallest rows at which the kernels can go wrong.
tests/test_logprob_inputs.py checks them on the CPU against the host definition,
llmi.sampling.token_logprobs; tests/test_gpu_logprobs.py runs them on the device.

A case is (name, logits [rows][V] f32, history [rows][n_hist] i32, params per row, uniforms
per row, n_top per row).  Rows longer than 1024 entries go through the radix select, shorter
ones are sorted whole.

The tolerance is derived, not measured.  Summing V non-negative doubles in any order has
relative error at most (V - 1) * 2^-53, so lse = m + log(S) moves by about that much absolutely
(log's derivative at S is 1 / S, and the error is relative to S); a log-probability has one
more subtraction.  64 ulps of slack cover exp and log on both sides (the device library's are
assumed, not measured):

    |dev - ref| <= (V + 64) * 2^-53 * max(1, |lse_ref|) + 2 * 2^-53 * |ref|

Ids and tokens have no tolerance; -inf is matched exactly."""
from __future__ import annotations

import numpy as np

from llmi.sampling import SamplingParams, sample_trace, token_logprobs

VS = (1, 2, 7, 11, 63, 64, 65, 255, 257, 777, 1025, 128256)
N_TOPS = (0, 1, 5, 20)
SCALES = (0.01, 3.0, 30.0, 300.0)
MAX_TOP = 20
EPS = 2.0 ** -53

GREEDY = SamplingParams(temperature=0.0)
PLAIN = dict(repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
FLAT = dict(top_p=1.0, min_p=0.0, **PLAIN)


def P(**kw) -> SamplingParams:
    return SamplingParams(**kw)


def tolerance(V: int, lse_ref: float, ref: float) -> float:
    return (V + 64) * EPS * max(1.0, abs(lse_ref)) + 2 * EPS * abs(ref)


def _rows(rng, rows, V, scale=3.0):
    return (rng.standard_normal((rows, V)) * scale).astype(np.float32)


def _no_hist(rows):
    return np.zeros((rows, 0), np.int32)


def shape_cases():
    """Every V with every n_top (n_top > V among them), a greedy and a sampled row of each."""
    out = []
    for V in VS:
        rng = np.random.default_rng(100 + V)
        n_top = list(N_TOPS) * 2
        params = [GREEDY] * 4 + [P(top_k=40)] * 4
        out.append((f"shape-V{V}", _rows(rng, 8, V), _no_hist(8), params, rng.random(8), n_top))
    return out


def row_count_cases():
    """1, 3 and 8 rows; rows that want nothing between rows that want output."""
    V = 777
    mix = [P(top_k=40), GREEDY, P(top_k=1), P(temperature=0.0, repeat_penalty=1.3, repeat_last_n=8),
           P(top_k=5, temperature=2.0, presence_penalty=0.5), P(top_k=256, top_p=0.5), P(temperature=0.0, top_k=7),
           P(top_k=64, min_p=0.3, frequency_penalty=0.2, repeat_last_n=3)]
    tops = [5, -1, 20, 0, -1, 1, -1, 20]
    out = []
    for rows in (1, 3, 8):
        rng = np.random.default_rng(200 + rows)
        hist = rng.integers(0, V, (rows, 12)).astype(np.int32)
        out.append((f"rows-{rows}", _rows(rng, rows, V), hist, mix[:rows], rng.random(rows), tops[:rows]))
    # the select's side of 1024 as well
    rng = np.random.default_rng(209)
    hist = rng.integers(0, 2000, (3, 12)).astype(np.int32)
    out.append(("rows-3-V2000", _rows(rng, 3, 2000), hist, mix[:3], rng.random(3), [-1, 20, -1]))
    return out


def tie_cases():
    out = []
    for V in (777, 2000, 128256):
        rng = np.random.default_rng(300 + V)
        # all logits equal: every logprob is -log V and the ids are 0 .. n-1
        eq = np.full((3, V), 1.5, np.float32)
        out.append((f"ties-all-equal-V{V}", eq, _no_hist(3), [GREEDY, GREEDY, P(top_k=40, temperature=1.0, **FLAT)],
                    [0.0, 0.0, 0.31], [20, 1, 5]))
        # a run of 100 equal logits at scattered ids straddling the n-th place (n = 5 and 20),
        # three distinct larger ones above it
        lg = _rows(rng, 2, V, 1.0)
        ids = rng.permutation(V)[:103]
        lg[:, ids[:3]] = 20.0 + np.arange(3, dtype=np.float32)
        lg[:, ids[3:]] = 12.0
        out.append((f"ties-straddle-V{V}", lg, _no_hist(2), [GREEDY, GREEDY], [0.0, 0.0], [5, 20]))
    return out


def range_cases():
    out = []
    for V in (257, 1500):
        rng = np.random.default_rng(400 + V)
        lg = _rows(rng, 4, V, 1.0) - 5000.0
        ids = rng.permutation(V)[:12]
        # gaps above 745 between candidates: exp underflows, x - lse stays finite
        lg[0, ids] = -800.0 * np.arange(12, dtype=np.float32)
        lg[1, ids] = -800.0 * np.arange(12, dtype=np.float32)
        lg[1, ids[1]] = -0.5
        # one finite entry, the rest -inf: its logprob is 0, the alternatives -inf in id order
        lg[2, :] = -np.inf
        lg[2, ids[0]] = 3.0
        # half the row -inf
        lg[3] = rng.standard_normal(V).astype(np.float32) * 3.0
        lg[3, rng.permutation(V)[:V // 2]] = -np.inf
        out.append((f"range-V{V}", lg, _no_hist(4), [GREEDY, P(top_k=16, temperature=1.0, **FLAT), GREEDY, P(top_k=40)],
                    [0.0, 0.7, 0.0, 0.4], [20, 20, 5, 20]))
    return out


def scale_cases():
    out = []
    for V in (777, 128256):
        rng = np.random.default_rng(500 + V)
        lg = np.stack([_rows(rng, 1, V, s)[0] for s in SCALES])
        out.append((f"scales-V{V}", lg, _no_hist(4), [GREEDY, P(top_k=40), GREEDY, P(top_k=256, temperature=100.0, **FLAT)],
                    rng.random(4), [20, 5, 20, 20]))
    return out


def penalty_cases():
    out = []
    for V in (257, 1500):
        rng = np.random.default_rng(600 + V)
        # a sampled row whose penalties move the chosen token's logit: ranks 1 .. 4 hold 10, 9,
        # 8, 7; the window is full of rank 4's token, a presence penalty of -1.5 lifts it to 8.5
        # (k_sample leaves 8.5 in the row, third in the cdf 0.35, 0.61, 0.82, 1) and the uniform
        # selects it.  Its logprob comes from 7.
        lg = _rows(rng, 2, V, 0.5)
        ids = rng.permutation(V)[:4]
        lg[:, ids] = np.array([10, 9, 8, 7], np.float32)
        hist = np.full((2, 4), ids[3], np.int32)
        p = P(top_k=4, temperature=3.0, repeat_last_n=4, presence_penalty=-1.5, top_p=1.0, min_p=0.0)
        out.append((f"pen-chosen-V{V}", lg, hist, [p, p], [0.7, 0.7], [5, 0]))
        # a penalized argmax row: the penalty dethrones the maximum, which stays alternative 0
        lg = _rows(rng, 2, V)
        top = int(np.argmax(lg[0]))
        lg[0, top] = abs(lg[0, top]) + 1.0
        lg[1] = lg[0]
        second = int(np.argsort(-lg[0])[1])
        # row 1: the window holds the runner-up, pushed down; the argmax is chosen unpenalized
        hist = np.stack([np.full(3, top), np.full(3, second)]).astype(np.int32)
        pa = P(temperature=0.0, repeat_last_n=3, repeat_penalty=50.0)
        out.append((f"pen-argmax-V{V}", lg, hist, [pa, pa], [0.0, 0.0], [5, 20]))
        # a long window with repeats, ids out of range, and the chain's own penalties
        lg = _rows(rng, 3, V)
        hist = rng.integers(0, V, (3, 256)).astype(np.int32)
        hist[:, -3:] = hist[:, -4:-3]
        hist[:, -5] = V + 7
        hist[:, -6] = -1
        pen = dict(repeat_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.25)
        out.append((f"pen-window-V{V}", lg, hist,
                    [P(top_k=40, repeat_last_n=256, **pen), P(temperature=0.0, repeat_last_n=64, **pen), GREEDY],
                    rng.random(3), [20, 5, 1]))
    return out


def all_cases():
    return shape_cases() + row_count_cases() + tie_cases() + range_cases() + scale_cases() + penalty_cases()


def reference(case):
    """Per row: (host token, lse, logprobs of the whole RAW row, top ids); the last three None
    for a row with n_top -1.  The token is the host sampler chain's."""
    _, lg, hist, params, us, n_top = case
    out = []
    for r, p in enumerate(params):
        h = [int(t) for t in hist[r]]
        tok = int(np.argmax(lg[r])) if p.greedy else sample_trace(p, lg[r], h, float(us[r]) if p.temperature > 0.0 else None).token
        if n_top[r] < 0:
            out.append((tok, None, None, None))
            continue
        lse, ids, lp = token_logprobs(lg[r], n_top[r])
        out.append((tok, lse, lp, [int(i) for i in ids]))
    return out
