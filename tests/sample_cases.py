"""Crafted inputs of the device sampler's kernel-level tests (llmi.sample_logits, k_sample):
the smallest rows at which the kernel can go wrong.  tests/test_sample_abi.py checks on the
CPU that the host reference decides every one of them with a margin of at least 1e-9 (so none
is set aside); tests/test_gpu_sample.py runs them on the device.

A case is (name, logits [rows][V] f32, history [rows][n_hist] i32, params per row, uniforms
per row).  Rows longer than 1024 entries go through the kernel's radix select, shorter ones
are sorted whole, so ties and penalties appear on both sides of that size.
"""
from __future__ import annotations

import numpy as np

from llmi.sampling import SamplingParams, _softmax, sample_trace

MARGIN = 1e-9  # the reference's own decision margin below which a case may be set aside
VS = (1, 2, 63, 64, 65, 255, 257, 777, 1025, 128256)
TOP_KS = (1, 2, 40, 64, 65, 256)
BELOW_ONE = float(np.nextafter(1.0, 0.0))

PLAIN = dict(repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
FLAT = dict(top_p=1.0, min_p=0.0, **PLAIN)  # every top_k candidate survives to the draw


def P(**kw) -> SamplingParams:
    return SamplingParams(**kw)


def _rows(rng, rows, V, scale=3.0):
    return (rng.standard_normal((rows, V)) * scale).astype(np.float32)


def final_cdf(p, logits, hist, u):
    """The normalised cdf over the final candidates (what the draw is searched in)."""
    tr = sample_trace(p, logits, hist, u)
    from llmi.sampling import penalized_logits

    x = penalized_logits(p, logits, hist)[list(tr.candidates)].astype(np.float64)
    cdf = np.cumsum(_softmax(x / p.temperature))
    return cdf / cdf[-1]


def shape_cases():
    """V x top_k (k > V included): one call per V, a row per top_k plus two rows whose 256
    candidates all reach the draw at temperature 1e-3 and 100."""
    out = []
    for V in VS + (7, 11):  # (rows of 4 .. 11 entries off a 16-byte boundary: all head and tail, no whole quad)
        rng = np.random.default_rng(1000 + V)
        params = [P(top_k=k) for k in TOP_KS] + [P(top_k=256, temperature=1e-3, **FLAT), P(top_k=256, temperature=100.0, **FLAT)]
        out.append((f"shape-V{V}", _rows(rng, 8, V), np.zeros((8, 0), np.int32), params, rng.random(8)))
    return out


def row_count_cases():
    """1, 3 and 8 rows, every row its own parameters, greedy rows among them."""
    V = 777
    mix = [P(top_k=40), P(temperature=0.0), P(top_k=1), P(temperature=0.0, repeat_penalty=1.3, repeat_last_n=8),
           P(top_k=5, temperature=2.0, presence_penalty=0.5), P(top_k=256, top_p=0.5), P(temperature=0.0, top_k=7),
           P(top_k=64, min_p=0.3, frequency_penalty=0.2, repeat_last_n=3)]
    out = []
    for rows in (1, 3, 8):
        rng = np.random.default_rng(2000 + rows)
        hist = rng.integers(0, V, (rows, 12)).astype(np.int32)
        # (a single row takes the chain, so that the one-slot launch runs it)
        out.append((f"rows-{rows}", _rows(rng, rows, V), hist, mix[:rows], rng.random(rows)))
    return out


def tie_cases():
    out = []
    for V in (777, 2000, 128256):
        rng = np.random.default_rng(3000 + V)
        # all logits equal: the candidates are ids 0 .. k-1
        eq = np.full((2, V), 1.5, np.float32)
        out.append((f"ties-all-equal-V{V}", eq, np.zeros((2, 0), np.int32),
                    [P(top_k=40, temperature=1.0, **FLAT), P(top_k=256, temperature=1.0, **FLAT)], [0.31, 0.905]))
        # ten distinct large logits, then a run of 100 equal ones at scattered ids across the
        # k-th place (k = 40): the 30 lowest ids of the run are in
        lg = _rows(rng, 1, V, 1.0)
        ids = rng.permutation(V)[:110]
        lg[0, ids[:10]] = 20.0 + np.arange(10, dtype=np.float32)
        lg[0, ids[10:]] = 12.0
        out.append((f"ties-straddle-V{V}", lg, np.zeros((1, 0), np.int32), [P(top_k=40, temperature=4.0, **FLAT)], [0.77]))
        # five tied at the maximum under min_p = 1: exactly those five, in id order
        lg = _rows(rng, 1, V, 1.0)
        lg[0, rng.permutation(V)[:5]] = 9.0
        out.append((f"ties-max-minp1-V{V}", lg, np.zeros((1, 0), np.int32), [P(top_k=40, top_p=1.0, min_p=1.0, **PLAIN)], [0.5]))
    return out


def range_cases():
    out = []
    for V in (257, 1500):
        rng = np.random.default_rng(4000 + V)
        # gaps above 745: the tail's probabilities underflow to 0, the cdf is flat
        lg = _rows(rng, 4, V, 1.0) - 5000.0
        ids = rng.permutation(V)[:12]
        lg[:, ids] = -800.0 * np.arange(12, dtype=np.float32)
        lg[1, ids[1]] = -0.5  # two live candidates, then the flat run
        lg[3, ids] = -np.inf  # -inf entries; the rest of the row finite
        lg[3, ids[0]] = 3.0
        lg[2, rng.permutation(V)[:V // 2]] = -np.inf
        params = [P(top_k=16, temperature=1.0, **FLAT), P(top_k=16, temperature=1.0, **FLAT),
                  P(top_k=40, temperature=1e-3), P(top_k=256, temperature=100.0, **FLAT)]
        out.append((f"range-V{V}", lg, np.zeros((4, 0), np.int32), params, [0.5, 0.7, 0.2, 0.999]))
    return out


def uniform_cases():
    """u = 0, the largest double below 1, and just above cdf[i] (by 1e-6) so that the first,
    a middle and the last candidate are chosen."""
    V = 257
    rng = np.random.default_rng(5000)
    p = P(top_k=16, temperature=5.0, **FLAT)
    lg = np.repeat(_rows(rng, 1, V), 5, axis=0)
    hist = np.zeros((5, 0), np.int32)
    cdf = final_cdf(p, lg[0], [], 0.5)
    us = [0.0, BELOW_ONE, 1e-6, float(cdf[6] + 1e-6), float(cdf[-2] + 1e-6)]
    return [("uniforms", lg, hist, [p] * 5, us)]


def top_p_min_p_cases():
    V = 777
    rng = np.random.default_rng(6000)
    combos = [(tp, mp) for tp in (0.0, 0.5, 0.95, 1.0) for mp in (0.0, 0.05, 1.0)]
    out = []
    for i in range(0, 12, 6):
        params = [P(top_k=40, top_p=tp, min_p=mp, temperature=1.5, **PLAIN) for tp, mp in combos[i:i + 6]]
        out.append((f"top_p-min_p-{i // 6}", _rows(rng, 6, V, 1.5), np.zeros((6, 0), np.int32), params, rng.random(6)))
    return out


def penalty_cases():
    out = []
    for V in (257, 1500):
        rng = np.random.default_rng(7000 + V)
        # history empty: a penalized chain with nothing to penalize
        pen = dict(repeat_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.25)
        out.append((f"pen-empty-V{V}", _rows(rng, 2, V), np.zeros((2, 0), np.int32),
                    [P(top_k=40, repeat_last_n=64, **pen), P(temperature=0.0, repeat_last_n=64, **pen)], [0.4, 0.0]))
        # history shorter (10 < 64) and longer (100 > 16) than the window: repeated tokens,
        # ids >= V and < 0, logits <= 0 and > 0 among them
        for n_hist, last_n in ((10, 64), (100, 16), (256, 256), (300, 0)):
            lg = _rows(rng, 3, V)
            hist = rng.integers(0, V, (3, n_hist)).astype(np.int32)
            hist[:, -3:] = hist[:, -4:-3]            # a token four times at the window's end
            hist[:, -5] = V + 7                      # out of range
            hist[:, -6] = -1
            hist[0, -7], hist[0, -8] = int(np.argmax(lg[0])), int(np.argmin(lg[0]))  # a logit > 0 and one <= 0
            lg[1, hist[1, -1]] = 0.0
            params = [P(top_k=40, repeat_last_n=last_n, **pen),
                      P(top_k=256, temperature=1.2, repeat_last_n=last_n, repeat_penalty=0.8, presence_penalty=-1.0,
                        frequency_penalty=-0.5, top_p=1.0, min_p=0.0),
                      P(temperature=0.0, repeat_last_n=last_n, **pen)]
            out.append((f"pen-h{n_hist}-w{last_n}-V{V}", lg, hist, params, rng.random(3)))
        # a token the penalty moves across the k-th place (k = 4), in each direction: ranks
        # 1 .. 6 hold 10, 9, 8, 7, 6, 5; row 0 divides rank 4's 7 to 3.5 (out, rank 5 in), row 1's
        # negative presence penalty lifts rank 5's 6 to 8 (in, rank 4 out)
        lg = _rows(rng, 2, V, 0.5)
        ids = rng.permutation(V)[:6]
        lg[:, ids] = np.array([10, 9, 8, 7, 6, 5], np.float32)
        hist = np.stack([np.full(4, ids[3]), np.full(4, ids[4])]).astype(np.int32)
        params = [P(top_k=4, temperature=3.0, repeat_last_n=4, repeat_penalty=2.0, top_p=1.0, min_p=0.0),
                  P(top_k=4, temperature=3.0, repeat_last_n=4, presence_penalty=-2.0, top_p=1.0, min_p=0.0)]
        out.append((f"pen-cross-k-V{V}", lg, hist, params, [0.9, 0.9]))
        # temperature <= 0 with penalties: the penalty dethrones the maximum
        lg = _rows(rng, 1, V)
        top = int(np.argmax(lg[0]))
        lg[0, top] = abs(lg[0, top]) + 1.0
        out.append((f"pen-argmax-V{V}", lg, np.full((1, 3), top, np.int32),
                    [P(temperature=0.0, repeat_last_n=3, repeat_penalty=50.0)], [0.0]))
    return out


def all_cases():
    return (shape_cases() + row_count_cases() + tie_cases() + range_cases() + uniform_cases() + top_p_min_p_cases() +
            penalty_cases())


def reference(case):
    """Per row: (token, candidate ids or () for a greedy row, margin, penalized row)."""
    from llmi.sampling import penalized_logits

    _, lg, hist, params, us = case
    out = []
    for r, p in enumerate(params):
        h = [int(t) for t in hist[r]]
        if p.greedy:
            out.append((int(np.argmax(lg[r])), (), float("inf"), lg[r]))
            continue
        tr = sample_trace(p, lg[r], h, float(us[r]) if p.temperature > 0.0 else None)
        out.append((tr.token, tr.candidates, tr.margin, penalized_logits(p, lg[r], h)))
    return out
