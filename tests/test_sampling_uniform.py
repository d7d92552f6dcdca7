"""sample_with_uniform is Sampler.sample with its one random draw made explicit: numpy's
Generator.choice(n, p=pr) draws a single random() double and searches it (side='right') in
cumsum(pr) / cumsum(pr)[-1].  Feeding sample_with_uniform from a second generator with the
same seed must therefore reproduce Sampler.sample token for token; the uniform is the whole
interface between a request's generator and the device sampler."""
from __future__ import annotations

import numpy as np
import pytest

from llmi.sampling import Sampler, SamplingParams, device_eligible, sample_trace, sample_with_uniform

SETS = [
    SamplingParams(seed=11),  # the server's defaults
    SamplingParams(seed=12, temperature=1.3, top_k=256, top_p=1.0, min_p=0.0),
    SamplingParams(seed=13, temperature=0.7, top_k=5, top_p=0.5, min_p=0.2, repeat_penalty=1.2, repeat_last_n=16),
    SamplingParams(seed=14, temperature=2.0, top_k=64, presence_penalty=0.6, frequency_penalty=0.3, repeat_last_n=8),
    SamplingParams(seed=15, temperature=1.0, top_k=0, top_p=0.9, min_p=0.01, repeat_penalty=1.1, repeat_last_n=-1),
    SamplingParams(seed=16, temperature=0.0, repeat_penalty=1.5, presence_penalty=1.0, repeat_last_n=32),  # draws nothing
]


def _logits(rng, V):
    lg = (rng.standard_normal(V) * 2.5).astype(np.float32)
    lg[rng.permutation(V)[:min(3, V)]] = lg.max()  # ties at the maximum
    return lg


@pytest.mark.parametrize("V", [129, 777, 1000, 128256])
@pytest.mark.parametrize("p", SETS, ids=lambda p: f"seed{p.seed}")
def test_sampler_equals_uniform_restatement(p, V):
    s, rng2 = Sampler(p), np.random.default_rng(p.seed)
    data = np.random.default_rng(100 * p.seed + V % 97)
    hist = [int(t) for t in data.integers(0, V, 5)]
    for _ in range(64):
        lg = _logits(data, V)
        u = rng2.random() if p.temperature > 0.0 else None
        want = s.sample(lg, hist)
        assert sample_with_uniform(p, lg, hist, u) == want
        hist.append(want)
    # both generators consumed the same number of draws (none when temperature <= 0)
    assert s.rng.random() == rng2.random()


def test_chunk_of_uniforms_is_the_single_draws():
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    assert list(a.random(8)) == [b.random() for _ in range(8)]


def test_trace_candidates_and_margins():
    p = SamplingParams(temperature=1.0, top_k=4, top_p=0.9, min_p=0.1)
    lg = np.log(np.array([0.05, 0.4, 0.3, 0.2, 0.05], np.float64)).astype(np.float32)
    tr = sample_trace(p, lg, [], 0.45)
    # top_k 4: ids 1, 2, 3 and the lower id of the tied 0 / 4; probabilities .421 .316 .211 .053:
    # top_p .9 is first reached by the third, min_p keeps all three
    assert tr.candidates == (1, 2, 3) and tr.token == 2
    assert tr.margin_top_p == pytest.approx(abs(0.4 / 0.95 + 0.3 / 0.95 + 0.2 / 0.95 - 0.9), abs=1e-6)
    assert tr.margin_min_p == pytest.approx(0.2 / 0.9 - 0.1 * 0.4 / 0.9, abs=1e-6)
    assert tr.margin_dist == pytest.approx(0.45 - 0.4 / 0.9, abs=1e-6)
    assert tr.margin == tr.margin_dist


def test_ties_across_the_kth_place_take_the_lower_ids():
    lg = np.zeros(50, np.float32)
    lg[[40, 7]] = 3.0
    tr = sample_trace(SamplingParams(temperature=1.0, top_k=6, top_p=1.0, min_p=0.0), lg, [], 0.99)
    assert tr.candidates == (7, 40, 0, 1, 2, 3)


def test_device_eligibility():
    assert device_eligible(SamplingParams())
    assert device_eligible(SamplingParams(top_k=256, repeat_last_n=256))
    for bad in (dict(top_k=0), dict(top_k=-1), dict(top_k=257), dict(repeat_last_n=-1), dict(repeat_last_n=257),
                dict(temperature=float("nan"))):
        assert not device_eligible(SamplingParams(**bad)), bad
