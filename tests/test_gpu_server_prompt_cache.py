"""The prompt cache over the real HIP path: the second turn of an exchange, served from the
rows its slot still holds, gives the tokens of a server that prefills everything
(LLMI_CACHE_PROMPT=0), reports the reused positions and sends only the suffix through the
prefill; and a request that shares a prefix with one still decoding gets that prefix by the
device copy (llama_kv_self_seq_cp) and equals its solo result, as does the donor."""
from __future__ import annotations

import numpy as np
import pytest

from llmi.sampling import SamplingParams
from llmi.server import Engine

pytestmark = pytest.mark.gpu

A = SamplingParams(seed=11, temperature=1.0)
B = SamplingParams(seed=12, temperature=1.3, top_k=100, top_p=0.9, min_p=0.01, repeat_penalty=1.2, repeat_last_n=32,
                   frequency_penalty=0.2)
N = 12


def _engine(path):
    eng = Engine(path, 256, 99, [0], slots=4, chunk=8, cache_prompt=True)
    eng.load()
    assert eng.ready, eng.error
    return eng


def _toks(rng, n):
    return [int(t) for t in rng.integers(3, 700, n)]


@pytest.fixture(scope="module")
def cold(gpu, tiny_models):
    """A server without the cache: the baseline every cached result must equal."""
    mp = pytest.MonkeyPatch()
    mp.setenv("LLMI_CACHE_PROMPT", "0")
    try:
        eng = _engine(tiny_models["tiny-mixed-d128"])
    finally:
        mp.undo()
    assert not eng.replicas[0].cache_prompt and not eng.prompt_cache

    def run(prompt, n, p):
        return eng.generate(prompt, n, True, lambda t: None, sampling=p)[0]

    return run


@pytest.mark.parametrize("p", [None, A, B], ids=["greedy", "sampled", "sampled-penalties"])
def test_second_turn_is_served_from_the_cache(gpu, tiny_models, cold, p):
    rng = np.random.default_rng(3)
    eng = _engine(tiny_models["tiny-mixed-d128"])
    rep = eng.replicas[0]
    assert rep.cache_prompt and eng.prompt_cache
    quiet = lambda t, e: None  # noqa: E731
    p1 = [1] + _toks(rng, 29)
    r1 = eng.run(p1, N, True, quiet, sampling=p)
    assert r1.cached == 0 and r1.out == cold(p1, N, p)
    p2 = p1 + r1.out + _toks(rng, 5)
    before = rep.ctx.prefill_tokens
    r2 = eng.run(p2, N, True, quiet, sampling=p)
    n = len(p1) + N - 1  # all the first turn fed: its last token was sampled, not decoded
    assert r2.cached == n and r2.seq == r1.seq
    assert r2.out == cold(p2, N, p)
    # the suffix alone went through the prefill (its last token is a decode step)
    assert rep.ctx.prefill_tokens - before == len(p2) - n - 1
    h = eng.health()["replicas"][0]
    assert h["prompt_tokens"] == len(p1) + len(p2) and h["cached_tokens"] == n


def test_a_prefix_of_a_running_request_is_copied(gpu, tiny_models, cold):
    rng = np.random.default_rng(4)
    eng = _engine(tiny_models["tiny-mixed-d128"])
    ctx = eng.replicas[0].ctx
    inner, copies = ctx.seq_cp, []

    def counted(src, dst, p0=0, p1=-1):
        copies.append((src, dst, p0, p1))
        return inner(src, dst, p0, p1)

    ctx.seq_cp = counted
    shared = [1] + _toks(rng, 39)
    pa, pb = shared + _toks(rng, 5), shared + _toks(rng, 7)
    ra = eng.submit(pa, 200, True, None, None)
    first = ra.q.get(timeout=120)           # admitted and decoding
    rb = eng.submit(pb, N, True, B, None)   # its penalty window reads the copied history
    got_b = []
    while (t := rb.q.get(timeout=120)) is not None:
        got_b += t
    assert ra.finish is None, "the donor was to be still running"
    got_a = list(first)
    while (t := ra.q.get(timeout=120)) is not None:
        got_a += t
    assert ra.error is None and rb.error is None, (ra.error, rb.error)
    assert copies == [(ra.seq, rb.seq, 0, 40)] and rb.cached == 40 and rb.seq != ra.seq
    assert got_b == cold(pb, N, B)
    assert got_a == cold(pa, 200, None)
