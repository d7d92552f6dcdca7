"""The context's device memory over its life (csrc/dev_mem.h DevPool, engine.h GraphCache):
blocks that grow on demand, the step graphs cached per tail, and teardown.

Contexts of n_ctx 256 and n_seq 3, so the dummy sequence of a batched step exists.  The
single-sequence cases run on tiny-mixed and on tiny-mixed-d128; the two-sequence cases on
tiny-mixed-d128 alone: tiny-mixed's first layer has ffn_gate and ffn_up of different types,
so it has no batched step (test_tiny_mixed_has_no_batched_step pins that refusal)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import llmi
import pyoracle as po
from llmi.sampling import SamplingParams, sample_with_uniform

pytestmark = pytest.mark.gpu

N_CTX, N_SEQ = 256, 3
PRESETS = ("tiny-mixed", "tiny-mixed-d128")
GREEDY = SamplingParams(temperature=0.0)
# flat enough that a draw rarely lands on the argmax (sampled_differs checks that it does not)
SAMPLED = SamplingParams(temperature=1.5, top_k=40, top_p=1.0, min_p=0.0)
SEED = 20
N_TOP = 5
FIRST = (1, 42)  # the two sequences' start tokens, both at position 0
N_TAIL = 8       # tokens per run of the tails test


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def models(gpu, tiny_models):
    ms = {p: llmi.Model(tiny_models[p]) for p in PRESETS}
    yield ms
    for m in ms.values():
        m.close()


def ctx(m, **kw):
    return llmi.Context(m, n_ctx=N_CTX, n_seq=N_SEQ, **kw)


# ---- growth keeps results ---------------------------------------------------------------

def _sampled(c, n, unis):
    return c.generate_sampled_batch([0], [FIRST[0]], [0], n, [SAMPLED], unis[:, :n])


def _logprobs(c, n, unis):
    return c.generate_logprobs_batch([0], [FIRST[0]], [0], n, [SAMPLED], unis[:, :n], [N_TOP])


def _logits_all(c, toks):
    assert c.decode(toks, pos=list(range(len(toks))), logits_all=True) == 0, llmi.last_error()
    return np.stack([bits(c.logits(i)) for i in range(len(toks))])


def _embd(c, toks, pooling):
    c.set_pooling(pooling)
    c.set_embeddings(True)
    assert c.decode(toks, pos=list(range(len(toks)))) == 0, llmi.last_error()
    if pooling == llmi.POOLING_NONE:
        got = np.stack([bits(c.embeddings_ith(i)) for i in range(len(toks))])
    else:
        got = bits(c.embeddings_seq(0))
    c.set_embeddings(False)
    return got


@pytest.mark.parametrize("preset", PRESETS)
def test_growth_keeps_results(models, preset):
    """Every block that grows on demand, first small and then past its capacity, on ONE
    context: the sample and logprob rings (64 entries at first: 4 steps, then 70), the logits
    output rows (2, then 5) and the embeddings rows (pooling NONE: 3, then 9; the pooled
    vectors before and after that growth).  Each large call equals, bit for bit, the same
    call on a fresh context that made no other."""
    m = models[preset]
    rng = np.random.default_rng(SEED)
    unis = rng.random((1, 70))
    toks = [1] + [int(t) for t in rng.integers(3, m.n_vocab - 1, 8)]
    c = ctx(m)
    _sampled(c, 4, unis)
    got_s = _sampled(c, 70, unis)
    _logprobs(c, 4, unis)
    got_l = _logprobs(c, 70, unis)
    _logits_all(c, toks[:2])
    got_lg = _logits_all(c, toks[:5])
    _embd(c, toks[:3], llmi.POOLING_MEAN)
    _embd(c, toks[:3], llmi.POOLING_NONE)
    got_en = _embd(c, toks, llmi.POOLING_NONE)
    got_em = _embd(c, toks, llmi.POOLING_MEAN)
    c.close()

    def fresh(f, *a):
        x = ctx(m)
        try:
            return f(x, *a)
        finally:
            x.close()

    assert got_s == fresh(_sampled, 70, unis), "sampled tokens after the uniforms grew"
    want_l = fresh(_logprobs, 70, unis)
    assert got_l[0] == want_l[0], "tokens after the logprob rings grew"
    assert got_l[1][0] == want_l[1][0], "log-probabilities and top ids after the logprob rings grew"
    assert len(got_l[1][0]) == 70 and all(len(e[1]) == N_TOP for e in got_l[1][0])
    assert np.array_equal(got_lg, fresh(_logits_all, toks[:5])), "logits rows after the output rows grew"
    assert np.array_equal(got_en, fresh(_embd, toks, llmi.POOLING_NONE)), "embedding rows after they grew"
    assert np.array_equal(got_em, fresh(_embd, toks, llmi.POOLING_MEAN)), "pooled embedding after the rows grew"


# ---- tails do not share graphs -----------------------------------------------------------

@pytest.fixture(scope="module")
def tail_unis(tiny_models):
    """The uniforms of the tails test, checked on the CPU oracle: with them SAMPLED's tokens
    differ from the greedy ones for both start tokens on both models (so a sampled or logprob
    run that replayed a greedy graph, or the reverse, cannot pass)."""
    unis = np.random.default_rng(SEED).random((2, N_TAIL))
    for preset in PRESETS:
        om = po.OracleModel(tiny_models[preset], n_ctx=N_CTX)
        for k, first in enumerate(FIRST):
            runs = []
            for p in (GREEDY, SAMPLED):
                hist = [first]
                for j in range(N_TAIL):
                    lg = om.decode(hist[-1], j)
                    hist.append(sample_with_uniform(p, lg, hist, float(unis[k][j]) if not p.greedy else None))
                runs.append(hist[1:])
            assert runs[0] != runs[1], f"{preset}, start token {first}: the sampled reference equals the greedy one; reseed"
        om.close()
    return unis


def _tail_runs(c, k, unis):
    """greedy, sampled, logprobs, greedy again for sequences 0..k-1 from FIRST at position 0"""
    seqs, first, pos0 = list(range(k)), list(FIRST[:k]), [0] * k
    return [c.generate_greedy_batch(seqs, first, pos0, N_TAIL),
            c.generate_sampled_batch(seqs, first, pos0, N_TAIL, [SAMPLED] * k, unis[:k]),
            c.generate_logprobs_batch(seqs, first, pos0, N_TAIL, [SAMPLED] * k, unis[:k], [N_TOP] * k),
            c.generate_greedy_batch(seqs, first, pos0, N_TAIL)]


@pytest.mark.parametrize("preset,k", [("tiny-mixed", 1), ("tiny-mixed-d128", 1), ("tiny-mixed-d128", 2)])
def test_tails_do_not_share_graphs(models, tail_unis, preset, k):
    """Greedy, sampled, logprobs and greedy again at the same positions of one context with
    graphs on: the same graph key three times over, one per tail.  Every run equals the same
    run without graphs, and the greedy run is the same before and after the others."""
    m = models[preset]
    c, eager = ctx(m), ctx(m, use_graphs=False)
    got, want = _tail_runs(c, k, tail_unis), _tail_runs(eager, k, tail_unis)
    c.close()
    eager.close()
    for g, w, what in zip(got, want, ("greedy", "sampled", "logprobs", "greedy again")):
        assert g == w, f"{what}: the graph's run differs from the eager one"
    assert got[0] == got[3]
    assert got[1] != got[0] and got[2][0] == got[1], "the sampled tails ran the sampler"


def test_tiny_mixed_has_no_batched_step(models):
    c = ctx(models["tiny-mixed"])
    with pytest.raises(llmi.LlmiError, match="ffn_gate / ffn_up of different types"):
        c.generate_greedy_batch([0, 1], list(FIRST), [0, 0], 2)
    c.close()


# ---- teardown returns the memory ---------------------------------------------------------

# Device-wide free memory after three create / exercise / close cycles, minus before them
# (tests/context_lifetime_child.py), as measured on the commit before the context owned its
# memory through a pool: two runs on one MI355X read 0 and 0 (308327481344 bytes free before
# and after).  The bound is the larger of the two.
PARENT_DROP_BYTES = 0


def test_teardown_returns_the_memory(gpu, tiny_models):
    """In a fresh process: one warm-up cycle, then three more must not take more device
    memory than they did when ~Context freed a hand-written list of pointers."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-s", os.path.join(here, "context_lifetime_child.py"), os.path.dirname(here),
                        tiny_models["tiny-mixed"], tiny_models["tiny-mixed-d128"]],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    drop = d["before"] - d["after"]
    print(f"free device memory: {d['before']} before, {d['after']} after 3 cycles: drop {drop} bytes")
    assert drop <= PARENT_DROP_BYTES
