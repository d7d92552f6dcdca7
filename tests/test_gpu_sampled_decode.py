"""llmi_generate_sampled_batch: the sampler chain on the device after every step's logits,
the sampled token fed back on the device.  The reference is the host path, step by step on a
second context: llama_decode(logits_all) + llmi.sampling.sample_with_uniform with the same
uniforms.  Token ids must be identical (the comparison rule of tests/test_gpu_sample.py: a
step could be set aside only below a reference margin of 1e-9, and the seeds are chosen so
that none is, which the reference asserts).  Vocabularies of 1000 and 777 entries (the odd
one leaves the rows of a batched step unaligned)."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
from llmi.sampling import SamplingParams, sample_trace

pytestmark = pytest.mark.gpu

N_CTX, N_GEN = 512, 20
GREEDY = SamplingParams(temperature=0.0)
MIX = [
    SamplingParams(),                                                        # the server's defaults
    GREEDY,
    SamplingParams(temperature=1.1, top_k=64, top_p=0.9, min_p=0.02, repeat_penalty=1.2, repeat_last_n=16,
                   presence_penalty=0.3, frequency_penalty=0.1),
    SamplingParams(temperature=0.0, repeat_penalty=1.5, repeat_last_n=64),   # argmax of the penalized logits
    SamplingParams(temperature=2.0, top_k=256, top_p=1.0, min_p=0.0),
    SamplingParams(top_k=1),                                                 # greedy by top_k
    SamplingParams(temperature=0.6, top_k=5, frequency_penalty=0.5, repeat_last_n=256),
    SamplingParams(temperature=1.0, top_k=40, top_p=0.5, min_p=0.3),
]


def _prompts(rng, lens, V):
    return [[1] + [int(t) for t in rng.integers(3, V - 1, n - 1)] for n in lens]


def _prefill(c, prompts):
    firsts = []
    for s, p in enumerate(prompts):
        assert c.decode(p, seq=[s] * len(p)) == 0
        firsts.append(c.greedy(-1))
    return firsts


def _host_path(c, prompts, firsts, params, unis, n_gen, seqs=None):
    """The parent's path: one llama_decode per token with every slot's logits copied, sampled
    on the host (sequence seqs[i] of c holds prompts[i]; default 0 .. k-1).  Returns the tokens
    and the smallest decision margin met."""
    k = len(prompts)
    seqs = list(range(k)) if seqs is None else seqs
    hist = [list(p) + [f] for p, f in zip(prompts, firsts)]
    out, margin = [[] for _ in range(k)], float("inf")
    for j in range(n_gen):
        rc = c.decode([h[-1] for h in hist], pos=[len(h) - 1 for h in hist], seq=seqs, logits_all=True)
        assert rc == 0
        for s in range(k):
            tr = sample_trace(params[s], c.logits(s), hist[s], float(unis[s][j]) if params[s].temperature > 0.0 else None)
            margin = min(margin, tr.margin)
            out[s].append(tr.token)
            hist[s].append(tr.token)
    assert margin >= 1e-9, f"reference margin {margin:.3g}: reseed the case (nothing may be set aside)"
    return out, margin


# (tiny-mixed, 1000 entries, has a layer whose ffn_gate and ffn_up differ in type: it has no
# batched step, so it runs the single-sequence step; tiny-mixed-d128 has 777 entries)
@pytest.mark.parametrize("preset,lens", [("tiny-mixed", (9,)), ("tiny-mixed", (250,)), ("tiny-mixed-d128", (9,)),
                                         ("tiny-mixed-d128", (5, 250, 31)),
                                         ("tiny-mixed-d128", (3, 17, 40, 250, 8, 100, 64, 2))],
                         ids=["V1000-1seq", "V1000-1seq-p250", "V777-1seq", "V777-3seq", "V777-8seq"])
def test_sampled_batch_equals_host_path(gpu, tiny_models, preset, lens):
    """1, 3 and 8 sequences at different positions, 20 tokens each; one sequence crosses
    position 256 (a new KV bucket, so a second sampled graph); greedy rows in the same call
    equal generate_greedy_batch alone."""
    m = llmi.Model(tiny_models[preset])
    rng = np.random.default_rng(len(lens) * 10 + m.n_vocab)
    k = len(lens)
    prompts = _prompts(rng, lens, m.n_vocab)
    params = MIX[:k]
    unis = rng.random((k, N_GEN))
    c = llmi.Context(m, n_ctx=N_CTX, n_seq=8)
    firsts = _prefill(c, prompts)
    got = c.generate_sampled_batch(list(range(k)), firsts, [len(p) for p in prompts], N_GEN, params, unis)
    ref = llmi.Context(m, n_ctx=N_CTX, n_seq=8)
    assert _prefill(ref, prompts) == firsts
    want, margin = _host_path(ref, prompts, firsts, params, unis, N_GEN)
    print(f"{preset} V {m.n_vocab} {k} sequences: smallest reference margin {margin:.3g}")
    for s in range(k):
        assert got[s] == want[s], f"sequence {s} ({params[s]})"
    greedy = [s for s in range(k) if params[s].greedy]
    if greedy:
        alone = llmi.Context(m, n_ctx=N_CTX, n_seq=8)
        _prefill(alone, prompts)
        g = alone.generate_greedy_batch(greedy, [firsts[s] for s in greedy], [len(prompts[s]) for s in greedy], N_GEN)
        assert [got[s] for s in greedy] == g


def test_sampled_graphs_hold_nothing_of_a_call(gpu, tiny_models):
    """Two consecutive calls on one context at the same positions (the same cached graphs)
    with different parameters and uniforms: each equals its own reference."""
    m = llmi.Model(tiny_models["tiny-mixed-d128"])
    rng = np.random.default_rng(77)
    prompts = _prompts(rng, (12, 30, 7), m.n_vocab)
    c, ref = llmi.Context(m, n_ctx=N_CTX, n_seq=4), llmi.Context(m, n_ctx=N_CTX, n_seq=4)
    firsts = _prefill(c, prompts)
    assert _prefill(ref, prompts) == firsts
    pos0 = [len(p) for p in prompts]
    for params in (MIX[:3], [MIX[4], MIX[6], MIX[0]]):
        unis = rng.random((3, N_GEN))
        got = c.generate_sampled_batch([0, 1, 2], firsts, pos0, N_GEN, params, unis)
        want, _ = _host_path(ref, prompts, firsts, params, unis, N_GEN)
        assert got == want
    # and the single-sequence step's sampled graph likewise
    for p in (MIX[2], MIX[4]):
        unis = rng.random((1, N_GEN))
        got = c.generate_sampled_batch([1], [firsts[1]], [pos0[1]], N_GEN, [p], unis)
        want, _ = _host_path(ref, prompts[1:2], firsts[1:2], [p], unis, N_GEN, seqs=[1])
        assert got == want


def test_greedy_is_unchanged_after_sampling(gpu, tiny_models):
    m = llmi.Model(tiny_models["tiny-mixed-d128"])
    rng = np.random.default_rng(5)
    prompts = _prompts(rng, (10, 20), m.n_vocab)
    pos0 = [len(p) for p in prompts]
    fresh = llmi.Context(m, n_ctx=N_CTX, n_seq=2)
    firsts = _prefill(fresh, prompts)
    want_batch = fresh.generate_greedy_batch([0, 1], firsts, pos0, N_GEN)
    want_one = fresh.generate_greedy_batch([1], [firsts[1]], [pos0[1]], N_GEN)
    c = llmi.Context(m, n_ctx=N_CTX, n_seq=2)
    assert _prefill(c, prompts) == firsts
    c.generate_sampled_batch([0, 1], firsts, pos0, N_GEN, [MIX[0], MIX[2]], rng.random((2, N_GEN)))
    c.generate_sampled_batch([1], [firsts[1]], [pos0[1]], N_GEN, [MIX[0]], rng.random((1, N_GEN)))
    assert c.generate_greedy_batch([0, 1], firsts, pos0, N_GEN) == want_batch
    assert c.generate_greedy_batch([1], [firsts[1]], [pos0[1]], N_GEN) == want_one
    assert want_one[0] == want_batch[1]
    # the single-context entry point on a one-sequence context
    one, one_fresh = llmi.Context(m, n_ctx=N_CTX), llmi.Context(m, n_ctx=N_CTX)
    for x in (one, one_fresh):
        assert x.decode(prompts[0]) == 0
    one.generate_sampled_batch([0], [firsts[0]], [pos0[0]], N_GEN, [MIX[4]], rng.random((1, N_GEN)))
    assert one.generate_greedy(firsts[0], pos0[0], N_GEN) == one_fresh.generate_greedy(firsts[0], pos0[0], N_GEN)


def test_device_limits_are_refused_with_a_context(gpu, tiny_models):
    m = llmi.Model(tiny_models["tiny-mixed"])
    c = llmi.Context(m, n_ctx=256, n_seq=2)
    for bad, field in ((SamplingParams(top_k=0), "top_k"), (SamplingParams(repeat_last_n=-1), "repeat_last_n")):
        with pytest.raises(llmi.LlmiError, match=field):
            c.generate_sampled_batch([0, 1], [1, 1], [0, 0], 4, [SamplingParams(), bad], np.zeros((2, 4)))
    with pytest.raises(llmi.LlmiError, match="exceeds n_ctx"):
        c.generate_sampled_batch([0], [1], [250], 10, [SamplingParams()], np.zeros((1, 10)))
