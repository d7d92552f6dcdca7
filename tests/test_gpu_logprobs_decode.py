"""llmi_generate_logprobs_batch: log-probabilities computed on the device next to the sampler,
by the method of tests/test_gpu_sampled_decode.py.  Tokens must be bit-identical to
llmi_generate_sampled_batch on a twin context; the log-probabilities are compared with
llmi.sampling.token_logprobs over the host path's rows (llama_decode(logits_all), one token per
call, fed the device's tokens) within the derived tolerance of tests/logprob_cases.py, the
alternatives' ids exactly."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
import logprob_cases as LC
from llmi.sampling import SamplingParams, token_logprobs

pytestmark = pytest.mark.gpu

N_CTX, N_GEN = 512, 20
GREEDY = SamplingParams(temperature=0.0)
MIX = [
    SamplingParams(),                                                        # sampled, the server's defaults
    GREEDY,
    SamplingParams(temperature=1.1, top_k=64, top_p=0.9, min_p=0.02, repeat_penalty=1.2, repeat_last_n=16,
                   presence_penalty=-0.8, frequency_penalty=0.1),           # penalized and sampled
    SamplingParams(temperature=0.0, repeat_penalty=1.5, repeat_last_n=64),   # argmax of the penalized logits
    SamplingParams(temperature=2.0, top_k=256, top_p=1.0, min_p=0.0),
    SamplingParams(top_k=1),                                                 # greedy by top_k
    SamplingParams(temperature=0.6, top_k=5, frequency_penalty=0.5, repeat_last_n=256),
    SamplingParams(temperature=1.0, top_k=40, top_p=0.5, min_p=0.3),
]
N_TOP = [5, 20, 20, 0, -1, 5, 20, 0]


def _prompts(rng, lens, V):
    return [[1] + [int(t) for t in rng.integers(3, V - 1, n - 1)] for n in lens]


def _prefill(c, prompts, seqs=None):
    firsts = []
    for s, p in zip(seqs or range(len(prompts)), prompts):
        assert c.decode(p, seq=[s] * len(p)) == 0
        firsts.append(c.greedy(-1))
    return firsts


def _host_rows(c, prompts, firsts, tokens, seqs=None):
    """The logits row of every step, [sequence][step], when the host path is fed `tokens`."""
    k, n_gen = len(prompts), len(tokens[0])
    seqs = list(range(k)) if seqs is None else seqs
    last, pos = list(firsts), [len(p) for p in prompts]
    rows = [[] for _ in range(k)]
    for j in range(n_gen):
        assert c.decode(last, pos=pos, seq=seqs, logits_all=True) == 0
        for s in range(k):
            rows[s].append(c.logits(s))
            last[s], pos[s] = tokens[s][j], pos[s] + 1
    return rows


def _check(name, rows, tokens, lps, n_top, V):
    worst = 0.0
    for s, n in enumerate(n_top):
        if n < 0:
            assert lps[s] is None
            continue
        assert len(lps[s]) == len(tokens[s])
        for j, (tok_lp, ids, top) in enumerate(lps[s]):
            lse, want_ids, lp = token_logprobs(rows[s][j], n)
            assert ids == [int(i) for i in want_ids], f"{name} sequence {s} step {j}: alternatives"
            for dev, ref in [(tok_lp, lp[tokens[s][j]])] + list(zip(top, lp[want_ids])):
                err, tol = abs(dev - float(ref)), LC.tolerance(V, lse, float(ref))
                assert err <= tol, f"{name} sequence {s} step {j}: |{dev!r} - {ref!r}| = {err:.3g} above {tol:.3g}"
                worst = max(worst, err / tol)
    print(f"{name}: worst error {worst:.3%} of the tolerance")


# (tiny-mixed, 1000 entries, has no batched step and runs the single-sequence step;
# tiny-mixed-d128 has 777 entries, which leaves the rows of a batched step unaligned)
@pytest.mark.parametrize("preset,lens,graphs", [
    ("tiny-mixed", (250,), True), ("tiny-mixed", (9,), False), ("tiny-mixed-d128", (9,), True),
    ("tiny-mixed-d128", (5, 250, 31), True), ("tiny-mixed-d128", (5, 250, 31), False),
    ("tiny-mixed-d128", (3, 17, 40, 250, 8, 100, 64, 2), True)],
    ids=["V1000-1seq-p250", "V1000-1seq-eager", "V777-1seq", "V777-3seq", "V777-3seq-eager", "V777-8seq"])
def test_logprobs_batch_equals_host_definition(gpu, tiny_models, preset, lens, graphs):
    """1, 3 and 8 sequences at different positions, 20 tokens each, one sequence crossing
    position 256 (a second graph of the family); greedy, sampled, penalized-argmax and
    penalized-sampled chains; n_top -1, 0, 5 and 20 in one call."""
    m = llmi.Model(tiny_models[preset])
    rng = np.random.default_rng(len(lens) * 10 + m.n_vocab)
    k = len(lens)
    prompts = _prompts(rng, lens, m.n_vocab)
    params = MIX[:k] if k > 1 else [MIX[2]]
    n_top = N_TOP[:k] if k > 1 else [20]
    unis = rng.random((k, N_GEN))
    pos0 = [len(p) for p in prompts]
    c = llmi.Context(m, n_ctx=N_CTX, n_seq=8, use_graphs=graphs)
    firsts = _prefill(c, prompts)
    got, lps = c.generate_logprobs_batch(list(range(k)), firsts, pos0, N_GEN, params, unis, n_top)
    twin = llmi.Context(m, n_ctx=N_CTX, n_seq=8, use_graphs=graphs)
    assert _prefill(twin, prompts) == firsts
    assert got == twin.generate_sampled_batch(list(range(k)), firsts, pos0, N_GEN, params, unis)
    ref = llmi.Context(m, n_ctx=N_CTX, n_seq=8)
    assert _prefill(ref, prompts) == firsts
    _check(f"{preset} {k} sequences", _host_rows(ref, prompts, firsts, got), got, lps, n_top, m.n_vocab)


def test_logprob_graphs_hold_nothing_of_a_call(gpu, tiny_models):
    """Two consecutive calls on one context from the same positions (the same cached graphs)
    that differ in parameters, n_top and n_gen: the second, of 70 steps, regrows the rings."""
    m = llmi.Model(tiny_models["tiny-mixed-d128"])
    rng = np.random.default_rng(78)
    prompts = _prompts(rng, (12, 30, 7), m.n_vocab)
    c, twin, ref = (llmi.Context(m, n_ctx=N_CTX, n_seq=4) for _ in range(3))
    firsts = _prefill(c, prompts)
    assert _prefill(twin, prompts) == firsts and _prefill(ref, prompts) == firsts
    pos0 = [len(p) for p in prompts]
    for params, n_top, n_gen in ((MIX[:3], [20, -1, 5], 12), ([MIX[4], MIX[6], MIX[0]], [0, 20, -1], 70)):
        unis = rng.random((3, n_gen))
        got, lps = c.generate_logprobs_batch([0, 1, 2], firsts, pos0, n_gen, params, unis, n_top)
        assert got == twin.generate_sampled_batch([0, 1, 2], firsts, pos0, n_gen, params, unis)
        _check(f"n_gen {n_gen}", _host_rows(ref, prompts, firsts, got), got, lps, n_top, m.n_vocab)
    # the single-sequence step's graphs likewise, on sequence 1
    for p, n, n_gen in ((MIX[2], 5, 8), (MIX[4], 20, 16)):
        unis = rng.random((1, n_gen))
        got, lps = c.generate_logprobs_batch([1], [firsts[1]], [pos0[1]], n_gen, [p], unis, [n])
        assert got == twin.generate_sampled_batch([1], [firsts[1]], [pos0[1]], n_gen, [p], unis)
        _check(f"one sequence n_gen {n_gen}", _host_rows(ref, prompts[1:2], firsts[1:2], got, seqs=[1]), got, lps, [n], m.n_vocab)


def test_other_calls_are_unchanged_after_logprobs(gpu, tiny_models):
    """The greedy and sampled families keep their own graphs and results."""
    m = llmi.Model(tiny_models["tiny-mixed-d128"])
    rng = np.random.default_rng(6)
    prompts = _prompts(rng, (10, 20), m.n_vocab)
    pos0 = [len(p) for p in prompts]
    fresh, c = llmi.Context(m, n_ctx=N_CTX, n_seq=2), llmi.Context(m, n_ctx=N_CTX, n_seq=2)
    firsts = _prefill(fresh, prompts)
    assert _prefill(c, prompts) == firsts
    unis = rng.random((2, N_GEN))
    want_greedy = fresh.generate_greedy_batch([0, 1], firsts, pos0, N_GEN)
    want_sampled = fresh.generate_sampled_batch([0, 1], firsts, pos0, N_GEN, [MIX[0], MIX[2]], unis)
    c.generate_logprobs_batch([0, 1], firsts, pos0, N_GEN, [MIX[0], MIX[2]], unis, [20, 0])
    assert c.generate_greedy_batch([0, 1], firsts, pos0, N_GEN) == want_greedy
    assert c.generate_sampled_batch([0, 1], firsts, pos0, N_GEN, [MIX[0], MIX[2]], unis) == want_sampled


def test_bad_n_top_is_refused_with_a_context(gpu, tiny_models):
    m = llmi.Model(tiny_models["tiny-mixed"])
    c = llmi.Context(m, n_ctx=256, n_seq=2)
    with pytest.raises(llmi.LlmiError, match=r"n_top\[1\]"):
        c.generate_logprobs_batch([0, 1], [1, 1], [0, 0], 4, [GREEDY, GREEDY], np.zeros((2, 4)), [5, 21])
