"""The scheduler over the real HIP path: a seeded sampled request gives the same tokens with
the sampler chain on the device (llmi_generate_sampled_batch, uniforms from the request's
generator) and with LLMI_DEVICE_SAMPLING=0 (the host sampler over copied logits); and a
greedy and two sampled requests decoded together each equal their solo result."""
from __future__ import annotations

import threading

import pytest

from llmi.sampling import SamplingParams
from llmi.server import Engine

pytestmark = pytest.mark.gpu

PROMPTS = ([1, 17, 300, 42], [1, 5, 99, 250, 7, 611], [1, 400, 3])
N = 24
A = SamplingParams(seed=11, temperature=1.0)
B = SamplingParams(seed=12, temperature=1.3, top_k=100, top_p=0.9, min_p=0.01, repeat_penalty=1.2, repeat_last_n=32,
                   frequency_penalty=0.2)


def _engine(path):
    eng = Engine(path, 256, 99, [0], slots=4, chunk=8)
    eng.load()
    assert eng.ready, eng.error
    return eng


def _solo(eng, prompt, p):
    toks, _ = eng.generate(prompt, N, True, lambda t: None, sampling=p)
    return toks


def test_same_seed_same_tokens_on_device_and_host(gpu, tiny_models, monkeypatch):
    path = tiny_models["tiny-mixed-d128"]
    dev = _engine(path)
    assert dev.replicas[0].device_sampling
    on_device = [_solo(dev, PROMPTS[0], A), _solo(dev, PROMPTS[1], B)]
    monkeypatch.setenv("LLMI_DEVICE_SAMPLING", "0")
    host = _engine(path)
    assert not host.replicas[0].device_sampling
    on_host = [_solo(host, PROMPTS[0], A), _solo(host, PROMPTS[1], B)]
    assert on_device == on_host and all(len(t) == N for t in on_device)
    assert on_device[0] != _solo(dev, PROMPTS[0], None)  # and they are not the greedy tokens


@pytest.mark.parametrize("preset,batched", [("tiny-mixed-d128", True), ("tiny-mixed", False)])
def test_concurrent_requests_equal_their_solo_results(gpu, tiny_models, preset, batched):
    """A greedy and two sampled requests served at once, each equal to its solo result.  On
    tiny-mixed-d128 they advance together: every generate_sampled_batch call succeeds, and
    calls of all three sequences (greedy and sampled slots in one weight pass) are among them.
    tiny-mixed has no batched step (a layer's ffn_gate and ffn_up differ in type): the calls of
    several sequences fail there and the scheduler replays them one sequence at a time."""
    eng = _engine(tiny_models[preset])
    jobs = [(PROMPTS[0], None), (PROMPTS[1], A), (PROMPTS[2], B)]
    solo = [_solo(eng, p, s) for p, s in jobs]
    ctx = eng.replicas[0].ctx
    inner, calls = ctx.generate_sampled_batch, []  # (sequences, greedy slots, succeeded)

    def counted(seqs, first, pos0, n, params, uniforms):
        calls.append([len(seqs), sum(p.greedy for p in params), False])
        out = inner(seqs, first, pos0, n, params, uniforms)
        calls[-1][2] = True
        return out

    ctx.generate_sampled_batch = counted
    reqs = [eng.submit(p, N, True, s, None) for p, s in jobs]
    got = []
    for r in reqs:
        out = []
        while (toks := r.q.get(timeout=120)) is not None:
            out += toks
        assert r.error is None, r.error
        got.append(out)
    assert got == solo
    print(f"{preset}: generate_sampled_batch calls (sequences, greedy slots, ok): {calls}")
    together = [c for c in calls if c[0] == 3]
    assert together and all(c[1] == 1 for c in together), calls
    if batched:
        assert all(c[2] for c in calls), calls
    else:
        assert not any(c[2] for c in together) and all(c[2] for c in calls if c[0] == 1), calls
