"""The scheduler's device-sampling route (llmi/server.py Replica._step), with a stand-in
context that records its calls: greedy and eligible sampled requests leave in one
generate_sampled_batch call, fed the next draws of each request's own generator; requests
outside the device limits, contexts without the call and LLMI_DEVICE_SAMPLING=0 keep the
host path; and a seed gives the same tokens on either path."""
from __future__ import annotations

import numpy as np
import pytest

from llmi.sampling import SamplingParams, sample_with_uniform
from llmi.server import Replica, Request

V = 64


class _HostCtx:
    """llmi.Context stand-in without device sampling: logits are a fixed function of the
    sequence's last two tokens."""

    def __init__(self):
        self.hist = {}
        self.batch = []
        self.calls = []

    def seq_rm(self, seq, p0=0, p1=-1):
        self.hist.pop(seq, None)
        return True

    @staticmethod
    def _lg(h):
        rng = np.random.default_rng(h[-1] * 131 + (h[-2] if len(h) > 1 else 0))
        return (rng.standard_normal(V) * 2.0).astype(np.float32)

    def decode(self, tokens, pos=None, logits_all=False, seq=None):
        self.calls.append(("decode", list(tokens), list(seq), logits_all))
        if logits_all:  # one token per sequence
            for t, s, p in zip(tokens, seq, pos):
                self.hist[s] = self.hist[s][:p] + [t]
            self.batch = [self._lg(self.hist[s]) for s in seq]
        else:           # a prompt
            self.hist[seq[0]] = list(tokens)
            self.batch = [self._lg(self.hist[seq[0]])]
        return 0

    def logits(self, i=-1):
        return self.batch[i]

    def greedy(self, i=-1):
        return int(np.argmax(self.batch[i]))

    def _generate(self, seqs, first, pos0, n, params, unis):
        outs = []
        for s, f, p0, p, u in zip(seqs, first, pos0, params, unis):
            h, o = self.hist[s][:p0] + [f], []
            for j in range(n):
                o.append(sample_with_uniform(p, self._lg(h), h, float(u[j]) if p.temperature > 0 else None))
                h.append(o[-1])
            self.hist[s] = h[:-1]
            outs.append(o)
        return outs

    def generate_greedy_batch(self, seqs, first, pos0, n):
        self.calls.append(("greedy", list(seqs), n))
        return self._generate(seqs, first, pos0, n, [SamplingParams(temperature=0.0)] * len(seqs), [None] * len(seqs))

    def stats(self):
        return 1.0, 1.0


class _DevCtx(_HostCtx):
    def generate_sampled_batch(self, seqs, first, pos0, n, params, uniforms):
        self.calls.append(("sampled", list(seqs), n, list(params), [np.array(u, dtype=np.float64) for u in uniforms]))
        return self._generate(seqs, first, pos0, n, params, uniforms)


class _Manual(Replica):
    def _run(self):  # the test drives _admit / _step itself
        pass


def _serve(ctx, reqs, chunk=4):
    rep = _Manual(0, ctx, 4, {2}, chunk, 256)
    for r in reqs:
        rep.n_queued += 1
        rep._admit(r)
    while rep.active:
        rep._step()
    return rep


def _req(p=None, n=11):
    return Request([1, 9, 4], n, True, p, None)


DEFAULTS = SamplingParams(seed=7)
PENALIZED = SamplingParams(seed=8, temperature=1.2, top_k=20, repeat_penalty=1.3, presence_penalty=0.2, repeat_last_n=8)
WIDE = SamplingParams(seed=9, top_k=0, top_p=0.9)  # top_k <= 0: not on the device


def test_greedy_and_sampled_share_one_call_per_chunk():
    ctx = _DevCtx()
    g, a, b = _req(None), _req(DEFAULTS), _req(PENALIZED)
    _serve(ctx, [g, a, b])
    steps = [c for c in ctx.calls if c[0] != "decode" or c[3]]
    assert steps and all(c[0] == "sampled" for c in steps), [c[0] for c in steps]
    # 10 tokens after the first: chunks of 4, 4, 2, every active request in each call
    assert [c[2] for c in steps] == [4, 4, 2]
    assert all(c[1] == [g.seq, a.seq, b.seq] for c in steps)
    # the greedy slot's record is an argmax of the raw logits
    for c in steps:
        assert c[3][0].greedy and c[3][1] == DEFAULTS and c[3][2] == PENALIZED
    # each sampled request's uniforms: its generator's draws after the first token's, in order
    for slot, p in ((1, DEFAULTS), (2, PENALIZED)):
        sent = np.concatenate([c[4][slot] for c in steps])
        assert np.array_equal(sent, np.random.default_rng(p.seed).random(11)[1:])
    assert len(g.out) == len(a.out) == len(b.out) == 11


def test_same_seed_same_tokens_on_either_path(monkeypatch):
    def serve(ctx):
        reqs = [_req(None), _req(DEFAULTS), _req(PENALIZED)]
        _serve(ctx, reqs)
        return [r.out for r in reqs]

    dev, host = serve(_DevCtx()), serve(_HostCtx())
    assert dev == host
    monkeypatch.setenv("LLMI_DEVICE_SAMPLING", "0")
    ctx = _DevCtx()
    assert serve(ctx) == host
    assert not [c for c in ctx.calls if c[0] == "sampled"]


def test_requests_outside_the_device_limits_stay_on_the_host():
    ctx = _DevCtx()
    a, w = _req(DEFAULTS), _req(WIDE)
    _serve(ctx, [a, w])
    sampled = [c for c in ctx.calls if c[0] == "sampled"]
    assert sampled and all(c[1] == [a.seq] for c in sampled)
    host_steps = [c for c in ctx.calls if c[0] == "decode" and c[3]]
    assert len(host_steps) == 10 and all(c[2] == [w.seq] for c in host_steps)
    # and its tokens are the host sampler's
    solo = _HostCtx()
    w2 = _req(WIDE)
    _serve(solo, [w2])
    assert w.out == w2.out


def test_context_without_the_call_behaves_as_before():
    ctx = _HostCtx()
    g, a = _req(None), _req(DEFAULTS)
    _serve(ctx, [g, a])
    kinds = [c[0] for c in ctx.calls]
    assert "greedy" in kinds and "sampled" not in kinds
    assert sum(1 for c in ctx.calls if c[0] == "decode" and c[3]) == 10


def test_pure_greedy_batch_still_calls_generate_greedy_batch():
    ctx = _DevCtx()
    _serve(ctx, [_req(None), _req(None)])
    kinds = {c[0] for c in ctx.calls if c[0] != "decode"}
    assert kinds == {"greedy"}


def test_a_request_ending_inside_a_chunk_discards_the_rest():
    ctx = _DevCtx()
    a, b = _req(DEFAULTS, n=11), _req(PENALIZED, n=6)
    _serve(ctx, [a, b])
    assert len(a.out) == 11 and len(b.out) == 6
    alone = _DevCtx()
    a2 = _req(DEFAULTS, n=11)
    _serve(alone, [a2])
    assert a.out == a2.out  # the other request's end changed the chunking, not the stream
