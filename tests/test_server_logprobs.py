"""Log-probabilities through the HTTP front end, on stand-in contexts (no GPU): off by default,
the three routes' shapes with --max-logprobs, values equal to llmi.sampling.token_logprobs
over the stand-in's logits, refusals, streamed entries, stop strings, and the -9999.0 floor.
One stand-in has only the host calls (entries from copied logits); the other adds
generate_logprobs_batch, so the scheduler's device path runs too."""
from __future__ import annotations

import http.client
import json
import threading

import numpy as np
import pytest

from llmi.sampling import token_logprobs
from llmi.server import Engine, Vocab, make_server

V = 64


def _lg(t):
    """Logits as a fixed function of the last token; token 40's row is all -inf but three."""
    lg = np.full(V, -5.0, np.float32)
    lg[(t * 5 + 3) % V] = 2.0
    lg[(t * 7 + 1) % V] = 1.5
    lg[(t * 11 + 2) % V] = 1.0
    if t == 40:
        lg[:] = -np.inf
        lg[[7, 8, 9]] = [2.0, 1.0, 0.5]
    return lg


class HostCtx:
    """llmi.Context stand-in without the device sampler or logprobs calls."""

    def __init__(self):
        self.batch = []
        self.calls = []

    def seq_rm(self, seq, p0=0, p1=-1):
        return True

    def decode(self, tokens, pos=None, logits_all=False, seq=None):
        self.batch = list(tokens) if logits_all else [tokens[-1]]
        self.calls.append("decode")
        return 0

    def logits(self, i=-1):
        return _lg(self.batch[i])

    def greedy(self, i=-1):
        return int(np.argmax(self.logits(i)))

    def generate_greedy_batch(self, seqs, first, pos0, n):
        self.calls.append("greedy")
        outs = []
        for f in first:
            t, o = f, []
            for _ in range(n):
                t = int(np.argmax(_lg(t)))
                o.append(t)
            outs.append(o)
        return outs

    def stats(self):
        return 1.0, 1.0


class DeviceCtx(HostCtx):
    """... with the device calls (greedy chains only: what these tests send)."""

    def generate_sampled_batch(self, seqs, first, pos0, n, params, uniforms):
        self.calls.append("sampled")
        return HostCtx.generate_greedy_batch(self, seqs, first, pos0, n)

    def generate_logprobs_batch(self, seqs, first, pos0, n, params, uniforms, n_top):
        self.calls.append(("logprobs", tuple(n_top)))
        outs, lps = [], []
        for f, k in zip(first, n_top):
            t, o, e = f, [], []
            for _ in range(n):
                lg = _lg(t)
                t = int(np.argmax(lg))
                o.append(t)
                _, ids, lp = token_logprobs(lg, max(k, 0))
                e.append((float(lp[t]), [int(i) for i in ids], [float(lp[i]) for i in ids]))
            outs.append(o)
            lps.append(e if k >= 0 else None)
        return outs, lps


def _serve(ctx, **kw):
    vocab = Vocab(["<unk>", "<s>", "</s>"] + [f" w{i}" for i in range(3, V)], 1, 2)
    eng = Engine("fake.gguf", 256, 99, [0], slots=4, chunk=4, contexts=([ctx], vocab), **kw)
    eng.load()
    srv = make_server(eng, "127.0.0.1", 0, None)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def post(route, body):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=30)
        c.request("POST", route, body=json.dumps(body).encode(), headers={"content-type": "application/json", "Connection": "close"})
        r = c.getresponse()
        raw = r.read()
        c.close()
        return r.status, raw

    return eng, srv, post


@pytest.fixture(params=[HostCtx, DeviceCtx], ids=["host-entries", "device-entries"])
def server(request):
    ctx = request.param()
    eng, srv, post = _serve(ctx, max_logprobs=5)
    yield eng, post, ctx
    srv.shutdown()
    srv.server_close()


BASE = {"prompt": [1, 9], "max_tokens": 10, "temperature": 0, "ignore_eos": True}
STOPPY = {**BASE, "prompt": [1, 10]}  # ten distinct ordinary tokens: w53 w12 w63 w62 w57 w32 w35 w50 w61 w52
CHAT = {"messages": [{"role": "user", "content": " w9 w10"}], "max_tokens": 10, "temperature": 0, "ignore_eos": True}


def _expected(prompt_last, ids, k):
    """(logprob, [(alternative, logprob)]) per generated token from the stand-in's logits."""
    out, t = [], prompt_last
    for tok in ids:
        _, alt, lp = token_logprobs(_lg(t), k)
        out.append((float(lp[tok]), [(int(a), float(lp[a])) for a in alt]))
        t = tok
    return out


def _floor(x):
    return x if np.isfinite(x) else -9999.0


def test_default_server_still_refuses():
    eng, srv, post = _serve(HostCtx())
    try:
        for route, body in (("/v1/completions", {**BASE, "logprobs": 5}), ("/v1/chat/completions", {**CHAT, "logprobs": True}),
                            ("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": 3}),
                            ("/completion", {**BASE, "n_probs": 2})):
            st, raw = post(route, body)
            assert st == 400 and "logprobs" in json.loads(raw)["error"]["message"], (route, body)
        # and what it has always accepted
        for body in ({**BASE, "logprobs": 0}, {**BASE, "logprobs": False}, {**BASE, "top_logprobs": 0}):
            st, raw = post("/v1/completions", body)
            assert st == 200 and json.loads(raw)["choices"][0]["logprobs"] is None
    finally:
        srv.shutdown()
        srv.server_close()


def test_max_logprobs_is_capped_at_20():
    assert Engine("fake.gguf", 256, 99, [0], max_logprobs=50).max_logprobs == 20
    assert Engine("fake.gguf", 256, 99, [0]).max_logprobs == 0
    from llmi.server import parse_args
    assert parse_args(["-m", "x"])[0].max_logprobs == 0 and parse_args(["-m", "x", "--max-logprobs", "7"])[0].max_logprobs == 7


def test_completions_shape_and_values(server):
    eng, post, ctx = server
    st, raw = post("/v1/completions", {**BASE, "logprobs": 3})
    d = json.loads(raw)
    assert st == 200
    ids, lp = d["llmi"]["tokens"], d["choices"][0]["logprobs"]
    plain = json.loads(post("/v1/completions", BASE)[1])
    assert ids == plain["llmi"]["tokens"] and plain["choices"][0]["logprobs"] is None
    want = _expected(9, ids, 3)
    vocab = eng.vocab
    assert lp["tokens"] == [vocab.detokenize([t]) for t in ids]
    assert lp["token_logprobs"] == pytest.approx([w[0] for w in want], abs=1e-12)
    assert len(lp["top_logprobs"]) == len(ids) and all(len(t) == 3 for t in lp["top_logprobs"])
    for got, (_, alts) in zip(lp["top_logprobs"], want):
        assert list(got) == [vocab.detokenize([a]) for a, _ in alts]  # in order
        assert list(got.values()) == pytest.approx([x for _, x in alts], abs=1e-12)
    text = d["choices"][0]["text"]
    assert [text[o:o + len(t)] for o, t in zip(lp["text_offset"], lp["tokens"])] == lp["tokens"]


def test_chat_shape_and_values(server):
    eng, post, ctx = server
    st, raw = post("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": 5})
    d = json.loads(raw)
    assert st == 200
    ids, content = d["llmi"]["tokens"], d["choices"][0]["logprobs"]["content"]
    prompt = eng.vocab.chat_ids(CHAT["messages"])
    want = _expected(prompt[-1], ids, 5)
    assert len(content) == len(ids) == 10
    for e, t, (lp, alts) in zip(content, ids, want):
        assert e["token"] == eng.vocab.detokenize([t]) and e["bytes"] == list(e["token"].encode())
        assert e["logprob"] == pytest.approx(lp, abs=1e-12)
        assert [a["token"] for a in e["top_logprobs"]] == [eng.vocab.detokenize([a]) for a, _ in alts]
        assert [a["logprob"] for a in e["top_logprobs"]] == pytest.approx([_floor(x) for _, x in alts], abs=1e-12)
        assert all(a["bytes"] == list(a["token"].encode()) for a in e["top_logprobs"])
    # logprobs alone: the chosen token's value, no alternatives
    d = json.loads(post("/v1/chat/completions", {**CHAT, "logprobs": True})[1])
    assert [e["top_logprobs"] for e in d["choices"][0]["logprobs"]["content"]] == [[]] * 10
    assert [e["logprob"] for e in d["choices"][0]["logprobs"]["content"]] == pytest.approx([w[0] for w in want], abs=1e-12)


def test_completion_route_n_probs(server):
    eng, post, ctx = server
    st, raw = post("/completion", {**BASE, "n_probs": 2})
    d = json.loads(raw)
    assert st == 200
    ids, probs = d["llmi"]["tokens"], d["completion_probabilities"]
    want = _expected(9, ids, 2)
    assert [p["id"] for p in probs] == ids
    for p, (lp, alts) in zip(probs, want):
        assert p["token"] == eng.vocab.detokenize([p["id"]]) and p["bytes"] == list(p["token"].encode())
        assert p["logprob"] == pytest.approx(lp, abs=1e-12)
        assert [(a["id"], a["logprob"]) for a in p["top_logprobs"]] == [(a, pytest.approx(x, abs=1e-12)) for a, x in alts]


def test_refusals(server):
    eng, post, ctx = server
    for route, body, word in (
            ("/v1/chat/completions", {**CHAT, "top_logprobs": 2}, "requires"),
            ("/v1/chat/completions", {**CHAT, "logprobs": False, "top_logprobs": 2}, "requires"),
            ("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": 6}, "5"),
            ("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": -1}, "top_logprobs"),
            ("/v1/chat/completions", {**CHAT, "logprobs": 3}, "boolean"),
            ("/v1/completions", {**BASE, "logprobs": 6}, "5"),
            ("/v1/completions", {**BASE, "logprobs": -1}, "logprobs"),
            ("/v1/completions", {**BASE, "top_logprobs": 2}, "top_logprobs"),
            ("/completion", {**BASE, "n_probs": 21}, "5")):
        st, raw = post(route, body)
        assert st == 400 and word in json.loads(raw)["error"]["message"], (route, body, raw)


def _events(raw):
    return [json.loads(e[6:]) for e in raw.decode().split("\n\n") if e.startswith("data: {")]


def test_streamed_entries_concatenate_to_the_whole(server):
    eng, post, ctx = server
    whole = json.loads(post("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": 2})[1])
    ev = _events(post("/v1/chat/completions", {**CHAT, "logprobs": True, "top_logprobs": 2, "stream": True})[1])
    parts = [c for e in ev for c in (e["choices"][0].get("logprobs") or {}).get("content", [])]
    assert parts == whole["choices"][0]["logprobs"]["content"] and len(parts) == 10
    # every sent chunk with text carries the entries of that text's tokens
    for e in ev:
        ch = e["choices"][0]
        if ch.get("delta", {}).get("content"):
            assert "".join(c["token"] for c in ch["logprobs"]["content"]) == ch["delta"]["content"]
    # /v1/completions likewise
    whole = json.loads(post("/v1/completions", {**BASE, "logprobs": 2})[1])["choices"][0]["logprobs"]
    ev = _events(post("/v1/completions", {**BASE, "logprobs": 2, "stream": True})[1])
    got = {k: [x for e in ev for x in (e["choices"][0].get("logprobs") or {}).get(k, [])] for k in whole}
    assert got == whole


def test_entries_end_at_a_stop_string(server):
    eng, post, ctx = server
    full = json.loads(post("/v1/completions", {**STOPPY, "logprobs": 1})[1])
    words = full["choices"][0]["text"].split(" ")
    stop = " " + words[4]  # the fourth token's text: three tokens begin before the cut
    st, raw = post("/v1/completions", {**STOPPY, "logprobs": 1, "stop": stop})
    d = json.loads(raw)
    lp = d["choices"][0]["logprobs"]
    assert d["choices"][0]["finish_reason"] == "stop" and "".join(lp["tokens"]) == d["choices"][0]["text"]
    assert len(lp["tokens"]) == 3 and lp["token_logprobs"] == full["choices"][0]["logprobs"]["token_logprobs"][:3]
    # a stop string inside a token's text: that token begins before the cut and stays
    inner = words[4][1:]
    lp2 = json.loads(post("/v1/completions", {**STOPPY, "logprobs": 1, "stop": inner})[1])["choices"][0]["logprobs"]
    assert len(lp2["tokens"]) == 4
    # streamed: the same entries
    for s, want in ((stop, lp), (inner, lp2)):
        ev = _events(post("/v1/completions", {**STOPPY, "logprobs": 1, "stop": s, "stream": True})[1])
        got = {k: [x for e in ev for x in (e["choices"][0].get("logprobs") or {}).get(k, [])] for k in want}
        assert got == want and ev[-1]["choices"][0]["finish_reason"] == "stop"


def test_minus_infinity_is_written_as_the_floor(server):
    eng, post, ctx = server
    # token 40's row: three finite logits, the rest -inf, so alternatives 4 and 5 are -inf, in id order
    st, raw = post("/completion", {"prompt": [1, 40], "max_tokens": 1, "temperature": 0, "n_probs": 5})
    assert st == 200 and b"Infinity" not in raw and b"NaN" not in raw
    top = json.loads(raw)["completion_probabilities"][0]["top_logprobs"]
    assert [a["id"] for a in top] == [7, 8, 9, 0, 1] and [a["logprob"] for a in top][3:] == [-9999.0, -9999.0]
    assert all(-10.0 < a["logprob"] <= 0.0 for a in top[:3])
    from llmi.server import Handler
    h = Handler.__new__(Handler)
    h.engine = eng
    j = h._logprob_json("/v1/completions", [7], [(-np.inf, [7, 8], [-np.inf, -1.0])], [0])
    assert j["logprobs"]["token_logprobs"] == [-9999.0] and list(j["logprobs"]["top_logprobs"][0].values()) == [-9999.0, -1.0]


def test_scheduler_uses_one_device_call_for_a_mixed_group():
    """Two greedy requests at once, one wanting logprobs: with the device call they share one
    generate_logprobs_batch (-1 for the other); without it the one that wants them takes the
    host path and the other stays on the greedy call."""
    for cls in (DeviceCtx, HostCtx):
        ctx = cls()
        eng, srv, post = _serve(ctx, max_logprobs=5)
        try:
            a = eng.submit([1, 9], 8, True, None, None, 3)
            b = eng.submit([1, 11], 8, True, None, None, -1)
            for r in (a, b):
                while r.q.get(timeout=30) is not None:
                    pass
            assert len(a.out) == len(a.lp) == 8 and b.lp == [] and len(b.out) == 8
            want = _expected(9, a.out, 3)
            assert [e[0] for e in a.lp] == pytest.approx([w[0] for w in want], abs=1e-12)
            assert [e[1] for e in a.lp] == [[i for i, _ in w[1]] for w in want]
            lp_calls = [c for c in ctx.calls if isinstance(c, tuple)]
            if cls is DeviceCtx:
                assert lp_calls and all(c[1][0] == 3 and set(c[1][1:]) <= {-1} for c in lp_calls)
            else:
                assert not lp_calls and "decode" in ctx.calls
        finally:
            srv.shutdown()
            srv.server_close()
