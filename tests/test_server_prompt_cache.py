"""The scheduler's prompt cache (llmi/server.py Replica._admit / _place), with a stand-in
context that has seq_cp, keeps each sequence's rows and records its calls: a prompt that
extends what a sequence holds is prefilled from there on, a prefix another (busy) sequence
holds is copied, ties go to the least recently used sequence, only what was fed and kept is
remembered, failures forget, and every way of switching the cache off gives the calls the
scheduler made before it had one.  The stand-in's logits depend on ALL the rows of the
sequence, so a request served from rows the cache got wrong would not give its cold tokens."""
from __future__ import annotations

import http.client
import json
import threading

import numpy as np
import pytest

from llmi.server import Engine, Replica, Request, Vocab, make_server

V, EOS = 64, 2


class _PlainCtx:
    """llmi.Context stand-in without seq_cp."""

    def __init__(self):
        self.rows = {}        # seq -> the tokens whose rows it holds
        self.batch = []
        self.calls = []
        self.eos_after = None  # a sequence holding this many rows puts EOS first
        self.fail_decode = False

    def _lg(self, h):
        rng = np.random.default_rng(hash(tuple(h)) & 0xFFFFFFFF)
        lg = (rng.standard_normal(V) * 2.0).astype(np.float32)
        lg[EOS] = 100.0 if len(h) == self.eos_after else -100.0
        return lg

    def seq_rm(self, seq, p0=0, p1=-1):
        self.calls.append(("seq_rm", seq, p0, p1))
        self.rows[seq] = self.rows.get(seq, [])[:p0] if p0 > 0 else []
        return True

    def decode(self, tokens, pos=None, logits_all=False, seq=None):
        self.calls.append(("decode", list(tokens), None if pos is None else list(pos), list(seq), logits_all))
        if self.fail_decode:
            return 1
        assert not logits_all and len(set(seq)) == 1  # a prompt (these tests send greedy requests)
        s = seq[0]
        p0 = len(self.rows.get(s, [])) if pos is None else pos[0]
        assert p0 <= len(self.rows.get(s, [])), "a hole in the sequence"
        assert pos is None or list(pos) == list(range(p0, p0 + len(tokens)))
        self.rows[s] = self.rows.get(s, [])[:p0] + list(tokens)
        self.batch = [self._lg(self.rows[s])]
        return 0

    def logits(self, i=-1):
        return self.batch[i]

    def greedy(self, i=-1):
        return int(np.argmax(self.batch[i]))

    def generate_greedy_batch(self, seqs, first, pos0, n):
        self.calls.append(("greedy", list(seqs), list(pos0), n))
        outs = []
        for s, f, p0 in zip(seqs, first, pos0):
            assert p0 <= len(self.rows[s])
            h, o = self.rows[s][:p0], []
            t = f
            for _ in range(n):
                h.append(t)
                t = int(np.argmax(self._lg(h)))
                o.append(t)
            self.rows[s] = h
            outs.append(o)
        return outs

    def stats(self):
        return 1.0, 1.0


class _Ctx(_PlainCtx):
    def seq_cp(self, src, dst, p0=0, p1=-1):
        self.calls.append(("seq_cp", src, dst, p0, p1))
        assert src != dst and 0 <= p0 < p1 <= len(self.rows[src]) and p0 <= len(self.rows.get(dst, []))
        self.rows[dst] = self.rows.get(dst, [])[:p0] + self.rows[src][p0:p1]
        return True


class _Manual(Replica):
    def _run(self):  # the test drives _admit / _step itself
        pass


def _replica(ctx, chunk=4, cache_prompt=True):
    return _Manual(0, ctx, 4, {EOS}, chunk, 256, cache_prompt=cache_prompt)


def _admit(rep, r):
    rep.n_queued += 1
    rep._admit(r)
    return r


def _finish(rep):
    while rep.active:
        rep._step()


def _serve(rep, r):
    _admit(rep, r)
    _finish(rep)
    return r


def _req(prompt, n=6, **kw):
    return Request(prompt, n, True, None, None, **kw)


def _cold(prompt, n=6):
    return _serve(_replica(_PlainCtx()), _req(prompt, n)).out


P = [1, 9, 4, 33, 17, 5, 60, 21, 8, 47]


def test_a_prompt_that_extends_prompt_and_output_decodes_the_suffix():
    ctx = _Ctx()
    rep = _replica(ctx)
    assert rep.cache_prompt
    r1 = _serve(rep, _req(P))
    assert r1.cached == 0 and len(r1.out) == 6
    held = P + r1.out[:-1]  # the last token was sampled, never fed
    assert rep.held[r1.seq] == held
    p2 = P + r1.out + [11, 12, 13]
    ctx.calls.clear()
    r2 = _serve(rep, _req(p2))
    n = len(held)
    assert r2.seq == r1.seq and r2.cached == n
    assert ctx.calls[:2] == [("seq_rm", r1.seq, n, -1), ("decode", p2[n:], list(range(n, len(p2))), [r1.seq] * (len(p2) - n), False)]
    assert not [c for c in ctx.calls if c[0] == "seq_cp"]
    assert r2.out == _cold(p2)
    assert (rep.prompt_tokens, rep.cached_tokens) == (len(P) + len(p2), n)


def test_a_prompt_cached_in_full_still_decodes_its_last_token():
    ctx = _Ctx()
    rep = _replica(ctx)
    r1 = _serve(rep, _req(P))
    ctx.calls.clear()
    r2 = _serve(rep, _req(P))
    n = len(P) - 1
    assert r2.cached == n and r2.seq == r1.seq
    assert ctx.calls[:2] == [("seq_rm", r1.seq, n, -1), ("decode", P[n:], [n], [r1.seq], False)]
    assert r2.out == r1.out == _cold(P)
    # and a one-token prompt has nothing to reuse: the calls of a server without the cache
    ctx.calls.clear()
    r3 = _serve(rep, _req(P[:1]))
    assert r3.cached == 0 and ctx.calls[:2] == [("seq_rm", r3.seq, 0, -1), ("decode", P[:1], None, [r3.seq], False)]


def test_a_prefix_held_by_a_busy_slot_is_copied_into_the_best_free_slot():
    ctx = _Ctx()
    rep = _replica(ctx)
    busy = _admit(rep, _req(P, n=200))                    # stays active throughout
    short = _admit(rep, _req(P[:3] + [50, 51], n=2))      # shares 3 positions: copied from the busy slot
    assert ("seq_cp", busy.seq, short.seq, 0, 3) in ctx.calls and short.cached == 3
    while short in rep.active:
        rep._step()
    assert busy in rep.active and short.seq in rep.free
    q = P[:8] + [40, 41, 42]
    ctx.calls.clear()
    r = _admit(rep, _req(q, n=5))
    # the free slot with the longest prefix of its own (3), extended from the busy one (8)
    assert r.seq == short.seq and r.cached == 8
    assert ctx.calls[:3] == [("seq_cp", busy.seq, r.seq, 3, 8), ("seq_rm", r.seq, 8, -1),
                             ("decode", q[8:], [8, 9, 10], [r.seq] * 3, False)]
    while r in rep.active:
        rep._step()
    assert r.out == _cold(q, 5) and short.out == _cold(P[:3] + [50, 51], 2)
    assert busy.out == _cold(P, 200)[:len(busy.out)]      # the donor went on undisturbed


def test_ties_go_to_the_least_recently_used_slot():
    ctx = _Ctx()
    rep = _replica(ctx)
    # (no shared first token: a common BOS would already be a prefix)
    seqs = [_serve(rep, _req([20 + i, 3 + i, 9], n=2)).seq for i in range(6)]
    assert seqs[:4] == [3, 2, 1, 0]        # untouched slots first (the free list's last, as before)
    assert seqs[4:] == [3, 2]              # then the one released longest ago
    # a hot slot is not the first to be overwritten: an unrelated prompt leaves slot 2's cache
    # (the most recent) alone and takes the least recently used one
    assert _serve(rep, _req([59, 58, 9], n=2)).seq == 1
    assert rep.held[2][:3] == [25, 8, 9]


def _calls_of(ctx, rep, prompts, **kw):
    for p in prompts:
        _serve(rep, _req(p, **kw))
    return ctx.calls


def test_switched_off_the_calls_are_those_of_a_server_without_the_cache(monkeypatch):
    prompts = [P, P + [30, 31], P[:4], P]
    plain = _PlainCtx()
    rep = _replica(plain)
    assert not rep.cache_prompt
    want = _calls_of(plain, rep, prompts)
    assert want[:2] == [("seq_rm", 3, 0, -1), ("decode", P, None, [3] * len(P), False)]
    assert sum(1 for c in want if c[0] == "decode") == 4 and all(c[0] != "seq_cp" for c in want)
    # cache_prompt: false in every request
    ctx = _Ctx()
    rep = _replica(ctx)
    assert rep.cache_prompt
    assert _calls_of(ctx, rep, prompts, cache_prompt=False) == want
    assert rep.held[3] == P + _cold(P)[:-1]  # ... which are still remembered
    # not asked for (the default; --no-cache-prompt)
    ctx = _Ctx()
    rep = _Manual(0, ctx, 4, {EOS}, 4, 256)
    assert not rep.cache_prompt and _calls_of(ctx, rep, prompts) == want
    # LLMI_CACHE_PROMPT=0, read when the replica starts, wins over the flag
    monkeypatch.setenv("LLMI_CACHE_PROMPT", "0")
    ctx = _Ctx()
    rep = _replica(ctx)
    assert not rep.cache_prompt and _calls_of(ctx, rep, prompts) == want
    # ... and LLMI_CACHE_PROMPT=1 switches it on, where the context can copy
    monkeypatch.setenv("LLMI_CACHE_PROMPT", "1")
    assert _Manual(0, _Ctx(), 4, {EOS}, 4, 256).cache_prompt and not _Manual(0, _PlainCtx(), 4, {EOS}, 4, 256).cache_prompt
    monkeypatch.delenv("LLMI_CACHE_PROMPT")
    # and with the cache the same requests give the same tokens with fewer rows decoded
    ctx = _Ctx()
    rep = _replica(ctx)
    rs = [_serve(rep, _req(p)) for p in prompts]
    assert [r.out for r in rs] == [_cold(p) for p in prompts]
    cached = [r.cached for r in rs]
    assert cached[:3] == [0, len(P), 3] and cached[3] >= 4
    fed = sum(len(c[1]) for c in ctx.calls if c[0] == "decode")
    assert fed == sum(len(p) for p in prompts) - sum(cached)


def test_tokens_fed_past_an_eos_inside_a_chunk_are_not_remembered():
    ctx = _Ctx()
    ctx.eos_after = len(P) + 2  # the chunk's second token is EOS; the chunk feeds two more
    rep = _replica(ctx, chunk=4)
    r = _admit(rep, Request(P, 50, False, None, None))
    _finish(rep)
    assert r.finish == "stop" and len(r.out) == 2
    assert len(ctx.rows[r.seq]) == len(P) + 4      # what the context was fed ...
    assert rep.held[r.seq] == P + r.out            # ... and what the request kept of it
    # the next turn reuses exactly that
    ctx.eos_after = None
    p2 = P + r.out + [7]
    r2 = _serve(rep, _req(p2))
    assert r2.cached == len(P) + 2 and r2.out == _cold(p2)


def test_a_failed_decode_empties_the_entry():
    ctx = _Ctx()
    rep = _replica(ctx)
    r1 = _serve(rep, _req(P))
    assert rep.held[r1.seq]
    ctx.fail_decode = True
    r2 = _admit(rep, _req(P + [30]))
    assert r2.error and "llama_decode returned 1" in r2.error
    assert r2 not in rep.active and sorted(rep.free) == [0, 1, 2, 3]
    assert rep.held[r1.seq] == []
    ctx.fail_decode = False
    r3 = _serve(rep, _req(P))
    assert r3.cached == 0 and r3.out == _cold(P)


def test_a_failing_context_empties_the_active_entries():
    ctx = _Ctx()

    def boom(*a, **k):
        raise RuntimeError("device lost")

    ctx.generate_greedy_batch = boom
    rep = Replica(0, ctx, 4, {EOS}, 4, 256, cache_prompt=True)  # with its scheduler thread
    try:
        r = _req(P, n=50)
        rep.submit(r)
        assert r.q.get(timeout=30) == [_cold(P, 1)[0]]
        assert r.q.get(timeout=30) is None
        assert r.error == "device lost" and rep.held[r.seq] == []
    finally:
        rep.stop = True


def _http(ctxs, cache_prompt=True):
    vocab = Vocab(["<unk>", "<s>", "</s>"] + [f" w{i}" for i in range(3, V)], 1, 2)
    eng = Engine("fake.gguf", 256, 99, list(range(len(ctxs))), slots=4, chunk=4, contexts=(ctxs, vocab), cache_prompt=cache_prompt)
    eng.load()
    assert eng.ready, eng.error
    srv = make_server(eng, "127.0.0.1", 0, None)
    threading.Thread(target=srv.serve_forever, daemon=True).start()

    def call(route, body=None):
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=30)
        c.request("POST" if body is not None else "GET", route, body=None if body is None else json.dumps(body).encode(),
                  headers={"content-type": "application/json", "Connection": "close"})
        r = c.getresponse()
        raw = r.read()
        c.close()
        return r.status, raw

    return eng, srv, call


def test_cached_tokens_in_usage_and_health():
    eng, srv, call = _http([_Ctx()])
    try:
        body = {"prompt": P, "max_tokens": 6, "temperature": 0, "ignore_eos": True}
        st, raw = call("/v1/completions", body)
        d1 = json.loads(raw)
        assert st == 200 and d1["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        assert d1["usage"]["prompt_tokens"] == len(P) and "tokens_cached" not in d1
        p2 = P + d1["llmi"]["tokens"] + [11]
        st, raw = call("/completion", {**body, "prompt": p2})
        d2 = json.loads(raw)
        n = len(P) + 5
        assert st == 200 and d2["usage"]["prompt_tokens_details"] == {"cached_tokens": n} and d2["tokens_cached"] == n
        assert d2["llmi"]["tokens"] == _cold(p2)
        # streamed: the final chunk's usage
        st, raw = call("/v1/completions", {**body, "stream": True})
        last = [json.loads(x[6:]) for x in raw.decode().split("\n\n") if x.startswith("data: {")][-1]
        assert last["usage"]["prompt_tokens_details"] == {"cached_tokens": len(P) - 1}
        # cache_prompt: false prefills everything; anything but a boolean is a 400
        st, raw = call("/v1/completions", {**body, "cache_prompt": False})
        assert st == 200 and json.loads(raw)["usage"]["prompt_tokens_details"] == {"cached_tokens": 0}
        assert call("/v1/completions", {**body, "cache_prompt": "no"})[0] == 400
        assert call("/v1/completions", {**body, "n": 2})[0] == 400  # forking a prompt is not part of this
        st, raw = call("/health")
        h = json.loads(raw)["replicas"][0]
        assert h["prompt_tokens"] == 3 * len(P) + len(p2) and h["cached_tokens"] == n + len(P) - 1
    finally:
        srv.shutdown()
        srv.server_close()


@pytest.mark.parametrize("off", ["flag", "context"])
def test_without_the_cache_responses_are_what_they_were(off):
    eng, srv, call = _http([_Ctx() if off == "flag" else _PlainCtx()], cache_prompt=off != "flag")
    try:
        assert not eng.prompt_cache
        st, raw = call("/completion", {"prompt": P, "max_tokens": 6, "temperature": 0, "ignore_eos": True})
        d = json.loads(raw)
        assert st == 200 and set(d["usage"]) == {"prompt_tokens", "completion_tokens", "total_tokens"}
        assert "tokens_cached" not in d and d["llmi"]["tokens"] == _cold(P)
        h = json.loads(call("/health")[1])["replicas"][0]
        assert "prompt_tokens" not in h and "cached_tokens" not in h
    finally:
        srv.shutdown()
        srv.server_close()


def test_engine_breaks_load_ties_by_prefix():
    ctxs = [_Ctx(), _Ctx(), _Ctx()]
    eng, srv, _ = _http(ctxs)
    try:
        done = lambda *a: None  # noqa: E731
        # all idle, nothing cached: the lowest index, as before
        assert eng.run(P, 4, True, done).replica == 0
        other = [1, 30, 31, 32, 33]
        for k in (0, 1):  # replica 2 serves `other` while the two before it look busy
            eng.replicas[k].n_queued += 1
        assert eng.run(other + [34], 4, True, done).replica == 2
        for k in (0, 1):
            eng.replicas[k].n_queued -= 1
        assert eng.run(other + [35], 4, True, done).replica == 2
        assert eng.run(P + [3], 4, True, done).replica == 0
        assert eng.run([1, 55], 4, True, done).replica == 0         # no prefix anywhere beyond BOS: lowest index
        assert eng.run(other, 4, True, done, cache_prompt=False).replica == 0
        # load comes first: a busy replica loses to an idle one whatever it holds
        eng.replicas[2].n_queued += 1
        assert eng.run(other + [36], 4, True, done).replica == 0
        eng.replicas[2].n_queued -= 1
    finally:
        srv.shutdown()
        srv.server_close()
