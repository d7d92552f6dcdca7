"""The scheduler's context shift (Replica._shift; --context-shift) over test_server_prompt_cache's
stand-in context plus a recording seq_shift: llama-server's n_keep / n_discard arithmetic at the
step where the slot is full, the token list cut the same way, truncated in the response."""
from __future__ import annotations

import http.client
import json
import threading

import pytest

from llmi.server import Engine, Request, Vocab, make_server
from test_server_prompt_cache import EOS, P, V, _Ctx, _Manual, _serve

N_CTX = 32


class _ShiftCtx(_Ctx):
    def seq_shift(self, seq, n_keep, n_discard):
        self.calls.append(("seq_shift", seq, n_keep, n_discard))
        assert 0 <= n_keep and 1 <= n_discard and n_keep + n_discard <= len(self.rows[seq])
        del self.rows[seq][n_keep:n_keep + n_discard]
        return True

    def generate_greedy_batch(self, seqs, first, pos0, n):
        assert all(p + n <= N_CTX for p in pos0), "a call past the context"
        return super().generate_greedy_batch(seqs, first, pos0, n)


def _replica(ctx, **kw):
    return _Manual(0, ctx, 4, {EOS}, 4, N_CTX, cache_prompt=True, **kw)


@pytest.mark.parametrize("n_keep,add_bos,keep", [(3, True, 4), (0, False, 0), (-1, False, len(P)), (100, True, N_CTX - 3)])
def test_shift_at_the_full_step_with_upstream_arithmetic(n_keep, add_bos, keep):
    ctx = _ShiftCtx()
    rep = _replica(ctx, context_shift=True, add_bos=add_bos)
    r = _serve(rep, Request(P, 40, True, None, None, n_keep=n_keep))
    d, shifts = (N_CTX - keep) // 2, [i for i, c in enumerate(ctx.calls) if c[0] == "seq_shift"]
    assert shifts and r.finish == "length" and len(r.out) == 40 and r.truncated
    for i in shifts:  # the call before filled the context, the call after starts d lower
        _, _, pos0, n = ctx.calls[i - 1]
        assert ctx.calls[i] == ("seq_shift", r.seq, keep, d) and pos0[0] + n == N_CTX
        assert ctx.calls[i + 1][:3] == ("greedy", [r.seq], [N_CTX - d])
    want = P + r.out[:-1]  # the token list: what was fed, every shift's discard cut out, as the context holds it
    for _ in shifts:
        del want[keep:keep + d]
    assert rep.held[r.seq] == want == ctx.rows[r.seq] and r.pos == len(want) and r.shifted == d * len(shifts)


def test_without_the_flag_the_calls_are_as_before():
    plain, ctx = _Ctx(), _ShiftCtx()
    r0 = _serve(_replica(plain), Request(P, 40, True, None, None))
    r1 = _serve(_replica(ctx), Request(P, 40, True, None, None, n_keep=3))
    assert ctx.calls == plain.calls and r1.out == r0.out and len(r1.out) == N_CTX - len(P)
    assert not r1.truncated and r1.finish == "length" and not _replica(plain, context_shift=True).context_shift


def test_truncated_in_the_response():
    vocab = Vocab(["<unk>", "<s>", "</s>"] + [f" w{i}" for i in range(3, V)], 1, 2)  # (adds BOS: 3 + 1 positions kept)
    eng = Engine("fake.gguf", N_CTX, 99, [0], slots=4, chunk=4, contexts=([_ShiftCtx()], vocab), context_shift=True)
    eng.load()
    srv = make_server(eng, "127.0.0.1", 0, None)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    try:
        c = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=30)
        body = {"prompt": P, "max_tokens": 40, "temperature": 0, "ignore_eos": True, "n_keep": 3}
        c.request("POST", "/completion", body=json.dumps(body).encode(), headers={"content-type": "application/json"})
        d = json.loads(c.getresponse().read())
        assert d["truncated"] is True and len(d["llmi"]["tokens"]) == 40 and ("seq_shift", 3, 4, 14) in eng.replicas[0].ctx.calls
    finally:
        srv.shutdown()
        srv.server_close()
