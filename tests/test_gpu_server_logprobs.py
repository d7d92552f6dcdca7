"""Log-probabilities through the HTTP front end over the real HIP path: one chat request with
temperature 0, logprobs true and top_logprobs 3 returns the tokens of the same request without
them, and its entries are within the derived tolerance (tests/logprob_cases.py) of
llmi.sampling.token_logprobs over a second context's logits for those tokens."""
from __future__ import annotations

import http.client
import json
import threading

import pytest

import llmi
import logprob_cases as LC
from llmi.sampling import token_logprobs
from llmi.server import Engine, make_server

pytestmark = pytest.mark.gpu

N = 12


def test_chat_logprobs_equal_host_definition(gpu, tiny_models):
    path = tiny_models["tiny-mixed-d128"]
    eng = Engine(path, 256, 99, [0], slots=2, chunk=8, max_logprobs=20)
    eng.load()
    assert eng.ready, eng.error
    assert eng.replicas[0].device_logprobs
    srv = make_server(eng, "127.0.0.1", 0, None)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    body = {"messages": [{"role": "user", "content": "hello there"}], "max_tokens": N, "temperature": 0, "ignore_eos": True}

    def post(extra):
        conn = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
        conn.request("POST", "/v1/chat/completions", body=json.dumps({**body, **extra}).encode(),
                     headers={"content-type": "application/json", "Connection": "close"})
        r = conn.getresponse()
        raw = r.read()
        conn.close()
        assert r.status == 200, raw
        return json.loads(raw)

    try:
        plain = post({})
        with_lp = post({"logprobs": True, "top_logprobs": 3})
    finally:
        srv.shutdown()
        srv.server_close()
    ids = with_lp["llmi"]["tokens"]
    assert ids == plain["llmi"]["tokens"] and len(ids) == N
    assert "logprobs" not in plain["choices"][0] or plain["choices"][0]["logprobs"] is None
    content = with_lp["choices"][0]["logprobs"]["content"]
    assert len(content) == N

    # the host function over a second context's rows for the same tokens
    prompt = eng.vocab.chat_ids(body["messages"])
    m = llmi.Model(path)
    c = llmi.Context(m, n_ctx=256)
    assert c.decode(prompt) == 0
    rows, pos = [c.logits(-1)], len(prompt)
    for t in ids[:-1]:
        assert c.decode([t], pos=[pos]) == 0
        rows.append(c.logits(-1))
        pos += 1
    worst = 0.0
    for j, (e, t) in enumerate(zip(content, ids)):
        lse, alt, lp = token_logprobs(rows[j], 3)
        assert e["token"] == eng.vocab.detokenize([t])
        assert [a["token"] for a in e["top_logprobs"]] == [eng.vocab.detokenize([int(a)]) for a in alt], f"step {j}"
        for dev, ref in [(e["logprob"], lp[t])] + [(a["logprob"], lp[i]) for a, i in zip(e["top_logprobs"], alt)]:
            err, tol = abs(dev - float(ref)), LC.tolerance(m.n_vocab, lse, float(ref))
            assert err <= tol, f"step {j}: |{dev!r} - {float(ref)!r}| = {err:.3g} above {tol:.3g}"
            worst = max(worst, err / tol)
        assert e["top_logprobs"][0]["logprob"] == e["logprob"]  # temperature 0: the token is the first alternative
    print(f"chat logprobs over HTTP: worst error {worst:.3%} of the tolerance")
