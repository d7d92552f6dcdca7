"""/v1/embeddings over the real HIP path: a server started with --embeddings --pooling mean on
the tiny-mixed model returns, for a string and for a list of three strings, exactly
normalize(ctx.embeddings_seq(...)) of a direct decode, each of unit length; a chat completion
issued before and after the embedding requests returns the same text (the embedding requests
left their slot clean and, with --cache-prompt, the prompt cache unpoisoned); and a server
without the flag answers 501."""
from __future__ import annotations

import http.client
import json
import threading

import numpy as np
import pytest

import llmi
from llmi.embedding import POOLING_NAMES, normalize
from llmi.server import Engine, make_server, parse_args

pytestmark = pytest.mark.gpu

TEXTS = ["hello world", "the quick brown fox", "a"]
CHAT = {"messages": [{"role": "user", "content": "hello there"}], "max_tokens": 12, "temperature": 0, "ignore_eos": True}


def serve(path, argv):
    """An engine and server as main() builds them from llama-server's argv."""
    a, extra = parse_args(["-m", path, "-c", "256", "-np", "2"] + argv)
    assert not extra
    eng = Engine(a.model, a.ctx_size, a.ngl, [0], slots=a.parallel, chunk=a.decode_chunk, cache_prompt=a.cache_prompt,
                 embeddings=a.embeddings, pooling=POOLING_NAMES[a.pooling] if a.pooling else None)
    eng.load()
    assert eng.ready, eng.error
    srv = make_server(eng, "127.0.0.1", 0, None)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    return eng, srv


def post(srv, path, body):
    conn = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
    conn.request("POST", path, body=json.dumps(body), headers={"content-type": "application/json", "Connection": "close"})
    r = conn.getresponse()
    d = json.loads(r.read())
    conn.close()
    return r.status, d


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("cache", [False, True], ids=["no-cache", "cache-prompt"])
def test_embeddings_route_matches_a_direct_decode(gpu, tiny_models, cache):
    path = tiny_models["tiny-mixed"]
    eng, srv = serve(path, ["--embeddings", "--pooling", "mean"] + (["--cache-prompt"] if cache else []))
    try:
        assert eng.embeddings and eng.pooling == llmi.POOLING_MEAN and eng.prompt_cache == cache
        ids = [eng.vocab.tokenize(t, add_bos=True) for t in TEXTS]
        # the vectors of a direct decode through the C ABI, on a context of its own
        m = llmi.Model(path)
        c = llmi.Context(m, n_ctx=256)
        c.set_embeddings(True)
        c.set_pooling(llmi.POOLING_MEAN)
        want = []
        for x in ids:
            c.kv_clear()
            assert c.decode(x) == 0
            want.append(normalize(c.embeddings_seq(0)))
        c.close()
        m.close()

        status, before = post(srv, "/v1/chat/completions", CHAT)
        assert status == 200
        status, one = post(srv, "/v1/embeddings", {"input": TEXTS[0]})
        assert status == 200 and len(one["data"]) == 1
        assert np.array_equal(bits(one["data"][0]["embedding"]), bits(want[0]))
        assert one["usage"] == {"prompt_tokens": len(ids[0]), "total_tokens": len(ids[0])}
        status, three = post(srv, "/v1/embeddings", {"input": TEXTS})
        assert status == 200 and [e["index"] for e in three["data"]] == [0, 1, 2]
        for e, w in zip(three["data"], want):
            v = np.asarray(e["embedding"], dtype=np.float32)
            assert np.array_equal(bits(v), bits(w))
            assert abs(float(np.linalg.norm(v.astype(np.float64))) - 1.0) < 1e-6
        status, after = post(srv, "/v1/chat/completions", CHAT)
        assert status == 200
        assert after["choices"][0]["message"]["content"] == before["choices"][0]["message"]["content"]
        assert after["llmi"]["tokens"] == before["llmi"]["tokens"]
        h = eng.health()["replicas"][0]
        assert h["embedding_requests"] == 4 and h["embedding_tokens"] == len(ids[0]) + sum(len(x) for x in ids)
    finally:
        srv.shutdown()
        srv.server_close()
        for r in eng.replicas:
            r.stop = True


def test_a_server_without_the_flag_answers_501(gpu, tiny_models):
    eng, srv = serve(tiny_models["tiny-mixed"], [])
    try:
        status, d = post(srv, "/v1/embeddings", {"input": "hello"})
        assert status == 501 and d["error"]["type"] == "not_supported_error"
        assert "embedding_requests" not in eng.health()["replicas"][0]
    finally:
        srv.shutdown()
        srv.server_close()
        for r in eng.replicas:
            r.stop = True
