"""POST /v1/embeddings (and upstream's aliases) of llmi/server.py against a deterministic
stand-in engine with an `embed` method (no GPU; tests/test_gpu_server_embeddings.py drives
the real one): every input form, the order of `index`, `usage`, the base64 round trip,
the normalisation, and the 400 / 401 / 500 / 501 shapes."""
from __future__ import annotations

import base64
import json
import threading

import numpy as np
import pytest

from llmi.embedding import POOLING_NAMES, normalize
from llmi.server import Vocab, make_server
from test_server import KEY, req

N_EMBD = 8


def pooled(ids) -> np.ndarray:
    """The stand-in's pooled vector of an input: a fixed function of its tokens."""
    ids = np.asarray(ids, dtype=np.float64)
    return np.array([np.sum(np.sin(ids * (e + 1))) + 0.25 * e for e in range(N_EMBD)], dtype=np.float32)


class EmbedEngine:
    def __init__(self, pooling="mean"):
        pieces = ["<unk>", "<s>", "</s>"] + [f" w{i}" for i in range(3, 100)]
        self.vocab = Vocab(pieces, 1, 2)
        self.ready, self.error, self.model_id, self.n_ctx = True, None, "fake.gguf", 16
        self.embeddings, self.pooling = True, POOLING_NAMES[pooling]
        self.calls = []

    def embed(self, tokens):
        self.calls.append(list(tokens))
        if self.pooling == POOLING_NAMES["none"]:
            return np.stack([pooled([t]) for t in tokens])
        return pooled(tokens)


@pytest.fixture()
def server(request):
    eng = EmbedEngine(getattr(request, "param", "mean"))
    srv = make_server(eng, "127.0.0.1", 0, KEY)
    threading.Thread(target=srv.serve_forever, daemon=True).start()
    yield eng, srv.server_address[1]
    srv.shutdown()
    srv.server_close()


def bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def post(port, body, path="/v1/embeddings", **kw):
    r, raw = req(port, "POST", path, body, **kw)
    return r.status, json.loads(raw)


def test_every_input_form(server):
    eng, port = server
    tok = lambda s: eng.vocab.tokenize(s, add_bos=True)  # noqa: E731
    forms = [
        ("a string", " w5 w6 w7", [tok(" w5 w6 w7")]),
        ("a list of strings", [" w5", " w6 w7", " w8"], [tok(" w5"), tok(" w6 w7"), tok(" w8")]),
        ("a list of token ids", [1, 5, 6], [[1, 5, 6]]),
        ("a list of lists", [[1, 5], [1, 6, 7, 8]], [[1, 5], [1, 6, 7, 8]]),
        ("a mixed list", [" w9", [1, 10, 11]], [tok(" w9"), [1, 10, 11]]),
    ]
    for what, inp, want_ids in forms:
        eng.calls.clear()
        status, d = post(port, {"model": "m", "input": inp})
        assert status == 200, (what, d)
        assert eng.calls == want_ids, what
        assert d["object"] == "list" and d["model"] == "m"
        assert [e["index"] for e in d["data"]] == list(range(len(want_ids))), what
        for e, ids in zip(d["data"], want_ids):
            assert e["object"] == "embedding"
            assert np.array_equal(bits(e["embedding"]), bits(normalize(pooled(ids)))), what
        n = sum(len(x) for x in want_ids)
        assert d["usage"] == {"prompt_tokens": n, "total_tokens": n}, what


def test_aliases_content_and_default_model(server):
    eng, port = server
    for path in ("/embeddings", "/embedding"):
        status, d = post(port, {"content": " w5 w6"}, path)
        assert status == 200 and d["model"] == "fake.gguf"
        assert np.array_equal(bits(d["data"][0]["embedding"]), bits(normalize(pooled(eng.vocab.tokenize(" w5 w6")))))


def test_base64_round_trip_and_normalize_modes(server):
    eng, port = server
    ids = [1, 20, 21, 22]
    status, d = post(port, {"input": ids, "encoding_format": "base64"})
    assert status == 200 and isinstance(d["data"][0]["embedding"], str)
    got = np.frombuffer(base64.b64decode(d["data"][0]["embedding"]), dtype="<f4")
    assert np.array_equal(bits(got), bits(normalize(pooled(ids))))
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-6
    status, d = post(port, {"input": ids, "embd_normalize": -1})
    assert status == 200 and np.array_equal(bits(d["data"][0]["embedding"]), bits(pooled(ids)))


@pytest.mark.parametrize("body,needle", [
    ({"input": ""}, "empty"),
    ({"input": []}, "input"),
    ({"input": [[]]}, "input"),
    ({"input": ["a", ""]}, "empty"),
    ({}, "input"),
    ({"input": 5}, "input"),
    ({"input": [1, 5000]}, "out of range"),
    ({"input": list(range(3, 20))}, "input is too large to process"),
    ({"input": [1, 5], "embd_normalize": 3}, "embd_normalize"),
    ({"input": [1, 5], "embd_normalize": 0}, "embd_normalize"),
    ({"input": [1, 5], "encoding_format": "hex"}, "encoding_format"),
], ids=["empty-string", "empty-list", "empty-ids", "empty-item", "missing", "number", "bad-id", "too-long", "norm-3", "norm-0",
        "format"])
def test_bad_requests_are_400(server, body, needle):
    eng, port = server
    status, d = post(port, body)
    assert status == 400 and d["error"]["type"] == "invalid_request_error" and d["error"]["code"] == 400
    assert needle in d["error"]["message"], d
    assert eng.calls == []


def test_invalid_json_is_400(server):
    eng, port = server
    import http.client
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request("POST", "/v1/embeddings", body=b"{not json", headers={"Authorization": f"Bearer {KEY}", "Connection": "close"})
    r = c.getresponse()
    d = json.loads(r.read())
    c.close()
    assert r.status == 400 and d["error"]["type"] == "invalid_request_error"


def test_401_without_the_key(server):
    eng, port = server
    for path in ("/v1/embeddings", "/embeddings", "/embedding"):
        status, d = post(port, {"input": "a"}, path, auth=False)
        assert status == 401 and d["error"]["type"] == "authentication_error"
    assert eng.calls == []


def test_failed_decode_is_500(server):
    eng, port = server

    def boom(tokens):
        raise RuntimeError("llama_decode returned -4")

    eng.embed = boom
    status, d = post(port, {"input": [1, 5]})
    assert status == 500 and d["error"]["type"] == "server_error" and d["error"]["code"] == 500 and "-4" in d["error"]["message"]


@pytest.mark.parametrize("server", ["none"], indirect=True)
def test_pooling_none_is_not_oai_compatible(server):
    eng, port = server
    status, d = post(port, {"input": [1, 5, 6]})
    assert status == 400 and d["error"]["type"] == "invalid_request_error"
    assert "Pooling type 'none' is not OAI compatible" in d["error"]["message"]
    # the native route returns every token's row, as it is
    status, d = post(port, {"content": [1, 5, 6]}, "/embedding")
    assert status == 200
    rows = d["data"][0]["embedding"]
    assert len(rows) == 3 and all(np.array_equal(bits(r), bits(pooled([t]))) for r, t in zip(rows, [1, 5, 6]))


def test_engine_without_embeddings_answers_501(server):
    eng, port = server
    for off in (lambda: setattr(eng, "embeddings", False), lambda: delattr(eng, "embeddings")):
        off()
        status, d = post(port, {"input": "a"})
        assert status == 501 and d["error"]["type"] == "not_supported_error" and "--embeddings" in d["error"]["message"]
    assert eng.calls == []


def test_flags():
    from llmi.server import parse_args

    a, _ = parse_args(["-m", "x.gguf"])
    assert a.embeddings is False and a.pooling is None
    for flag in ("--embeddings", "--embedding"):
        a, extra = parse_args(["-m", "x.gguf", flag, "--pooling", "last"])
        assert a.embeddings is True and a.pooling == "last" and not extra
    mp = pytest.MonkeyPatch()
    mp.setenv("LLMI_EMBEDDINGS", "1")
    try:
        assert parse_args(["-m", "x.gguf"])[0].embeddings is True
    finally:
        mp.undo()
    with pytest.raises(SystemExit):
        parse_args(["-m", "x.gguf", "--pooling", "rank"])


class FakeContext:
    """What Replica._embed needs of a context, with a log of the calls."""

    def __init__(self):
        self.pooling, self.on, self.log, self.fail = POOLING_NAMES["cls"], False, [], False

    def set_pooling(self, p):
        self.pooling = p

    def set_embeddings(self, on):
        self.on = on
        self.log.append(("embeddings", on))

    def seq_rm(self, seq, p0=0, p1=-1):
        self.log.append(("seq_rm", seq, p0))
        return True

    def decode(self, tokens, pos=None, seq=None):
        assert self.on, "embeddings are switched on around the decode"
        self.log.append(("decode", list(tokens), list(pos), list(seq)))
        self.last = list(tokens)
        return -3 if self.fail else 0

    def embeddings_seq(self, seq):
        assert self.on
        return pooled(self.last)


def test_scheduler_runs_one_decode_in_a_clean_slot():
    from llmi.server import Engine

    ctx = FakeContext()
    vocab = Vocab(["<unk>", "<s>", "</s>"] + [f" w{i}" for i in range(3, 100)], 1, 2)
    eng = Engine("fake.gguf", 32, 99, [0], slots=2, contexts=([ctx], vocab), embeddings=True, pooling=POOLING_NAMES["mean"])
    eng.load()
    assert eng.ready and eng.pooling == POOLING_NAMES["mean"] and ctx.pooling == POOLING_NAMES["mean"]
    rep = eng.replicas[0]
    rep.held[1] = [1, 2, 3]  # what the slot an input will take held for the prompt cache
    try:
        vec = eng.embed([1, 7, 8])
        assert np.array_equal(bits(vec), bits(pooled([1, 7, 8])))
        seq = ctx.log[0][1]
        assert ctx.log == [("seq_rm", seq, 0), ("embeddings", True), ("decode", [1, 7, 8], [0, 1, 2], [seq] * 3),
                           ("embeddings", False), ("seq_rm", seq, 0)]
        assert rep.held[seq] == [] and sorted(rep.free) == [0, 1] and not ctx.on
        h = eng.health()["replicas"][0]
        assert h["embedding_requests"] == 1 and h["embedding_tokens"] == 3
        ctx.fail = True
        with pytest.raises(RuntimeError, match="llama_decode returned -3"):
            eng.embed([1, 9])
        assert sorted(rep.free) == [0, 1] and not ctx.on
        assert eng.health()["replicas"][0]["embedding_requests"] == 1
    finally:
        rep.stop = True
