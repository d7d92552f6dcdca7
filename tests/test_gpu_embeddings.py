"""Embeddings through llama_decode on the tiny-mixed synthetic model (2 layers, E = 256)
against the oracle on the same file: per token om.decode, om.tap(1) (the final hidden state),
pyoracle.rms_norm_mul with output_norm.weight as tests/gguf_reader.py reads it, then the
pooling of include/llmi.h in NumPy.  Every comparison is bit for bit.

The prompts are prefixes of one 70-token list, so one oracle pass serves every length: 1 (one
decode step), 2 (below the prefill's minimum run), 3 (a prefill of 2 and a step) and 70 with
LLMI_PF_UBATCH=64 in the environment when the context is created (two prefill ubatches, 64 +
5, and the step).  (The norm of a model's hidden state rests on the exactness argument the
logits' fused norm rests on, which the parity suite depends on already: DESIGN.md §5.)"""
from __future__ import annotations

import numpy as np
import pytest

import gguf_reader
import gguf_variants as gv
import llmi
import pyoracle as po

pytestmark = pytest.mark.gpu

N_CTX = 128
LENGTHS = (1, 2, 3, 70)
POOLINGS = {"mean": llmi.POOLING_MEAN, "last": llmi.POOLING_LAST, "cls": llmi.POOLING_CLS, "none": llmi.POOLING_NONE}
PROMPT = [1] + [int(t) for t in np.random.default_rng(70).integers(3, 700, 69)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pool(y: np.ndarray, pooling: int) -> np.ndarray:
    if pooling == llmi.POOLING_NONE:
        return y
    if pooling == llmi.POOLING_CLS:
        return y[0]
    if pooling == llmi.POOLING_LAST:
        return y[-1]
    inv = np.float32(1.0) / np.float32(y.shape[0])
    acc = np.zeros(y.shape[1], dtype=np.float64)
    for t in range(y.shape[0]):
        acc = acc + (y[t] * inv).astype(np.float64)
    return acc.astype(np.float32)


@pytest.fixture(scope="module")
def ref(gpu, tiny_models):
    """The oracle's normed rows y [70][E] and logits [70][V] of PROMPT, computed once."""
    path = tiny_models["tiny-mixed"]
    g = gguf_reader.read_gguf(path)
    w = next(np.frombuffer(t["data"], dtype=np.float32) for t in g["tensors"] if t["name"] == "output_norm.weight")
    eps = float(g["kv"]["llama.attention.layer_norm_rms_epsilon"])
    om = po.OracleModel(path, n_ctx=N_CTX)
    ys, lgs = [], []
    for pos, tok in enumerate(PROMPT):
        lgs.append(om.decode(tok, pos).copy())
        ys.append(po.rms_norm_mul(om.tap(1), w, eps))
    om.close()
    y, lg = np.stack(ys), np.stack(lgs)
    y.setflags(write=False)
    lg.setflags(write=False)
    return y, lg


@pytest.fixture(scope="module")
def ctx(gpu, tiny_models):
    mp = pytest.MonkeyPatch()
    mp.setenv("LLMI_PF_UBATCH", "64")  # read when the context first prefills
    mp.delenv("LLMI_NO_PREFILL", raising=False)
    m = llmi.Model(tiny_models["tiny-mixed"])
    c = llmi.Context(m, n_ctx=N_CTX, n_seq=2)
    assert m.prefill_supported
    yield c
    mp.undo()
    c.close()
    m.close()


def run(c, tokens, pooling, on=True, **kw):
    c.kv_clear()
    c.set_pooling(pooling)
    c.set_embeddings(on)
    assert c.decode(tokens, **kw) == 0, llmi.last_error()


def check(c, y, pooling, n, what):
    want = pool(y[:n], pooling)
    if pooling == llmi.POOLING_NONE:
        got = np.stack([c.embeddings_ith(i) for i in range(n)])
        assert np.array_equal(bits(c.embeddings_ith(-1)), bits(want[-1])), what
        with pytest.raises(llmi.LlmiError, match="llama_get_embeddings_seq"):
            c.embeddings_seq(0)
        with pytest.raises(llmi.LlmiError, match="outside the last batch"):
            c.embeddings_ith(n)
    else:
        got = c.embeddings_seq(0)
        with pytest.raises(llmi.LlmiError, match="llama_get_embeddings_ith"):
            c.embeddings_ith(0)
        with pytest.raises(llmi.LlmiError, match="seq_id 1 had no token"):
            c.embeddings_seq(1)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} values differ from the oracle, first at {int(bad[0])}"


@pytest.mark.parametrize("pooling", list(POOLINGS))
@pytest.mark.parametrize("n", LENGTHS)
def test_embeddings_equal_the_oracle(ctx, ref, n, pooling):
    y, lg = ref
    p = POOLINGS[pooling]
    before = ctx.prefill_tokens
    run(ctx, PROMPT[:n], p)
    assert ctx.prefill_tokens - before == (n - 1 if n >= 3 else 0)  # the path the length was chosen for
    check(ctx, y, p, n, f"{n} tokens, {pooling}")
    # the logits: the oracle's, and those of the same call with embeddings off
    with_embd = ctx.logits(-1)
    assert np.array_equal(bits(with_embd), bits(lg[n - 1]))
    run(ctx, PROMPT[:n], p, on=False)
    assert np.array_equal(bits(ctx.logits(-1)), bits(with_embd))


@pytest.mark.parametrize("pooling", list(POOLINGS))
@pytest.mark.parametrize("n", (3, 70))
def test_decode_steps_give_the_same_bits(ctx, ref, n, pooling, monkeypatch):
    """LLMI_NO_PREFILL=1: every token is a decode step, pooled one row at a time."""
    y, _ = ref
    monkeypatch.setenv("LLMI_NO_PREFILL", "1")
    before = ctx.prefill_tokens
    run(ctx, PROMPT[:n], POOLINGS[pooling])
    assert ctx.prefill_tokens == before
    check(ctx, y, POOLINGS[pooling], n, f"{n} decode steps, {pooling}")


@pytest.mark.parametrize("pooling", list(POOLINGS))
def test_two_sequences_in_one_call(ctx, ref, pooling):
    """Sequence 0 (5 tokens) and sequence 1 (1 token) interleaved in one batch: each gets the
    bits it gets alone, and the call's logits are those of the call with embeddings off."""
    y, _ = ref
    p = POOLINGS[pooling]
    tokens = [PROMPT[0], PROMPT[0]] + PROMPT[1:5]
    kw = dict(pos=[0, 0, 1, 2, 3, 4], seq=[0, 1, 0, 0, 0, 0], logits_all=True)
    run(ctx, tokens, p, **kw)
    if p == llmi.POOLING_NONE:
        rows = [0, 0, 1, 2, 3, 4]  # batch token i is this position of its sequence
        for i, r in enumerate(rows):
            assert np.array_equal(bits(ctx.embeddings_ith(i)), bits(y[r])), f"batch token {i}"
    else:
        assert np.array_equal(bits(ctx.embeddings_seq(0)), bits(pool(y[:5], p)))
        assert np.array_equal(bits(ctx.embeddings_seq(1)), bits(pool(y[:1], p)))
    with_embd = [ctx.logits(i) for i in range(6)]
    run(ctx, tokens, p, on=False, **kw)
    for i in range(6):
        assert np.array_equal(bits(ctx.logits(i)), bits(with_embd[i])), f"logits of batch token {i}"


def test_switching_off_leaves_the_context_as_it_was(ctx, ref, tiny_models):
    run(ctx, PROMPT[:5], llmi.POOLING_MEAN)
    ctx.embeddings_seq(0)
    ctx.set_embeddings(False)
    L = llmi.lib()
    assert not L.llama_get_embeddings_seq(ctx._h, 0) and "embeddings are off" in llmi.last_error()
    assert not L.llama_get_embeddings_ith(ctx._h, 0) and "embeddings are off" in llmi.last_error()
    assert not L.llama_get_embeddings(ctx._h) and "embeddings are off" in llmi.last_error()
    ctx.kv_clear()
    assert ctx.decode(PROMPT[:5]) == 0
    first = ctx.greedy(-1)
    got = [first] + ctx.generate_greedy(first, 5, 12)
    m = llmi.Model(tiny_models["tiny-mixed"])
    fresh = llmi.Context(m, n_ctx=N_CTX)
    assert fresh.decode(PROMPT[:5]) == 0
    f0 = fresh.greedy(-1)
    assert got == [f0] + fresh.generate_greedy(f0, 5, 12)
    fresh.close()
    m.close()


def test_set_pooling_refuses_rank_and_unknown_types(ctx):
    ctx.set_pooling(llmi.POOLING_CLS)
    for bad in (4, 7):
        with pytest.raises(llmi.LlmiError, match="llmi_set_pooling_type: type"):
            ctx.set_pooling(bad)
        assert ctx.pooling == llmi.POOLING_CLS


def test_pooling_type_of_the_gguf_is_the_default(gpu, tiny_models, synth_dir):
    base = tiny_models["tiny-mixed"]
    m = llmi.Model(base)
    c = llmi.Context(m, n_ctx=N_CTX)
    assert m.pooling_type == -1 and c.pooling == llmi.POOLING_NONE
    c.close()
    m.close()
    path = gv._variant(base, synth_dir, "pooling-last", lambda g: g.set_kv("llama.pooling_type", gv.U32, 3))
    m = llmi.Model(path)
    c = llmi.Context(m, n_ctx=N_CTX)
    assert m.pooling_type == 3 and c.pooling == llmi.POOLING_LAST
    c.close()
    m.close()
