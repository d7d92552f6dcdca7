"""llama_kv_self_seq_cp at engine level: a sequence that received another sequence's prefix by
the device copy (k_kv_seq_cp: K, V and token history) decodes on exactly as a sequence that
decoded the prefix itself.  tiny-mixed-d128, n_ctx 512, 4 sequences; every reference comes from
a fresh one-sequence context that decodes everything itself, and logits are compared bit for bit.

Covered: a full copy into a destination that held an unrelated, longer prompt, then a batched
step over source and copy; partial copies ([0, 13), and [10, 29) behind the destination's own
first 10 positions); a prompt beyond the first 256-position KV bucket and a copy that stops
short of the bucket's edge and decodes across it; the device sampler's penalty window over the
copied history; the x86 and flash-attention numerics; every refusal, which must leave both
sequences as they were."""
from __future__ import annotations

import numpy as np
import pytest

import llmi
from llmi.sampling import SamplingParams

pytestmark = pytest.mark.gpu

N_CTX, N_SEQ = 512, 4


def _toks(rng, n):
    return [1] + [int(t) for t in rng.integers(3, 700, n - 1)]


@pytest.fixture(scope="module")
def model(gpu, tiny_models):
    return llmi.Model(tiny_models["tiny-mixed-d128"])


def _ref_logits(m, prefix, tail):
    """A fresh context decodes prefix, then tail with every token's logits: [len(tail)][V]."""
    c = llmi.Context(m, n_ctx=N_CTX)
    assert c.decode(prefix) == 0
    assert c.decode(tail, pos=list(range(len(prefix), len(prefix) + len(tail))), logits_all=True) == 0
    out = np.stack([c.logits(i) for i in range(len(tail))])
    c.close()
    return out


def _ref_greedy(m, prefix, first, n):
    c = llmi.Context(m, n_ctx=N_CTX)
    assert c.decode(prefix) == 0
    out = c.generate_greedy(first, len(prefix), n)
    c.close()
    return out


def _tail_logits(c, seq, pos0, tail):
    assert c.decode(tail, pos=list(range(pos0, pos0 + len(tail))), seq=[seq] * len(tail), logits_all=True) == 0
    return np.stack([c.logits(i) for i in range(len(tail))])


def _full_copy_then_tail(m):
    rng = np.random.default_rng(41)
    dirty, prompt, tail = _toks(rng, 60), _toks(rng, 40), [int(t) for t in rng.integers(3, 700, 5)]
    c = llmi.Context(m, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(dirty, seq=[2] * 60) == 0
    assert c.decode(prompt, seq=[0] * 40) == 0
    assert c.seq_cp(0, 2), llmi.last_error()
    assert c.seq_pos_max(2) == 39 and c.seq_pos_max(0) == 39
    got = _tail_logits(c, 2, 40, tail)
    assert np.array_equal(got, _ref_logits(m, prompt, tail)), "logits after the copy differ from the reference"
    return c, prompt, tail, rng


def test_full_copy_into_a_dirty_destination(model):
    c, prompt, tail, rng = _full_copy_then_tail(model)
    assert c.seq_pos_max(2) == 44
    # source and copy advance together with different continuations
    a, b = int(rng.integers(3, 700)), int(rng.integers(3, 700))
    got = c.generate_greedy_batch([0, 2], [a, b], [40, 45], 8)
    assert got[0] == _ref_greedy(model, prompt, a, 8), "the source changed"
    assert got[1] == _ref_greedy(model, prompt + tail, b, 8)


def test_partial_copies(model):
    rng = np.random.default_rng(42)
    prompt = _toks(rng, 40)
    sfx1, sfx2 = [int(t) for t in rng.integers(3, 700, 9)], [int(t) for t in rng.integers(3, 700, 6)]
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(prompt, seq=[0] * 40) == 0
    assert c.seq_cp(0, 1, 0, 13), llmi.last_error()
    assert c.seq_pos_max(1) == 12
    assert np.array_equal(_tail_logits(c, 1, 13, sfx1), _ref_logits(model, prompt[:13], sfx1))
    # the destination decoded its own first 10 tokens; [10, 29) comes from the source
    assert c.decode(prompt[:10], seq=[3] * 10) == 0
    assert c.seq_cp(0, 3, 10, 29), llmi.last_error()
    assert c.seq_pos_max(3) == 28 and c.seq_pos_max(0) == 39
    assert np.array_equal(_tail_logits(c, 3, 29, sfx2), _ref_logits(model, prompt[:29], sfx2))
    # the source is as it was
    assert np.array_equal(_tail_logits(c, 0, 40, sfx2), _ref_logits(model, prompt, sfx2))


def test_copy_across_a_kv_bucket(model):
    rng = np.random.default_rng(43)
    prompt = _toks(rng, 300)
    first = int(rng.integers(3, 700))
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(prompt, seq=[0] * 300) == 0
    assert c.seq_cp(0, 1), llmi.last_error()
    assert c.seq_pos_max(1) == 299
    # a copy that stops 6 positions short of the bucket's edge and decodes across it
    assert c.seq_cp(0, 2, 0, 250), llmi.last_error()
    got = c.generate_greedy_batch([1, 2], [first, prompt[250]], [300, 250], 12)
    assert got[0] == _ref_greedy(model, prompt, first, 12)
    assert got[1] == _ref_greedy(model, prompt[:250], prompt[250], 12)


@pytest.mark.parametrize("params", [SamplingParams(repeat_penalty=1.3, repeat_last_n=64),
                                    SamplingParams(temperature=0.0, repeat_penalty=1.3, repeat_last_n=64)],
                         ids=["dist", "argmax"])
def test_history_is_copied_for_the_penalty_window(model, params):
    rng = np.random.default_rng(44)
    # a prompt of few distinct tokens: the window's penalties decide the sampled tokens
    dirty, prompt = _toks(rng, 60), [1] + [int(t) for t in rng.integers(3, 12, 39)]
    first, n = int(prompt[5]), 16
    unis = rng.random((1, n))
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(dirty, seq=[1] * 60) == 0
    assert c.decode(prompt, seq=[0] * 40) == 0
    assert c.decode(prompt, seq=[2] * 40) == 0  # decoded the prompt itself
    assert c.seq_cp(0, 1), llmi.last_error()
    want = c.generate_sampled_batch([2], [first], [40], n, [params], unis)
    got = c.generate_sampled_batch([1], [first], [40], n, [params], unis)
    assert got == want


@pytest.mark.parametrize("numerics", [llmi.NUMERICS_X86, llmi.NUMERICS_GENERIC | llmi.NUMERICS_FA], ids=["x86", "fa"])
def test_other_numerics(gpu, tiny_models, numerics):
    m = llmi.Model(tiny_models["tiny-mixed-d128"], numerics=numerics)
    assert m.numerics == numerics
    _full_copy_then_tail(m)


def test_zero_length_copy(model):
    rng = np.random.default_rng(45)
    prompt = _toks(rng, 20)
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(prompt, seq=[1] * 20) == 0
    assert c.seq_cp(0, 1, 0, -1), llmi.last_error()  # sequence 0 is empty
    assert c.seq_pos_max(1) == -1 and c.seq_pos_max(0) == -1


def test_refusals_change_nothing(model):
    rng = np.random.default_rng(46)
    p0_, p1_ = _toks(rng, 30), _toks(rng, 12)
    tail = [int(t) for t in rng.integers(3, 700, 2)]
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=N_SEQ)
    assert c.decode(p0_, seq=[0] * 30) == 0
    assert c.decode(p1_, seq=[1] * 12) == 0
    bad = [((-1, 1, 0, -1), "seq_src"), ((4, 1, 0, -1), "seq_src"), ((0, -1, 0, -1), "seq_dst"), ((0, 4, 0, -1), "seq_dst"),
           ((0, 0, 0, -1), "same"), ((1, 1, 0, 5), "same"),
           ((0, 1, 0, 31), "p1"),      # beyond the source's past
           ((1, 0, 0, 13), "p1"),
           ((0, 1, 13, 20), "p0"),     # beyond the destination's past: a hole
           ((0, 1, 5, 5), "p0"), ((0, 1, 6, 5), "p0"),
           ((0, 2, 1, -1), "p0")]      # an empty destination takes only p0 = 0
    for args, word in bad:
        assert c.seq_cp(*args) is False, args
        err = llmi.last_error()
        assert err.startswith("llama_kv_self_seq_cp") and word in err, (args, err)
        assert [c.seq_pos_max(s) for s in range(N_SEQ)] == [29, 11, -1, -1], args
    assert llmi.lib().llama_kv_self_seq_cp(None, 0, 1, 0, -1) is False
    assert np.array_equal(_tail_logits(c, 0, 30, tail), _ref_logits(model, p0_, tail))
    assert np.array_equal(_tail_logits(c, 1, 12, tail), _ref_logits(model, p1_, tail))
