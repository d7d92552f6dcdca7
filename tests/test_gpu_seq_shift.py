"""llmi_kv_self_seq_shift at engine level (n_ctx 256): a sequence that filled its context is
shifted (5 kept, 125 discarded) and decodes on past the former limit; the greedy ids after the
shift agree between a single-sequence context, slot 1 of a two-sequence context and one without
graphs.  tiny-mixed has no batched step (ffn_gate / ffn_up types differ): slot 1 steps alone there."""
from __future__ import annotations

import numpy as np
import pytest

import llmi

pytestmark = pytest.mark.gpu

N_CTX, N_PROMPT, N_KEEP, D, N_AFTER = 256, 250, 5, 125, 20


@pytest.fixture(scope="module", params=["tiny-mixed", "tiny-mixed-d128"])
def model(request, gpu, tiny_models):
    return llmi.Model(tiny_models[request.param])


def _prompt(seed, n):
    return [1] + [int(t) for t in np.random.default_rng(seed).integers(3, 700, n - 1)]


def _fill_shift_continue(model, n_seq, use_graphs):
    c, s = llmi.Context(model, n_ctx=N_CTX, use_graphs=use_graphs, n_seq=n_seq), n_seq - 1
    seqs = list(range(n_seq)) if model.n_embd // model.n_head == 128 else [s]
    pos = [N_PROMPT if q == s else 100 for q in seqs]  # the other has room to step along
    for q, n in zip(seqs, pos):
        assert c.decode(_prompt(7 if q == s else 70 + q, n), seq=[q] * n) == 0
    fill = c.generate_greedy_batch(seqs, [11] * len(seqs), pos, N_CTX - N_PROMPT)  # sequence s now holds n_ctx positions
    assert c.seq_pos_max(s) == N_CTX - 1
    with pytest.raises(llmi.LlmiError, match="exceeds n_ctx"):
        c.generate_greedy_batch([s], [fill[-1][-1]], [N_CTX], 2)  # (2: the call returns 1 for "no room")
    assert c.seq_shift(s, N_KEEP, D) and c.seq_pos_max(s) == N_CTX - D - 1, llmi.last_error()
    pos = [p + N_CTX - N_PROMPT for p in pos[:-1]] + [N_CTX - D]
    out = c.generate_greedy_batch(seqs, [f[-1] for f in fill], pos, N_AFTER)
    assert c.seq_pos_max(s) == N_CTX - D + N_AFTER - 1
    return fill[-1], out[-1]


def test_ids_after_the_shift_agree_across_step_builders(model):
    fill, want = _fill_shift_continue(model, 1, True)
    assert _fill_shift_continue(model, 2, True) == (fill, want), "slot 1 of a two-sequence context"
    assert _fill_shift_continue(model, 1, False) == (fill, want), "without graphs"


def test_refusals_change_nothing(model):
    c = llmi.Context(model, n_ctx=N_CTX, n_seq=2)
    c.decode(_prompt(9, 30), seq=[1] * 30)
    for args, word in [((-1, 0, 1), "seq_id"), ((2, 0, 1), "seq_id"), ((1, -1, 4), "n_keep"), ((1, 0, 0), "n_discard"),
                       ((1, 4, -2), "n_discard"), ((1, 20, 11), "n_keep + n_discard"), ((0, 0, 1), "n_keep + n_discard")]:
        assert c.seq_shift(*args) is False and word in llmi.last_error(), (args, llmi.last_error())
        assert [c.seq_pos_max(0), c.seq_pos_max(1)] == [-1, 29]
    assert llmi.lib().llmi_kv_self_seq_shift(None, 0, 0, 1) is False and "ctx" in llmi.last_error()
