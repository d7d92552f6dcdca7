"""The streamed flash-attention decode kernel (k_attn_fa_s / k_battn_fa_s, attnfa_stream.hip;
test option "fa_stream": 0 by length, 1 streamed at every length, 2 k_attn_fa alone), bit for
bit against the oracle's attn_head_fa (pyoracle.attention, no length limit):

- forced streamed at the lengths where the tile hand-off, the carried maximum, the ragged
  last tile and the double buffer can go wrong (TK from llmi_fa_stream_tile);
- by length across k_attn_fa's 8192 positions; batched slots against their own launches;
- whole models: a context that crosses 8192 positions, and the streamed kernel through the
  step graphs and the batched step; the flash prefill kernel past 8192 positions.
Inputs as test_gpu_fa_prefill._tie_case: tied scores, NaN in every stale cache position, V
scaled so that the f16 accumulator (n_kv * max |v|, not normalised) stays finite.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

import llmi
import pyoracle as po
from test_gpu_fa_prefill import ASSOC, _kernel_vs_decode, _tie_case

pytestmark = pytest.mark.gpu

TK = llmi.lib().llmi_fa_stream_tile()
EDGES = [1, 2, TK - 1, TK, TK + 1, 2 * TK - 1, 2 * TK, 2 * TK + 1, 3 * TK + 5]


@contextlib.contextmanager
def _options(num, fa_stream):
    old = llmi.test_option("numerics", num | llmi.NUMERICS_FA), llmi.test_option("fa_stream", fa_stream)
    try:
        yield
    finally:
        llmi.test_option("numerics", old[0]), llmi.test_option("fa_stream", old[1])


def _inputs(shape, n_kv, n_ctx, seed):
    """q [H][D], K and V of n_ctx positions, n_kv of them live, |v| * n_kv < 65504."""
    H, HK, D = shape
    e = 0
    while n_kv * 2.0 ** (14 + e) >= 65504:
        e -= 1
    q, K, V, nc, _ = _tie_case(H, HK, D, 1, n_kv - 1, seed, v_exp=e)
    Kp, Vp = np.full((HK, n_ctx, D), np.nan, np.float16), np.full((HK, D, n_ctx), np.nan, np.float16)
    Kp[:, :n_kv], Vp[:, :, :n_kv] = K[:, :n_kv], V[:, :, :n_kv]
    return q[0], Kp, Vp


def _attend(shape, n_kvs, n_ctx, q, K, V):
    """llmi_attention (n_kvs an int) or llmi_battention (a list: q, K, V stacked per slot)."""
    import torch
    from helpers import to_dev

    H, HK, D = shape
    qd, kd, vd = to_dev(q.reshape(-1)), to_dev(K.view(np.uint16).reshape(-1)), to_dev(V.view(np.uint16).reshape(-1))
    out = torch.full(q.shape, float("nan"), dtype=torch.float32, device="cuda")
    if isinstance(n_kvs, int):
        rc = llmi.lib().llmi_attention(H, HK, D, n_kvs, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), 0)
    else:
        rc = llmi.lib().llmi_battention(H, HK, D, len(n_kvs), (ctypes.c_int32 * len(n_kvs))(*n_kvs), n_ctx,
                                        qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr())
    assert rc == 0, llmi.last_error()
    return out.cpu().numpy()


def _vs_oracle(shape, n_kv, n_ctx, assoc, fa_stream):
    num, flags = ASSOC[assoc]
    q, K, V = _inputs(shape, n_kv, n_ctx, seed=7 * n_kv + shape[0] + num)
    want = po.attention(q, K, V, n_kv, x86=flags | po.X86_FA)
    assert np.isfinite(want).all()
    with _options(num, fa_stream):
        got = _attend(shape, n_kv, n_ctx, q, K, V)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{np.argwhere(got != want)[:3].tolist()}"


@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("n_kv", EDGES)
@pytest.mark.parametrize("shape", [(8, 8, 64), (32, 8, 128), (32, 4, 64)], ids=str)   # G = 1, 4, 8
def test_streamed_kernel_vs_oracle(gpu, shape, n_kv, assoc):
    _vs_oracle(shape, n_kv, (n_kv + 255) // 256 * 256, assoc, 1)


@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("n_kv", [8192, 8193, 8449])
def test_by_length_across_the_one_pass_limit(gpu, n_kv, assoc):
    """8192 runs k_attn_fa, 8193 and 8449 (KV bounds 8448 and 8704) the streamed kernel."""
    _vs_oracle((32, 8, 128), n_kv, 8704, assoc, 0)


@pytest.mark.parametrize("assoc", ["generic", "x86"])
def test_batched_slots_equal_their_own_launches(gpu, assoc):
    shape, n_ctx, n_kvs = (32, 8, 128), 8448, [1, TK, TK + 1, 2 * TK + 3, 8193]
    q, K, V = (np.stack(x) for x in zip(*[_inputs(shape, n, n_ctx, seed=n) for n in n_kvs]))
    with _options(ASSOC[assoc][0], 0):
        got = _attend(shape, n_kvs, n_ctx, q, K, V)   # KV bound 8448: every slot streamed
        for t, n in enumerate(n_kvs):
            want = _attend(shape, n, n_ctx, q[t], K[t], V[t])
            assert np.isfinite(want).all() and np.array_equal(got[t].view(np.uint32), want.view(np.uint32)), f"slot {t}"


def _lockstep(path, n_ctx, prompt, n_gen):
    """The prompt, then n_gen greedy steps: logits bit-identical to the oracle's at each."""
    om = po.OracleModel(path, n_ctx=n_ctx, x86=po.X86_FA)
    m = llmi.Model(path, numerics=llmi.NUMERICS_FA)
    c = llmi.Context(m, n_ctx=n_ctx)
    if len(prompt) > 1:
        om.prefill(prompt[:-1])
    lo, pos = om.decode(prompt[-1], len(prompt) - 1), len(prompt)
    assert c.decode(prompt) == 0, llmi.last_error()
    for step in range(n_gen):
        assert np.array_equal(c.logits(-1), lo), f"step {step} (position {pos - 1})"
        t = int(np.argmax(lo))
        lo = om.decode(t, pos)
        assert c.decode([t], pos=[pos]) == 0, llmi.last_error()
        pos += 1
    assert np.array_equal(c.logits(-1), lo)
    om.close(), c.close()
    return m


def test_context_crosses_8192_positions(gpu, synth_dir):
    path = str(synth_dir / "tiny-mixed-d128-L1.gguf")
    llmi.write_synthetic_gguf(path, "tiny-mixed-d128", seed=5, n_layer=1)
    prompt = [1] + [int(t) for t in np.random.default_rng(3).integers(3, 700, 8184)]
    old = llmi.test_option("fa_stream", 0)
    try:
        _lockstep(path, 8448, prompt, 30).close()   # positions 8185 .. 8214
    finally:
        llmi.test_option("fa_stream", old)


def test_streamed_through_graphs_and_batched_steps(gpu, tiny_models):
    old = llmi.test_option("fa_stream", 1)
    try:
        m = _lockstep(tiny_models["tiny-mixed-d128"], 256, [1], 40)
        c, c1 = llmi.Context(m, n_ctx=256, n_seq=3), llmi.Context(m, n_ctx=256)
        got = c.generate_greedy_batch([0, 1, 2], [5, 9, 11], [0, 0, 0], 40)
        for k, first in enumerate((5, 9, 11)):
            c1.kv_clear()
            assert c1.generate_greedy(first, 0, 40) == got[k]
        c.close(), c1.close(), m.close()
    finally:
        llmi.test_option("fa_stream", old)


@pytest.mark.parametrize("assoc", ["generic", "x86"])
def test_pf_attention_fa_past_8192_positions(gpu, monkeypatch, assoc):
    """12 rows ending at 8192 + 300 positions against 12 (streamed) decode launches."""
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    old = llmi.test_option("fa_stream", 0)
    try:
        _kernel_vs_decode(32, 8, 128, 12, 8192 + 300 - 12, assoc, -12)
    finally:
        llmi.test_option("fa_stream", old)
