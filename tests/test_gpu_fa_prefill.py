"""Batched prefill in the flash-attention numerics (opt-in, LLMI_FA_PREFILL=1; k_pf_attn_fa
in pfattnfa.hip).  The bar is BIT IDENTITY with flash-attention decode steps
(k_attn_fa), which tests/test_gpu_fa.py pins to the oracle's OR_X86_FA mode:

- the kernel (llmi_pf_attention_fa) against T launches of the decode kernel
  (llmi_attention under numerics assoc | NUMERICS_FA), every GQA group and head dim, ragged
  token counts, prompts starting mid-cache, NaN in every stale cache position (a causal
  edge that multiplies by zero instead of skipping shows as NaN), duplicated K rows (ties
  take the `else` branch of the running max);
- end to end against the oracle on the tiny presets, with the token counter proving that
  the batched path ran (and that without the variable nothing changed);
- across ubatch boundaries and a second batch at n_past > 0, at real widths, and into a
  sequence of a multi-sequence context: prefill against steps.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import llmi
import pyoracle as po
from test_gpu_pf_attention import _case

pytestmark = pytest.mark.gpu

F32 = np.float32
ASSOC = {"generic": (llmi.NUMERICS_GENERIC, 0), "x86": (llmi.NUMERICS_X86, po.X86_ALL)}


def _tie_case(H, HK, D, T, pos0, seed, v_exp=-10):
    """_case of test_gpu_pf_attention plus two duplicated K rows per KV head: equal scores,
    so the second of each pair takes the `else` branch (vs = expf(0)) in every query row
    that sees both.

    V is scaled by 2^v_exp = 2^-10 (to 2^-24 .. 2^4, f16 subnormals included): this mode accumulates
    V in f16 without normalising (|VKQ| <= n_kv * max |v|), so _case's values up to 2^14
    overflow the REFERENCE to inf at n_kv in the hundreds; with |v| <= 16 and n_kv <= 770
    the accumulator stays below 12320 < 65504, the decode kernel's results are finite, and
    a non-finite output can only be a stale (NaN) position that leaked in.  (At the 8192
    positions of the KV limit: 2^-14, |v| <= 1.)"""
    q, K, V, n_ctx, G = _case(H, HK, D, T, pos0, seed)
    V = (V.astype(F32) * F32(2.0 ** v_exp)).astype(np.float16)   # stale positions stay NaN
    rng = np.random.default_rng(seed + 1000)
    nkv = pos0 + T
    for g in range(HK):
        for _ in range(2):
            if nkv >= 2:
                src, dst = rng.choice(nkv, size=2, replace=False)
                K[g, dst, :] = K[g, src, :]
    return q, K, V, n_ctx, G


@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("H,HK,D,T,pos0", [
    (32, 8, 128, 64, 0),      # Llama-3 / Mistral heads, the first ubatch, one whole key tile
    (32, 8, 128, 37, 700),    # ragged, mid-cache (pos0 not a multiple of the key tile)
    (32, 4, 64, 40, 300),     # TinyLlama heads (G = 8)
    (64, 8, 128, 24, 500),    # 70B heads (G = 8)
    (16, 8, 128, 21, 260),    # G = 2
    (8, 8, 64, 70, 130),      # G = 1 (three query tiles, the last ragged)
    (8, 8, 64, 3, 0),         # three positions: the first one alone (Mold = -inf)
])
def test_pf_attention_fa_equals_decode_kernel(gpu, H, HK, D, T, pos0, assoc):
    _kernel_vs_decode(H, HK, D, T, pos0, assoc, -10)


@pytest.mark.parametrize("assoc", ["generic", "x86"])
def test_pf_attention_fa_at_the_kv_limit(gpu, assoc):
    """The last 12 rows below kFaMaxKV = 8192 positions (128 key tiles, the last one whole),
    the longest run the engine sends to the kernel."""
    _kernel_vs_decode(32, 8, 128, 12, 8192 - 12, assoc, -14)


def _kernel_vs_decode(H, HK, D, T, pos0, assoc, v_exp):
    import torch
    from helpers import to_dev

    num = ASSOC[assoc][0]
    q, K, V, n_ctx, G = _tie_case(H, HK, D, T, pos0, seed=131 * T + pos0 + num, v_exp=v_exp)
    L = llmi.lib()
    qd = to_dev(np.ascontiguousarray(q.reshape(-1)))
    kd = to_dev(K.view(np.uint16).reshape(-1))
    vd = to_dev(V.view(np.uint16).reshape(-1))
    got_d = torch.full((T * H * D,), float("nan"), dtype=torch.float32, device="cuda")
    want_d = torch.full((T, H * D), float("nan"), dtype=torch.float32, device="cuda")
    old = llmi.test_option("numerics", num | llmi.NUMERICS_FA)
    try:
        us = L.llmi_pf_attention_fa(H, HK, D, T, pos0, n_ctx, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(),
                                    got_d.data_ptr())
        assert us >= 0, llmi.last_error()
        for t in range(T):
            rc = L.llmi_attention(H, HK, D, pos0 + t + 1, n_ctx, qd.data_ptr() + 4 * t * H * D, kd.data_ptr(),
                                  vd.data_ptr(), want_d[t].data_ptr(), 0)
            assert rc == 0, llmi.last_error()
    finally:
        llmi.test_option("numerics", old)
    got = got_d.cpu().numpy().reshape(T, H, D)
    want = want_d.cpu().numpy().reshape(T, H, D)
    assert np.isfinite(want).all()
    assert np.isfinite(got).all(), "a stale (NaN) cache position leaked into the output"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{len(bad)} outputs differ, first (t, h, d) {bad[:3].tolist()}: "
                           f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def _prompt(n, seed, hi):
    rng = np.random.default_rng(seed)
    return [1] + [int(t) for t in rng.integers(3, hi, n - 1)]


def _run(m, prompt, n_ctx, n_gen, second=None):
    """Logits after the prompt (and after `second`, a batch at n_past = len(prompt)), then
    n_gen greedy steps; the context's prefill token count."""
    c = llmi.Context(m, n_ctx=n_ctx)
    assert c.decode(prompt) == 0
    out = [c.logits(-1)]
    pos = len(prompt)
    if second:
        assert c.decode(second, pos=list(range(pos, pos + len(second)))) == 0
        out.append(c.logits(-1))
        pos += len(second)
    for _ in range(n_gen):
        t = c.greedy(-1)
        assert c.decode([t], pos=[pos]) == 0
        out.append(c.logits(-1))
        pos += 1
    n_pf = c.prefill_tokens
    c.close()
    return out, n_pf


def _assert_steps_equal(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what} step {k}: max |d| {np.abs(x - y).max():.3g}"


@pytest.fixture(scope="module")
def oracle_logits(tiny_models):
    """Oracle logits per (preset, assoc, n_prompt), computed once: prompt, then 6 greedy steps."""
    cache = {}

    def get(preset, assoc, n_prompt):
        key = (preset, assoc, n_prompt)
        if key not in cache:
            prompt = _prompt(n_prompt, 11 + n_prompt, 700)
            om = po.OracleModel(tiny_models[preset], n_ctx=512, x86=ASSOC[assoc][1] | po.X86_FA)
            if len(prompt) > 1:
                om.prefill(prompt[:-1])
            lo = om.decode(prompt[-1], len(prompt) - 1)
            out, pos = [lo], len(prompt)
            for _ in range(6):
                lo = om.decode(int(np.argmax(lo)), pos)
                out.append(lo)
                pos += 1
            om.close()
            cache[key] = (prompt, out)
        return cache[key]

    return get


@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("n_prompt", [2, 37, 70, 300])
@pytest.mark.parametrize("preset", ["tiny-mixed", "tiny-mixed-d128"])
def test_fa_prefill_vs_oracle_tiny(gpu, tiny_models, oracle_logits, monkeypatch, preset, n_prompt, assoc):
    prompt, want = oracle_logits(preset, assoc, n_prompt)
    monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    m = llmi.Model(tiny_models[preset], numerics=ASSOC[assoc][0] | llmi.NUMERICS_FA)
    assert m.prefill_supported
    got, n_pf = _run(m, prompt, 512, 6)
    # every token but the last (a decode step, for its logits) is prefilled; the engine
    # prefills runs of >= 2 tokens (capi.cpp kPrefillMin), so the 2-token prompt's single
    # leading token is a decode step in every numerics
    assert n_pf == (len(prompt) - 1 if len(prompt) - 1 >= 2 else 0)
    _assert_steps_equal(got, want, f"{preset} {assoc}")
    m.close()


@pytest.mark.parametrize("assoc", ["generic", "x86"])
def test_fa_prefill_is_opt_in(gpu, tiny_models, oracle_logits, monkeypatch, assoc):
    """Without LLMI_FA_PREFILL the same model runs its prompt as decode steps, as before;
    the variable is read on every call, so one model serves both ways."""
    prompt, want = oracle_logits("tiny-mixed-d128", assoc, 37)
    monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
    monkeypatch.delenv("LLMI_FA_PREFILL", raising=False)
    m = llmi.Model(tiny_models["tiny-mixed-d128"], numerics=ASSOC[assoc][0] | llmi.NUMERICS_FA)
    assert not m.prefill_supported
    got, n_pf = _run(m, prompt, 512, 6)
    assert n_pf == 0
    _assert_steps_equal(got, want, "steps")
    monkeypatch.setenv("LLMI_FA_PREFILL", "0")
    assert not m.prefill_supported
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    assert m.prefill_supported
    got, n_pf = _run(m, prompt, 512, 6)
    assert n_pf == len(prompt) - 1
    _assert_steps_equal(got, want, "prefill")
    monkeypatch.setenv("LLMI_NO_PREFILL", "1")   # still wins
    got, n_pf = _run(m, prompt, 512, 6)
    assert n_pf == 0
    _assert_steps_equal(got, want, "LLMI_NO_PREFILL")
    m.close()


@pytest.mark.parametrize("assoc", ["generic", "x86"])
def test_fa_prefill_ubatch_boundary_and_second_turn(gpu, tiny_models, monkeypatch, assoc):
    """Ubatches of 64, 64 and 21 tokens (the second and third start mid-cache and read the KV
    rows the GEMMs of the ones before wrote), then a second batch of 9 tokens at n_past =
    150 (pos0 not a multiple of the key tile): the bits of decode steps."""
    monkeypatch.setenv("LLMI_PF_UBATCH", "64")   # read when the context allocates its scratch
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    prompt, second = _prompt(150, 5, 700), [int(t) for t in np.random.default_rng(6).integers(3, 700, 9)]
    m = llmi.Model(tiny_models["tiny-mixed-d128"], numerics=ASSOC[assoc][0] | llmi.NUMERICS_FA)
    monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
    a, n_pf = _run(m, prompt, 256, 2, second)
    assert n_pf == 149 + 8
    monkeypatch.setenv("LLMI_NO_PREFILL", "1")
    b, n_st = _run(m, prompt, 256, 2, second)
    assert n_st == 0
    _assert_steps_equal(a, b, assoc)
    m.close()


@pytest.mark.parametrize("assoc", ["generic", "x86"])
@pytest.mark.parametrize("preset,n_prompt", [("llama3-8b-q4km", 131),   # G = 4, D = 128
                                             ("tinyllama-q8_0", 96)])   # G = 8, D = 64
def test_fa_prefill_vs_steps_real_widths(gpu, synth_dir, monkeypatch, preset, n_prompt, assoc):
    path = str(synth_dir / f"{preset}-L2-fa.gguf")
    if not os.path.exists(path):
        llmi.write_synthetic_gguf(path, preset, seed=3, n_layer=2)
    prompt = _prompt(n_prompt, 4, 30000)
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
    m = llmi.Model(path, numerics=ASSOC[assoc][0] | llmi.NUMERICS_FA)
    assert m.prefill_supported
    a, n_pf = _run(m, prompt, 256, 4)
    assert n_pf == n_prompt - 1
    monkeypatch.setenv("LLMI_NO_PREFILL", "1")
    b, n_st = _run(m, prompt, 256, 4)
    assert n_st == 0
    _assert_steps_equal(a, b, f"{preset} {assoc}")
    m.close()


def test_fa_prefill_into_a_sequence_of_a_multi_sequence_context(gpu, tiny_models, monkeypatch):
    """A prompt sent to sequence 1 of a two-sequence context is prefilled into that
    sequence's caches: the logits of a single-sequence context given the same prompt."""
    monkeypatch.setenv("LLMI_FA_PREFILL", "1")
    monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
    prompt = _prompt(40, 8, 700)
    m = llmi.Model(tiny_models["tiny-mixed-d128"], numerics=llmi.NUMERICS_FA)
    assert m.prefill_supported
    c2 = llmi.Context(m, n_ctx=256, n_seq=2)
    assert c2.decode(prompt, seq=[1] * 40) == 0
    got = c2.logits(-1)
    assert c2.prefill_tokens == 39
    c1 = llmi.Context(m, n_ctx=256)
    assert c1.decode(prompt) == 0
    assert c1.prefill_tokens == 39
    assert np.array_equal(got, c1.logits(-1))
    monkeypatch.setenv("LLMI_NO_PREFILL", "1")
    c1.kv_clear()
    assert c1.decode(prompt) == 0
    assert c1.prefill_tokens == 39   # unchanged: this prompt ran as steps
    assert np.array_equal(got, c1.logits(-1))
    c2.close(), c1.close(), m.close()
