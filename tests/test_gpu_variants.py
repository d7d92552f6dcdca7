"""GPU parity on the GGUF shapes the loader accepts but no synthetic preset has
(tests/gguf_variants.py; tests/test_gguf_variants.py shows on the CPU that each one changes
what the oracle computes): rope_freqs.weight, a partial rotary (n_rot < head_dim, at
half the head and with only the last pair unrotated), tied embeddings of every quant type,
MHA, and Llama-3.2's combination of rope_freqs and tied embeddings.

The bar is the suite's: logits BIT-IDENTICAL to the oracle at every step, greedy ids
equal, per-op taps bit-equal (tap 2 the roped q, tap 7 the roped K row in the f16 cache),
on every path that holds its own copy of the RoPE guard or of the output-matrix pointer:
decode steps, the batched prefill (70 tokens: past the 64-token workgroup), batched decode
steps, the x86 and flash-attention numerics, and at Llama-3-8B widths the layer engine
(its early RoPE load) and the matrix-core batched matvec.

Greedy ties: files whose output matrix repeats the argmax row, so two or three logits are
bit-equal maxima; the device argmax (64 atomicMax slots) must return the first of them, as
np.argmax and upstream's strict '>' scan do, also when it feeds the token back on the
device (generate_greedy / generate_greedy_batch).
"""
from __future__ import annotations

import numpy as np
import pytest

import gguf_variants as gv
import llmi
import pyoracle as po
from helpers import Q6_K
from test_gpu_batch import _batched, _single_reference
from test_gpu_decode import run_parity
from test_gpu_taps import _check_taps, _gpu_kv_rows

pytestmark = pytest.mark.gpu

PRESETS = ("tiny-mixed", "tiny-mixed-d128")
NAMES = list(gv.VARIANTS)


def _variant(tiny_models, synth_dir, preset, name):
    return gv.VARIANTS[name](tiny_models[preset], synth_dir, gv.TINY_HEAD_DIM[preset])


def _oracle_at(path, toks, n_ctx, x86=0):
    """An oracle that has decoded toks at positions 0 .. len(toks) - 1 (taps: the last)."""
    om = po.OracleModel(path, n_ctx=n_ctx, x86=x86)
    if len(toks) > 1:
        om.prefill(toks[:-1])
    lo = om.decode(toks[-1], len(toks) - 1)
    return om, lo


# ---- decode steps ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("preset", PRESETS)
def test_variant_decode_steps(gpu, tiny_models, synth_dir, preset, name):
    """12 prompt tokens and 12 generated ones, one decode step each."""
    path = _variant(tiny_models, synth_dir, preset, name)
    rng = np.random.default_rng(2)
    prompt = [1] + [int(t) for t in rng.integers(3, 700, 11)]
    worst, g, o, margins, m, c = run_parity(path, prompt, 12, n_ctx=128, exact=True)
    assert g == o, f"greedy ids differ: gpu {g} oracle {o}"
    toks = prompt + o[:-1]  # what both sides were fed, positions 0 .. 22
    om, _ = _oracle_at(path, toks, 128)
    _check_taps(c, om, len(toks) - 1, f"{preset} {name} pos {len(toks) - 1}")
    om.close(), c.close(), m.close()


def test_partial_rotary_to_the_last_table_row(gpu, tiny_models, synth_dir):
    """n_rot = head_dim / 2 with n_ctx = 256, stepped to position 255: the last row of the
    RoPE table [n_ctx][n_rot / 2], whose stride is what a wrong d < n_rot guard gets wrong."""
    path = _variant(tiny_models, synth_dir, "tiny-mixed-d128", "nrot-half")
    rng = np.random.default_rng(3)
    prompt = [1] + [int(t) for t in rng.integers(3, 700, 11)]
    worst, g, o, margins, m, c = run_parity(path, prompt, 245, n_ctx=256, exact=True)
    assert c.n_ctx == 256 and len(prompt) + len(o) - 2 == 255  # the last step's position
    assert g == o
    toks = prompt + o[:-1]
    om, _ = _oracle_at(path, toks, 256)
    _check_taps(c, om, 255, "pos 255")
    om.close(), c.close(), m.close()


# ---- batched prefill ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("preset", PRESETS)
def test_variant_prefill(gpu, tiny_models, synth_dir, monkeypatch, preset, name):
    """A 70-token prompt in one llama_decode, then one step: logits and taps equal the
    oracle's, and the same context shape run as decode steps (LLMI_NO_PREFILL=1)."""
    path = _variant(tiny_models, synth_dir, preset, name)
    rng = np.random.default_rng(11)
    prompt = [1] + [int(t) for t in rng.integers(3, 700, 69)]
    om, lo = _oracle_at(path, prompt, 128)
    got = {}
    for no_pf in (False, True):
        if no_pf:
            monkeypatch.setenv("LLMI_NO_PREFILL", "1")
        else:
            monkeypatch.delenv("LLMI_NO_PREFILL", raising=False)
        m = llmi.Model(path)
        c = llmi.Context(m, n_ctx=128)
        assert c.decode(prompt) == 0
        if no_pf:
            assert c.prefill_tokens == 0
        else:
            assert m.prefill_supported, "every tiny variant is a shape the prefill takes"
            assert c.prefill_tokens > 0, "the prompt did not take the batched prefill"
        lg = c.logits(-1)
        assert np.array_equal(lg, lo), f"no_prefill={no_pf}: prompt logits, max |d| {np.abs(lg - lo).max():.3g}"
        if not no_pf:
            _check_taps(c, om, 69, f"{preset} {name} after the prefill")
            # K rows the prefill's own RoPE epilogue wrote, in both 64-token workgroups
            HK, D = om.n_head_kv, om.head_dim
            gk, ok = c.tap(7, HK * c.n_ctx * D), om.tap(7).reshape(om.n_ctx, HK * D)
            for pos in (0, 1, 63, 64, 68):
                assert np.array_equal(_gpu_kv_rows(gk, HK, c.n_ctx, D, pos, False), ok[pos]), f"prefilled K row {pos}"
        nxt = c.greedy(-1)
        assert nxt == int(np.argmax(lo))
        assert c.decode([nxt], pos=[70]) == 0
        got[no_pf] = (lg, c.logits(-1), c, m)
    lo1 = om.decode(int(np.argmax(lo)), 70)
    for no_pf, (_, lg1, c, m) in got.items():
        assert np.array_equal(lg1, lo1), f"no_prefill={no_pf}: step after the prompt, max |d| {np.abs(lg1 - lo1).max():.3g}"
        _check_taps(c, om, 70, f"{preset} {name} no_prefill={no_pf} pos 70")
        c.close(), m.close()
    om.close()


# ---- batched decode steps ----------------------------------------------------------------------
def _oracle_greedy(path, prompt, n_gen, n_ctx, x86=0):
    """[first] + n_gen greedy ids after the prompt, the oracle stepped with np.argmax."""
    om, lo = _oracle_at(path, prompt, n_ctx, x86)
    ids = [int(np.argmax(lo))]
    for k in range(n_gen):
        ids.append(int(np.argmax(om.decode(ids[-1], len(prompt) + k))))
    om.close()
    return ids


@pytest.mark.parametrize("name", NAMES)
def test_variant_batched_steps(gpu, tiny_models, synth_dir, name):
    """Three sequences at different positions through generate_greedy_batch (which refuses
    a model it cannot batch, tests/test_gpu_batch.py test_mixed_gate_up_types_fall_back: a
    result means every step was a batched one).  Base: tiny-mixed-d128 (tiny-mixed's
    layer 0 mixes gate / up types and never batches)."""
    path = _variant(tiny_models, synth_dir, "tiny-mixed-d128", name)
    rng = np.random.default_rng(13)
    prompts = [[1] + [int(t) for t in rng.integers(3, 700, n - 1)] for n in (5, 17, 30)]
    want, want_lg = _single_reference(path, prompts, 8, 256)
    got, got_lg, c = _batched(path, prompts, 8, 256, n_seq=3)
    for s, p in enumerate(prompts):
        assert np.array_equal(got_lg[s], want_lg[s]), f"seq {s}: prompt logits differ"
        assert got[s] == want[s], f"seq {s}: batched {got[s]} single {want[s]}"
        ora = _oracle_greedy(path, p, 8, 256)
        assert got[s] == ora, f"seq {s}: batched {got[s]} oracle {ora}"
    c.close()


# ---- x86 and flash-attention numerics ----------------------------------------------------------
NUMERICS = {"x86": (llmi.NUMERICS_X86, po.X86_ALL), "fa": (llmi.NUMERICS_FA, po.X86_FA)}


@pytest.mark.parametrize("mode", list(NUMERICS))
@pytest.mark.parametrize("name", ["ropefreqs", "nrot-half", "tied-q6_K"])
@pytest.mark.parametrize("preset", PRESETS)
def test_variant_numerics(gpu, tiny_models, synth_dir, preset, name, mode):
    """20 steps in the x86 association (oracle: X86_ALL) and the flash-attention numerics
    (oracle: X86_FA), which have their own matvec and attention kernels."""
    num, flags = NUMERICS[mode]
    path = _variant(tiny_models, synth_dir, preset, name)
    m = llmi.Model(path, numerics=num)
    assert m.numerics == num
    c = llmi.Context(m, n_ctx=64)
    om = po.OracleModel(path, n_ctx=64, x86=flags)
    t = 1
    for pos in range(20):
        assert c.decode([t], pos=[pos]) == 0
        lg, lo = c.logits(-1), om.decode(t, pos)
        assert np.array_equal(lg, lo), f"pos {pos}: max |d| {np.abs(lg - lo).max():.3g}"
        t = int(np.argmax(lo))
        assert c.greedy(-1) == t
    om.close(), c.close(), m.close()


# ---- Llama-3-8B widths: the layer engine and the matrix-core batched matvec --------------------
WIDE = {
    # n_rot 64 of head_dim 128 with the 32 factors it needs
    "nrot64-ropefreqs": lambda b, o: gv.nrot_ropefreqs(b, o, 64),
    "llama32like": lambda b, o: gv.llama32like(b, o, Q6_K),
}


@pytest.fixture(scope="module")
def wide_base(synth_dir):
    path = str(synth_dir / "llama3-8b-q4km-L2-v32000-variants.gguf")
    llmi.write_synthetic_gguf(path, "llama3-8b-q4km", seed=5, n_layer=2, n_vocab=32000)
    return path


@pytest.mark.parametrize("name", list(WIDE))
def test_variant_engine_real_widths(gpu, synth_dir, wide_base, name):
    """Engine on: a 6-token prompt and 6 generated tokens bit-identical to the oracle, one
    'layer' launch per layer; engine off: the same tokens and final logits."""
    path = WIDE[name](wide_base, synth_dir)
    prompt = [1, 100, 2000, 31000, 7, 9]
    res = {}
    for on in (1, 0):
        old = llmi.test_option("engine", on)
        try:
            if on:
                worst, g, o, margins, m, c = run_parity(path, prompt, 6, n_ctx=64, exact=True)
                assert g == o
                toks = prompt + o[:-1]  # what both sides were fed, positions 0 .. 10
            else:
                m = llmi.Model(path)
                c = llmi.Context(m, n_ctx=64)
                g = []
                for pos, t in enumerate(toks):
                    assert c.decode([t], pos=[pos]) == 0
                    if pos >= len(prompt) - 1:
                        g.append(c.greedy(-1))
            res[on] = (g, c.logits(-1).copy())
            launches = c.profile_kernels(g[-1], len(toks), 1)["layer"]["launches_per_step"]
            assert launches == (m.n_layer if on else 0), f"engine {on}: {launches} layer launches"
            c.close(), m.close()
        finally:
            llmi.test_option("engine", old)
    assert res[1][0] == res[0][0], "engine tokens differ from separate launches"
    assert np.array_equal(res[1][1], res[0][1]), "engine logits differ from separate launches"


@pytest.mark.parametrize("name", list(WIDE))
def test_variant_bmm_real_widths(gpu, synth_dir, wide_base, monkeypatch, name):
    """Three sequences in batched steps at widths the matrix-core batched matvec takes
    (K-quants at steps of LLMI_BMM_MIN tokens or more: 3 by default, set to 1 as
    test_bmm_any_batch_size sets it, so a change of the default cannot move this test to
    k_mvn): each equals its single-sequence decode and the oracle's greedy ids.  (The
    library counts no launches of the batched kernels: which one ran is the launcher's
    documented choice, not an assertion here.)"""
    monkeypatch.setenv("LLMI_BMM_MIN", "1")
    path = WIDE[name](wide_base, synth_dir)
    rng = np.random.default_rng(8)
    prompts = [[1] + [int(t) for t in rng.integers(3, 30000, n - 1)] for n in (4, 9, 14)]
    want, want_lg = _single_reference(path, prompts, 6, 256)
    got, got_lg, c = _batched(path, prompts, 6, 256, n_seq=3)
    for s, p in enumerate(prompts):
        assert np.array_equal(got_lg[s], want_lg[s]), f"seq {s}: prompt logits differ"
        assert got[s] == want[s], f"seq {s}"
        ora = _oracle_greedy(path, p, 6, 64)
        assert got[s] == ora, f"seq {s}: batched {got[s]} oracle {ora}"
    c.close()


# ---- greedy ties -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", gv.TIE_SETS)
@pytest.mark.parametrize("tied", [False, True], ids=["separate", "tied"])
def test_greedy_ties_first_max_wins(gpu, tiny_models, synth_dir, tied, kind):
    base = tiny_models["tiny-mixed-d128"]
    if tied:
        base = gv.tied(base, synth_dir, Q6_K)
    path, rows = gv.tie_file(base, synth_dir, kind)
    prompt, n_gen = gv.TIE_PROMPT, 8
    want = _oracle_greedy(path, prompt, n_gen, 64)
    assert want[0] == min(rows)
    m = llmi.Model(path)
    # decode steps, then the prompt prefilled: the host sees the tie, the device picks the first
    for prefilled in (False, True):
        c = llmi.Context(m, n_ctx=64)
        if prefilled:
            assert c.decode(prompt) == 0
            assert c.prefill_tokens > 0
        else:
            for pos, t in enumerate(prompt):
                assert c.decode([t], pos=[pos]) == 0
        lg = c.logits(-1)
        assert np.all(lg[rows].view(np.uint32) == lg[rows].view(np.uint32)[0]) and lg[rows[0]] == lg.max()
        assert int(np.argmax(lg)) == min(rows)
        assert c.greedy(-1) == min(rows), f"prefilled={prefilled}: device argmax took {c.greedy(-1)} of the tie {rows}"
        # the continuation from the chosen token
        assert c.generate_greedy(min(rows), len(prompt), n_gen) == want[1:]
        c.close()
    # the tie broken on the device and fed back through k_embed: the step at the prompt's
    # last token is generate_greedy's first
    c = llmi.Context(m, n_ctx=64)
    assert c.decode(prompt[:-1]) == 0
    assert c.generate_greedy(prompt[-1], len(prompt) - 1, n_gen + 1) == want
    c.close()
    # the same in a batched step (per-sequence StepState slots), beside another sequence
    other = [1, 300, 12, 650, 88]
    want_other = _oracle_greedy(path, other, n_gen, 64)
    c = llmi.Context(m, n_ctx=64, n_seq=2)
    assert c.decode(other[:-1], seq=[0] * (len(other) - 1)) == 0
    assert c.decode(prompt[:-1], seq=[1] * (len(prompt) - 1)) == 0
    got = c.generate_greedy_batch([0, 1], [other[-1], prompt[-1]], [len(other) - 1, len(prompt) - 1], n_gen + 1)
    assert got[1] == want, f"batched: {got[1]} oracle {want}"
    assert got[0] == want_other
    c.close(), m.close()
