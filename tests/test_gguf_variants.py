"""The GGUF variants of tests/gguf_variants.py are what they claim (CPU), so the GPU parity
on them (tests/test_gpu_variants.py) cannot be vacuous:

- an identity rewrite is byte-identical, and every variant re-read by the independent
  reader differs from its base in exactly the intended KVs and tensors;
- the oracle loads every variant and reports the intended n_rot / n_head_kv / n_vocab;
- every variant is live in the oracle: rope_freqs and a partial rotary leave position 0
  bit-equal (every angle is 0) and change every later position; tying changes the logits
  and nothing before the output head; MHA changes the logits;
- the tie files tie: the oracle's logits at the tie set are bit-equal and the maximum;
- the loader refuses what it does not implement, naming the key or tensor, before any
  device call (vocab_only), and loads a good model afterwards.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import gguf_variants as gv
import llmi
import pyoracle as po
from gguf_reader import read_gguf
from helpers import F16, F32, Q4_K, Q5_K, Q6_K, Q8_0, QTYPES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny-mixed.gguf")
PRESETS = ("tiny-mixed", "tiny-mixed-d128")
N_VOCAB = {"tiny-mixed": 1000, "tiny-mixed-d128": 777}  # d128: odd, a single-row last LOGITS pair
TOKS = [1, 42, 7, 300, 555, 19]


def test_identity_rewrite_is_byte_identical(synth_dir):
    out = gv.identity(GOLDEN, synth_dir)
    assert open(out, "rb").read() == open(GOLDEN, "rb").read()


def test_identity_rewrite_of_every_preset_shape(tiny_models, synth_dir):
    for preset in PRESETS:
        out = gv.identity(tiny_models[preset], synth_dir)
        assert open(out, "rb").read() == open(tiny_models[preset], "rb").read()


@pytest.mark.parametrize("n", [16, 31, 32, 63, 64])
def test_rope_factors(n):
    """1.0 and 8.0 are there, and at least four values strictly between, none of them a
    power of two (theta / ff rounds); non-decreasing like Llama-3.1's."""
    ff = gv.rope_factors(n)
    assert ff.dtype == np.float32 and ff.shape == (n,)
    assert ff[0] == 1.0 and ff[-1] == 8.0 and np.all(np.diff(ff) >= 0)
    mid = ff[(ff > 1.0) & (ff < 8.0)]
    assert mid.size >= 4
    assert not np.any(np.log2(mid.astype(np.float64)) == np.round(np.log2(mid.astype(np.float64))))


# ---- exactly the intended changes -----------------------------------------------------------
def _diff(base: str, var: str):
    """(changed or added KVs, dropped KVs, added / dropped / changed tensors by name)."""
    b, v = read_gguf(base), read_gguf(var)
    assert (v["version"], v["alignment"]) == (b["version"], b["alignment"])
    kv = {k: x for k, x in v["kv"].items() if k not in b["kv"] or b["kv"][k] != x}
    kv_gone = set(b["kv"]) - set(v["kv"])
    bt, vt = {t["name"]: t for t in b["tensors"]}, {t["name"]: t for t in v["tensors"]}
    assert len(vt) == len(v["tensors"])
    end = 0
    for t in v["tensors"]:  # the layout rules of test_gguf_format.py
        assert t["offset"] % v["alignment"] == 0 and t["offset"] >= end and len(t["data"]) == t["nbytes"]
        end = t["offset"] + t["nbytes"]
    assert v["data_start"] + (end + v["alignment"] - 1) // v["alignment"] * v["alignment"] == v["file_size"]
    changed = {n for n in set(bt) & set(vt)
               if (bt[n]["ne"], bt[n]["type"], bt[n]["data"]) != (vt[n]["ne"], vt[n]["type"], vt[n]["data"])}
    return kv, kv_gone, set(vt) - set(bt), set(bt) - set(vt), changed, bt, vt


def _expect(name: str, base: str):
    """What variant `name` of `base` changes: (KVs, tensors added, dropped, changed)."""
    kvb = read_gguf(base)["kv"]
    D = kvb["llama.embedding_length"] // kvb["llama.attention.head_count"]
    L = kvb["llama.block_count"]
    kv, add, drop, chg = {}, set(), set(), set()
    if name in ("ropefreqs", "llama32like"):
        add.add("rope_freqs.weight")
    if name.startswith("nrot"):
        kv["llama.rope.dimension_count"] = D // 2 if name == "nrot-half" else D - 2
    if name.startswith("tied") or name == "llama32like":
        drop.add("output.weight")
        chg.add("token_embd.weight")
    if name == "mha":
        kv["llama.attention.head_count_kv"] = kvb["llama.attention.head_count"]
        chg |= {f"blk.{l}.attn_{x}.weight" for l in range(L) for x in "kv"}
    return kv, add, drop, chg


TIED_TYPE = {"tied-q4_K": Q4_K, "tied-q5_K": Q5_K, "tied-q6_K": Q6_K, "tied-q8_0": Q8_0, "llama32like": Q6_K}


@pytest.mark.parametrize("name", list(gv.VARIANTS))
@pytest.mark.parametrize("preset", PRESETS)
def test_variant_changes_exactly_what_it_names(tiny_models, synth_dir, preset, name):
    base = tiny_models[preset]
    D = gv.TINY_HEAD_DIM[preset]
    var = gv.VARIANTS[name](base, synth_dir, D)
    kv, kv_gone, added, dropped, changed, bt, vt = _diff(base, var)
    want_kv, want_add, want_drop, want_chg = _expect(name, base)
    assert (kv, kv_gone, added, dropped, changed) == (want_kv, set(), want_add, want_drop, want_chg)
    E, V = bt["token_embd.weight"]["ne"]
    assert V == N_VOCAB[preset], "the preset's vocabulary is kept"
    if "rope_freqs.weight" in added:
        t = vt["rope_freqs.weight"]
        assert (t["ne"], t["type"]) == ([D // 2], F32)
        assert np.array_equal(np.frombuffer(t["data"], np.float32), gv.rope_factors(D // 2))
    if "token_embd.weight" in changed:
        t = vt["token_embd.weight"]
        assert (t["ne"], t["type"]) == ([E, V], TIED_TYPE[name])
    if name == "mha":
        for n in changed:
            assert (vt[n]["ne"], vt[n]["type"]) == ([E, E], bt[n]["type"]), n


# ---- the oracle loads them, and they are live ------------------------------------------------
def _oracle_run(path, toks=TOKS, taps=()):
    """Per position: the oracle's logits, and the taps of `taps` after that step."""
    om = po.OracleModel(path, n_ctx=64)
    out, tp = [], []
    for pos, t in enumerate(toks):
        out.append(om.decode(t, pos))
        tp.append([om.tap(k) for k in taps])
    info = (om.n_rot, om.n_head_kv, om.n_vocab, om.n_head, om.head_dim)
    om.close()
    return out, tp, info


@pytest.fixture(scope="module")
def base_runs(tiny_models):
    return {p: _oracle_run(tiny_models[p]) for p in PRESETS}


@pytest.mark.parametrize("name", list(gv.VARIANTS))
@pytest.mark.parametrize("preset", PRESETS)
def test_oracle_loads_variant_and_it_is_live(tiny_models, synth_dir, base_runs, preset, name):
    base = tiny_models[preset]
    D = gv.TINY_HEAD_DIM[preset]
    var = gv.VARIANTS[name](base, synth_dir, D)
    base_lg, _, (b_rot, b_hkv, b_voc, H, b_D) = base_runs[preset]
    assert (b_rot, b_D, b_voc) == (D, D, N_VOCAB[preset])
    lg, _, (n_rot, n_head_kv, n_vocab, _, head_dim) = _oracle_run(var)
    want_kv, *_ = _expect(name, base)
    assert n_rot == want_kv.get("llama.rope.dimension_count", D)
    assert n_head_kv == (H if name == "mha" else b_hkv)
    assert (n_vocab, head_dim) == (N_VOCAB[preset], D)
    same = [np.array_equal(a, b) for a, b in zip(lg, base_lg)]
    if name in ("ropefreqs", "nrot-half", "nrot-last-pair"):
        assert same[0], "position 0 rotates by angle 0 whatever the frequencies"
        assert not any(same[1:]), f"positions equal to the base: {same}"
    else:
        assert not any(same), f"positions equal to the base: {same}"


@pytest.mark.parametrize("qtype", QTYPES)
@pytest.mark.parametrize("preset", PRESETS)
def test_tied_changes_only_the_output_head(tiny_models, synth_dir, preset, qtype):
    """tied(T) against the same token_embd with the base's output.weight kept: the
    residual stream, roped q, attention and SwiGLU outputs (taps 1-4) are bit-equal at
    every step, the logits differ."""
    base = tiny_models[preset]
    lg_t, tp_t, _ = _oracle_run(gv.tied(base, synth_dir, qtype), taps=(1, 2, 3, 4))
    lg_e, tp_e, _ = _oracle_run(gv.embd_only(base, synth_dir, qtype), taps=(1, 2, 3, 4))
    for pos in range(len(TOKS)):
        for a, b in zip(tp_t[pos], tp_e[pos]):
            assert np.array_equal(a, b), pos
        assert not np.array_equal(lg_t[pos], lg_e[pos]), pos


# ---- greedy ties ------------------------------------------------------------------------------
def tie_base(tiny_models, synth_dir, tied: bool) -> str:
    base = tiny_models["tiny-mixed-d128"]
    return gv.tied(base, synth_dir, Q6_K) if tied else base


@pytest.mark.parametrize("kind", gv.TIE_SETS)
@pytest.mark.parametrize("tied", [False, True], ids=["separate", "tied"])
def test_tie_files_tie_in_the_oracle(tiny_models, synth_dir, tied, kind):
    base = tie_base(tiny_models, synth_dir, tied)
    path, rows = gv.tie_file(base, synth_dir, kind)
    r = gv.oracle_argmax(base, gv.TIE_PROMPT)
    assert r in rows
    if kind == "pair":
        assert rows[0] % 2 == 0 and rows[1] == rows[0] + 1
    elif kind == "spread":
        assert len(rows) == 3 and rows[0] < 64 and rows[-1] > 777 // 2
    else:
        assert rows[-1] == 776
    # only the output matrix changed, and only the copied rows of it
    kv, kv_gone, added, dropped, changed, bt, vt = _diff(base, path)
    name = "token_embd.weight" if tied else "output.weight"
    assert (kv, kv_gone, added, dropped, changed) == ({}, set(), set(), set(), {name})
    rb = len(bt[name]["data"]) // 777
    b = np.frombuffer(bt[name]["data"], np.uint8).reshape(777, rb)
    v = np.frombuffer(vt[name]["data"], np.uint8).reshape(777, rb)
    assert set(np.flatnonzero((b != v).any(axis=1))) == set(rows) - {r}
    assert all(np.array_equal(v[x], b[r]) for x in rows)
    om = po.OracleModel(path, n_ctx=64)
    for pos, t in enumerate(gv.TIE_PROMPT):
        lo = om.decode(t, pos)
    om.close()
    at = lo[rows]
    assert np.all(at.view(np.uint32) == at.view(np.uint32)[0]), "the tie set's logits are not bit-equal"
    assert at[0] == lo.max() and set(np.flatnonzero(lo == lo.max())) == set(rows)
    assert int(np.argmax(lo)) == min(rows)


# ---- loader rejections (vocab_only: model_load checks everything before any device call) ----
def _rope_freqs(n, type_):
    data = gv.rope_factors(max(n, 4))[:n].astype(np.float32 if type_ == F32 else np.float16).tobytes()
    return lambda g: g.add_tensor("rope_freqs.weight", [n], type_, data)


def _embd_f16(g):
    cols, rows = g.tensor("token_embd.weight").ne
    w = (np.random.default_rng(3).standard_normal(rows * cols) * 0.02).astype(np.float16)
    g.replace_tensor("token_embd.weight", [cols, rows], F16, w.tobytes())


def _scaling(type_, factor):
    def edit(g):
        if type_ is not None:
            g.set_kv("llama.rope.scaling.type", gv.STR, type_)
        if factor is not None:
            g.set_kv("llama.rope.scaling.factor", gv.F32_KV, factor)
    return edit


# tiny-mixed: head_dim 64, n_rot 64
REJECTED = {
    "rope_freqs-too-short": (_rope_freqs(31, F32), "rope_freqs.weight"),
    "rope_freqs-f16": (_rope_freqs(32, F16), "rope_freqs.weight"),
    "n_rot-odd": (lambda g: gv.edit_nrot(g, 31), "rope.dimension_count"),
    "n_rot-above-head_dim": (lambda g: gv.edit_nrot(g, 66), "rope.dimension_count"),
    "n_rot-zero": (lambda g: gv.edit_nrot(g, 0), "rope.dimension_count"),
    "token_embd-f16": (_embd_f16, "token_embd"),
    "scaling-linear-4": (_scaling("linear", 4.0), "llama.rope.scaling.type"),
    "scaling-yarn-4": (_scaling("yarn", 4.0), "llama.rope.scaling.type"),
    "scaling-factor-4-alone": (_scaling(None, 4.0), "llama.rope.scaling.factor"),
    "scaling-none-factor-4": (_scaling("none", 4.0), "llama.rope.scaling.factor"),
}


@pytest.mark.parametrize("case", list(REJECTED))
def test_loader_rejects(tiny_models, synth_dir, case):
    edit, names = REJECTED[case]
    good = tiny_models["tiny-mixed"]
    bad = gv._variant(good, synth_dir, "bad-" + case, edit)
    assert read_gguf(bad)["kv"]["general.architecture"] == "llama"  # a well-formed file
    with pytest.raises(llmi.LlmiError, match=names.replace(".", r"\.")):
        llmi.Model(bad, vocab_only=True)
    llmi.Model(good, vocab_only=True).close()


def test_loader_accepts_unscaled_rope_keys(tiny_models, synth_dir):
    """scaling.type "none" and factor 1 say what the loader does: they load."""
    ok = gv._variant(tiny_models["tiny-mixed"], synth_dir, "scaling-none-1", _scaling("none", 1.0))
    llmi.Model(ok, vocab_only=True).close()
    for name in gv.VARIANTS:
        llmi.Model(gv.VARIANTS[name](tiny_models["tiny-mixed"], synth_dir, 64), vocab_only=True).close()
