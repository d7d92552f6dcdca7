"""Q3_K on the host: the loader's arena plan and the synthetic writer's Q3_K_M table."""
from __future__ import annotations

import gguf_reader as gr
import llmi
from q3k_cases import Q3_K

Q4_K, Q5_K, Q6_K = 12, 13, 14
gr.GGML_TYPES.setdefault(Q3_K, ("Q3_K", 256, 110))  # gguf_reader.py predates Q3_K and may not be edited


def _q3km(synth_dir, n_layer=4):
    path = str(synth_dir / f"tiny-q3km-{n_layer}.gguf")
    assert llmi.write_synthetic_gguf(path, "tiny-q3km", seed=2, n_layer=n_layer) > 0
    return path


def test_writer_q3km_table(synth_dir):
    g = gr.read_gguf(_q3km(synth_dir))
    assert g["kv"]["general.file_type"] == 12
    types = {t["name"]: t["type"] for t in g["tensors"]}
    for l in range(4):
        got = [types[f"blk.{l}.{k}.weight"] for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")]
        assert got == [Q3_K, Q3_K, Q5_K if l < 2 else Q4_K, Q4_K, Q3_K, Q3_K, Q5_K if l < 1 else Q4_K], (l, got)
    assert types["token_embd.weight"] == Q3_K and types["output.weight"] == Q6_K


def test_vocab_only_load_plans_the_files_bytes(synth_dir):
    path = _q3km(synth_dir)
    m = llmi.Model(path, vocab_only=True)
    assert "ftype 12" in m.desc
    assert m.size == sum(t["nbytes"] for t in gr.read_gguf(path)["tensors"])
    m.close()
