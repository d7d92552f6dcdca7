"""Q2_K on the host: the synthetic writer's Q2_K table and blocks, and the device layout's size."""
from __future__ import annotations

import numpy as np

import gguf_reader as gr
import llmi
from q2k_cases import Q2_K, dequant_f64

Q3_K, Q6_K = 11, 14
for _t, _v in ((Q2_K, ("Q2_K", 256, 84)), (Q3_K, ("Q3_K", 256, 110))):  # gguf_reader.py predates both types
    gr.GGML_TYPES.setdefault(_t, _v)


def test_writer_q2k_table_blocks_and_layout_bytes(synth_dir):
    path = str(synth_dir / "tiny-q2k-2.gguf")
    assert llmi.write_synthetic_gguf(path, "tiny-q2k", seed=2, n_layer=2) > 0
    g = gr.read_gguf(path)
    assert g["kv"]["general.file_type"] == 10
    tensors = {t["name"]: t for t in g["tensors"]}
    for l in range(2):
        got = [tensors[f"blk.{l}.{k}.weight"]["type"] for k in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")]
        assert got == [Q2_K, Q2_K, Q3_K, Q3_K, Q2_K, Q2_K, Q3_K], (l, got)
    emb = tensors["token_embd.weight"]
    assert emb["type"] == Q2_K and tensors["output.weight"]["type"] == Q6_K
    assert emb["nbytes"] == 777 * (512 // 256) * 84
    # the device planes hold GGUF's bytes (64 + 16 + 4 per block; whole 256-B plane lines here)
    assert llmi._lib.lib().llmi_device_layout_bytes(Q2_K, 64, 512) == 64 * 2 * 84
    m = llmi.Model(path, vocab_only=True)
    assert "ftype 10" in m.desc and m.size == sum(t["nbytes"] for t in g["tensors"])
    m.close()
    # the synthetic blocks' calibration: weights of mean ~0 and std ~0.02
    w = dequant_f64(np.frombuffer(bytes(emb["data"]), dtype=np.uint8))
    assert abs(w.mean()) < 1e-3 and 0.018 < w.std() < 0.022, (w.mean(), w.std())
