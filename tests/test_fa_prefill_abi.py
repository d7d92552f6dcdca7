"""The flash-attention prefill's C surface without a GPU: llmi_pf_attention_fa and
llmi_prefill_token_count are exported, and llmi_pf_attention_fa rejects bad arguments
before any device call (so these run on a machine with no GPU)."""
from __future__ import annotations

import llmi


def test_fa_prefill_symbols_are_exported():
    L = llmi.lib()
    assert hasattr(L, "llmi_pf_attention_fa")
    assert hasattr(L, "llmi_prefill_token_count")
    assert L.llmi_prefill_token_count(None) == 0


def test_pf_attention_fa_rejects_bad_arguments():
    L = llmi.lib()
    # (pointers are never dereferenced: the checks come first)
    assert L.llmi_pf_attention_fa(32, 8, 96, 16, 0, 256, 1, 1, 1, 1) < 0      # head_dim
    assert "llmi_pf_attention_fa" in llmi.last_error()
    assert L.llmi_pf_attention_fa(32, 8, 128, 16, 250, 256, 1, 1, 1, 1) < 0   # pos0 + T > n_ctx
    assert "llmi_pf_attention_fa" in llmi.last_error()
    assert L.llmi_pf_attention_fa(32, 8, 128, 16, 0, 256, None, 1, 1, 1) < 0  # null q
    assert L.llmi_pf_attention_fa(32, 8, 128, 16, 0, 256, 1, 1, 1, None) < 0  # null out
    assert L.llmi_pf_attention_fa(30, 8, 128, 16, 0, 256, 1, 1, 1, 1) < 0     # heads not a multiple of KV heads
    assert L.llmi_pf_attention_fa(32, 8, 128, 0, 0, 256, 1, 1, 1, 1) < 0      # no tokens
