"""The batched-prefill attention hooks' C surface without a GPU: llmi_pf_attn_path and
llmi_pf_attention reject bad arguments before any device call (the path itself depends on
the compiled kernels' static LDS and is asserted on the device,
tests/test_gpu_pf_attention_edges.py)."""
from __future__ import annotations

import llmi


def test_pf_attn_path_symbol_is_exported():
    assert hasattr(llmi.lib(), "llmi_pf_attn_path")


def test_pf_attn_path_rejects_bad_arguments():
    p = llmi.lib().llmi_pf_attn_path
    for bad in ((32, 8, 96, 256, 1),      # head_dim
                (30, 8, 128, 256, 1),     # n_head not a multiple of n_head_kv
                (0, 8, 128, 256, 1), (32, 0, 128, 256, 1),
                (32, 8, 128, 0, 1), (32, 8, 128, -5, 1),   # max_kv
                (32, 8, 128, 256, 0),     # mode 0 is the tiled kernel: no LDS ladder
                (32, 8, 128, 256, 3), (32, 8, 128, 256, -1)):
        assert p(*bad) == -2, bad
        assert "llmi_pf_attn_path" in llmi.last_error(), bad


def test_pf_attention_length_limits_by_mode():
    """Mode 0 takes pos0 + T up to n_ctx (what the engine does wherever k_pf_fa's scratch
    exists); modes 1 and 2 end at 32768 positions.  Only refusals can be asked for here:
    the accepted side launches (tests/test_gpu_pf_attention_edges.py)."""
    L = llmi.lib()
    n_ctx = 33280
    for mode in (1, 2):
        assert L.llmi_pf_attention(8, 1, 128, 9, 32768 - 8, n_ctx, 1, 1, 1, 1, mode, 0) == -1, mode
        assert "bad arguments" in llmi.last_error()
    for mode in (0, 1, 2):
        assert L.llmi_pf_attention(8, 1, 128, 9, n_ctx - 8, n_ctx, 1, 1, 1, 1, mode, 0) == -1, mode  # past n_ctx
        assert L.llmi_pf_attention(8, 1, 128, 0, 0, n_ctx, 1, 1, 1, 1, mode, 0) == -1, mode
        assert L.llmi_pf_attention(8, 1, 128, 4, 0, 300, 1, 1, 1, 1, mode, 0) == -1, mode           # n_ctx % 256
        assert L.llmi_pf_attention(8, 1, 128, 4, 0, 256, None, 1, 1, 1, mode, 0) == -1, mode
    assert L.llmi_pf_attention(8, 1, 128, 4, 0, 256, 1, 1, 1, 1, 3, 0) == -1
    assert L.llmi_pf_attention(6, 2, 128, 4, 0, 256, 1, 1, 1, 1, 0, 0) == -1   # G = 3: no tiled kernel
    assert "no tiled kernel" in llmi.last_error()
