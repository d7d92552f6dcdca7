"""The decode-attention hooks' C surface without a GPU: llmi_attn_path (host only) returns
the path launch_attention takes, read off attn_path in csrc/attn.hip, and
llmi_battention rejects bad arguments before any device call."""
from __future__ import annotations

import ctypes as C

import llmi


def test_attention_hook_symbols_are_exported():
    L = llmi.lib()
    assert hasattr(L, "llmi_attn_path")
    assert hasattr(L, "llmi_battention")


def test_attn_path_documented_points():
    p = llmi.lib().llmi_attn_path
    # auto, 8B heads (G = 4, 8 dim slices): dim-split to 1024, split to 2048, long beyond
    assert [p(32, 8, 128, kvb, 0) for kvb in (256, 1024, 1280, 2048, 2304, 4352)] == [6, 6, 2, 2, 7, 7]
    # auto, G = 8: long-context past 1024; G = 1: as G <= 4
    assert [p(32, 4, 64, kvb, 0) for kvb in (1024, 1280)] == [6, 7]
    assert [p(8, 8, 64, kvb, 0) for kvb in (1024, 2048, 2304)] == [6, 2, 7]
    assert p(128, 16, 128, 1024, 0) == 6
    # forced modes inside their limits
    assert p(32, 8, 128, 8192, 1) == 1 and p(32, 8, 128, 8192, 2) == 2 and p(32, 8, 128, 8448, 3) == 3
    assert p(32, 8, 128, 1024, 4) == 4 and p(32, 8, 128, 512, 5) == 5 and p(32, 8, 128, 1024, 6) == 6
    assert p(32, 8, 128, 256, 7) == 7 and p(32, 8, 128, 8448, 7) == 7
    # ... and outside: split while G * kv_bound * 4 <= 128 KiB, else fused to 8192, else two-kernel
    assert p(32, 8, 128, 1280, 4) == 2 and p(32, 8, 128, 768, 5) == 2 and p(32, 8, 128, 1280, 6) == 2
    assert p(32, 4, 64, 4096, 2) == 2 and p(32, 4, 64, 4352, 2) == 1 and p(32, 4, 64, 8448, 2) == 3
    assert p(32, 8, 128, 8448, 1) == 3 and p(8, 8, 64, 8448, 1) == 2 and p(32, 8, 128, 8448, 2) == 3


def test_attn_path_rejects_bad_arguments():
    p = llmi.lib().llmi_attn_path
    assert p(32, 8, 96, 256, 0) < 0 and "llmi_attn_path" in llmi.last_error()
    assert p(30, 8, 128, 256, 0) < 0
    assert p(32, 8, 128, 0, 0) < 0
    assert p(32, 8, 128, 256, 8) < 0


def test_battention_rejects_bad_arguments():
    L = llmi.lib()

    def call(H=32, HK=8, D=128, nt=2, n_kv=(10, 200), n_ctx=256, q=1, kc=1, vc=1, out=1):
        # (pointers are never dereferenced: the checks come first)
        arr = (C.c_int32 * 8)(*n_kv) if n_kv is not None else None
        return L.llmi_battention(H, HK, D, nt, arr, n_ctx, q, kc, vc, out)

    for bad in (dict(nt=0), dict(nt=9), dict(H=30), dict(D=96), dict(n_kv=(10, 257)), dict(n_kv=(0, 5)),
                dict(n_kv=None), dict(q=None), dict(kc=None), dict(vc=None), dict(out=None), dict(n_ctx=200)):
        assert call(**bad) < 0, bad
        assert "llmi_battention" in llmi.last_error(), bad
