"""llama_model_get_vocab's handle lives exactly as long as its model (include/llmi.h,
INTEGRATION.md): it is a member of the model, so it never outlives it into the next model
allocated at the same address, and it does not depend on the thread that asked for it.
CPU only (vocab_only models); raw ctypes where the Python wrapper would hide the handle."""
from __future__ import annotations

import ctypes as C
import threading

import pytest

import llmi
from llmi._lib import lib

N_VOCAB_A, N_VOCAB_B = 1000, 777


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("vocab_lifetime")
    out = {}
    for name, nv in (("a", N_VOCAB_A), ("b", N_VOCAB_B)):
        out[name] = str(d / f"{name}.gguf")
        llmi.write_synthetic_gguf(out[name], "tiny-mixed", seed=1, n_layer=1, n_vocab=nv)
    return out


def _load(path: str):
    L = lib()
    p = L.llama_model_default_params()
    p.vocab_only = True
    h = L.llama_model_load_from_file(path.encode(), p)
    assert h, L.llmi_last_error()
    return h


def _tokenize(v, text: bytes) -> list[int]:
    buf = (C.c_int32 * 64)()
    n = lib().llama_tokenize(v, text, len(text), buf, 64, True, True)
    assert n >= 0
    return list(buf[:n])


def _read(v) -> tuple:
    L = lib()
    return (L.llama_vocab_n_tokens(v), L.llama_vocab_bos(v), L.llama_vocab_eos(v), L.llama_vocab_get_text(v, 51),
            _tokenize(v, b" w51 w7 hello"))


def _on_thread(fn):
    out = []
    t = threading.Thread(target=lambda: out.append(fn()))
    t.start()
    t.join()
    assert len(out) == 1, "the thread raised"
    return out[0]


def test_reuse(paths):
    """A model freed and the next one loaded (often at the same address): the new model's
    handle reads the new model's tokenizer, every time."""
    L = lib()
    texts = []
    for _ in range(40):
        h = _load(paths["a"])
        texts.append(L.llama_vocab_get_text(L.llama_model_get_vocab(h), 51))
        L.llama_model_free(h)
    assert texts == [b" w51"] * 40


def test_interleaved(paths):
    L = lib()
    a = _load(paths["a"])
    va = L.llama_model_get_vocab(a)
    assert L.llama_vocab_n_tokens(va) == N_VOCAB_A
    for _ in range(40):
        b = _load(paths["b"])
        vb = L.llama_model_get_vocab(b)
        assert vb != va
        assert L.llama_vocab_n_tokens(vb) == N_VOCAB_B
        assert L.llama_vocab_get_text(vb, 51) == b" w51"
        L.llama_model_free(b)
        assert L.llama_vocab_n_tokens(va) == N_VOCAB_A
        assert L.llama_vocab_get_text(va, 51) == b" w51"
        assert L.llama_vocab_get_text(va, N_VOCAB_A - 1) == f" w{N_VOCAB_A - 1}".encode()
    L.llama_model_free(a)


def test_thread_exit(paths):
    """A handle taken on a thread that has exited (the server's loader thread) serves the
    main thread, and one taken on the main thread serves a short-lived thread."""
    L = lib()

    def load_and_take():
        h = _load(paths["a"])
        return h, L.llama_model_get_vocab(h)

    h, v = _on_thread(load_and_take)
    fresh_model = _load(paths["a"])
    want = _read(L.llama_model_get_vocab(fresh_model))
    assert want[0] == N_VOCAB_A and want[3] == b" w51" and len(want[4]) > 0
    assert _read(v) == want
    L.llama_model_free(h)

    v_main = L.llama_model_get_vocab(fresh_model)
    assert _on_thread(lambda: _read(v_main)) == want
    L.llama_model_free(fresh_model)


def test_stable_handle(paths):
    L = lib()
    h = _load(paths["a"])
    v = L.llama_model_get_vocab(h)
    assert v and L.llama_model_get_vocab(h) == v
    assert _on_thread(lambda: L.llama_model_get_vocab(h)) == v
    before = _read(v)
    L.llmi_vocab_free(v)  # a model-owned handle: no-op
    assert L.llama_model_get_vocab(h) == v and _read(v) == before
    L.llama_model_free(h)
