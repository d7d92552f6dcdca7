"""llmi — MI355X-native GGUF decode path (Python host side over the libllmi.so C ABI).

Mirrors the llama.cpp decode surface the reference's llama-server drives
(SURVEY.md §8b): a Model is `llama_model_load_from_file`, a Context is
`llama_init_from_model`, `Context.decode` is `llama_decode` with the same return
codes, `Context.logits` is `llama_get_logits_ith`.  All compute runs in the HIP
library; nothing here computes numerics.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._lib import LlmiLibraryError, last_error, lib, llama_context_params, llama_model_params  # noqa: F401
from ._lib import (POOLING_CLS, POOLING_LAST, POOLING_MEAN, POOLING_NONE, POOLING_RANK,  # noqa: F401
                   POOLING_UNSPECIFIED)

# ggml type ids
F32, F16, Q8_0, Q4_K, Q5_K, Q6_K, Q8_K = 0, 1, 8, 12, 13, 14, 15
# model numerics (llama_model_params.numerics): ggml's generic scalar order, or upstream's
# x86 AVX2 association (the reference's NGL=0 build)
NUMERICS_GENERIC, NUMERICS_X86, NUMERICS_FA = 0, 1, 2  # NUMERICS_FA is OR-ed into either (llmi.h)
PRESETS = (
    "llama3-8b-q4km", "llama3-70b-q4km", "tinyllama-q8_0", "mistral7b-q6k", "mistral7b-q5km",
    "tiny-mixed", "tiny-mixed-d128",
)


class LlmiError(RuntimeError):
    pass


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    if lib().llmi_rccl_unique_id(buf, 128) != 0:
        raise LlmiError(last_error())
    return buf.raw


def test_option(name: str, value: int = -1) -> int:
    """llmi_test_option: set a test-only option (value < 0: query); returns the old value."""
    r = int(lib().llmi_test_option(name.encode(), int(value)))
    if r < 0:
        raise LlmiError(last_error())
    return r


def device_count() -> int:
    return int(lib().llmi_device_count())


def fanout_plan(arena_bytes: int, chunk: int, prefix_ends: Sequence[int]) -> list[int]:
    """The replica fan-out schedule (model.cpp fanout_plan): for each chunk-sized piece of
    the arena, the index of the first upload prefix that covers it.  Host only."""
    n = len(prefix_ends)
    pe = (C.c_uint64 * max(1, n))(*prefix_ends)
    cap = (arena_bytes + chunk - 1) // chunk if chunk else 0
    rd = (C.c_int32 * max(1, cap))()
    k = lib().llmi_fanout_plan(int(arena_bytes), int(chunk), pe, n, rd, int(cap))
    if k < 0:
        raise LlmiError("llmi_fanout_plan: bad arguments")
    return [int(rd[i]) for i in range(k)]


def write_synthetic_gguf(path: str, preset: str, seed: int = 3, n_layer: int = 0, n_vocab: int = 0,
                         n_threads: int = 0) -> int:
    """Write a synthetic GGUF with the exact shapes/type table of `preset`."""
    n = lib().llmi_synth_write_gguf(path.encode(), preset.encode(), seed, n_layer, n_vocab, n_threads)
    if n < 0:
        raise LlmiError(last_error())
    return int(n)


class Vocab:
    """The native tokenizer (llama_tokenize / llama_token_to_piece / llama_detokenize of
    the C ABI, csrc/tokenizer.cpp).  From a model (Model.vocab) or, tokenizer only, from
    any GGUF's metadata (Vocab.from_file)."""

    def __init__(self, handle, owned: bool = False, keep=None):
        if not handle:
            raise LlmiError(f"vocab: {last_error()}")
        self._h, self._owned, self._keep = handle, owned, keep

    @classmethod
    def from_file(cls, path: str) -> "Vocab":
        return cls(lib().llmi_vocab_load_from_file(path.encode()), owned=True)

    @property
    def n_tokens(self) -> int:
        return lib().llama_vocab_n_tokens(self._h)

    @property
    def bos(self) -> int:
        return lib().llama_vocab_bos(self._h)

    @property
    def eos(self) -> int:
        return lib().llama_vocab_eos(self._h)

    def tokenize(self, text: str, add_special: bool = True, parse_special: bool = True) -> list[int]:
        L = lib()
        b = text.encode("utf-8")
        cap = len(b) + 8
        while True:
            buf = (C.c_int32 * cap)()
            n = L.llama_tokenize(self._h, b, len(b), buf, cap, add_special, parse_special)
            if n == -(2 ** 31):
                raise LlmiError(f"llama_tokenize: {last_error()}")
            if n >= 0:
                return list(buf[:n])
            cap = -n

    def piece(self, tid: int, special: bool = False, lstrip: int = 0) -> bytes:
        L = lib()
        buf = C.create_string_buffer(64)
        n = L.llama_token_to_piece(self._h, int(tid), buf, 64, lstrip, special)
        if n < 0:
            buf = C.create_string_buffer(-n)
            n = L.llama_token_to_piece(self._h, int(tid), buf, -n, lstrip, special)
        return buf.raw[:n]

    def detokenize(self, ids: Sequence[int], remove_special: bool = False, unparse_special: bool = False) -> bytes:
        L = lib()
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        cap = 16 * len(ids) + 16
        buf = C.create_string_buffer(cap)
        n = L.llama_detokenize(self._h, arr, len(ids), buf, cap, remove_special, unparse_special)
        if n < 0:
            buf = C.create_string_buffer(-n)
            n = L.llama_detokenize(self._h, arr, len(ids), buf, -n, remove_special, unparse_special)
        return buf.raw[:n]

    def close(self) -> None:
        if self._owned and self._h:
            lib().llmi_vocab_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



def device_hash(ptr: int, nbytes: int) -> int:
    """llmi_device_hash: the arena hash of any device memory (test hook)."""
    h = C.c_uint64()
    if lib().llmi_device_hash(C.c_void_p(ptr), int(nbytes), C.byref(h)) != 0:
        raise LlmiError(last_error())
    return int(h.value)

class Model:
    """llama_model_load_from_file: GGUF -> HBM arena on `main_gpu`."""

    def __init__(self, path: str, n_gpu_layers: int = 999, main_gpu: int = 0, vocab_only: bool = False,
                 no_upload: bool = False, numerics: int = NUMERICS_GENERIC):
        L = lib()
        p = L.llama_model_default_params()
        p.n_gpu_layers = n_gpu_layers
        p.main_gpu = main_gpu
        p.vocab_only = vocab_only
        p.no_upload = no_upload
        p.numerics = numerics
        self._h = L.llama_model_load_from_file(path.encode(), p)
        if not self._h:
            raise LlmiError(last_error())
        self.path = path
        self.device = main_gpu
        v = L.llama_model_get_vocab(self._h)
        self._vocab = v
        self.n_vocab = L.llama_vocab_n_tokens(v)
        self.bos = L.llama_vocab_bos(v)
        self.eos = L.llama_vocab_eos(v)
        self.n_embd = L.llama_model_n_embd(self._h)
        self.n_layer = L.llama_model_n_layer(self._h)
        self.n_head = L.llama_model_n_head(self._h)
        self.n_head_kv = L.llama_model_n_head_kv(self._h)
        self.n_ctx_train = L.llama_model_n_ctx_train(self._h)
        self.size = int(L.llama_model_size(self._h))
        buf = C.create_string_buffer(256)
        L.llama_model_desc(self._h, buf, 256)
        self.desc = buf.value.decode()
        self.numerics = int(L.llmi_model_numerics(self._h))

    @property
    def pooling_type(self) -> int:
        """The GGUF's <arch>.pooling_type (llmi_model_pooling_type), -1 when absent."""
        return int(lib().llmi_model_pooling_type(self._h))

    @classmethod
    def load_fanout(cls, path: str, main_gpu: int, uid: bytes, nranks: int, rank: int,
                    numerics: int = NUMERICS_GENERIC) -> "Model":
        """Load with the replica fan-out pipelined behind the upload (llmi_model_load_fanout,
        SURVEY.md §8e): every rank calls it with the same RCCL unique id; rank 0 uploads the
        GGUF, the others receive the arena in 256 MB pieces over xGMI."""
        L = lib()
        p = L.llama_model_default_params()
        p.main_gpu = main_gpu
        p.numerics = numerics
        h = L.llmi_model_load_fanout(path.encode(), p, uid, int(nranks), int(rank))
        if not h:
            raise LlmiError(last_error())
        return cls._from_handle(h, path, main_gpu)

    @classmethod
    def load_replicated(cls, path: str, main_gpu: int, devices: Sequence[int], n_gpu_layers: int = 999,
                        numerics: int = NUMERICS_GENERIC) -> tuple["Model", list["Model"]]:
        """One process: the model on main_gpu and a replica on each of `devices`, the RCCL
        broadcast pipelined behind the upload (llmi_model_load_replicated)."""
        L = lib()
        p = L.llama_model_default_params()
        p.main_gpu = main_gpu
        p.n_gpu_layers = n_gpu_layers
        p.numerics = numerics
        n = len(devices)
        devs = (C.c_int32 * max(1, n))(*devices)
        out = (C.c_void_p * max(1, n))()
        h = L.llmi_model_load_replicated(path.encode(), p, devs, n, out)
        if not h:
            raise LlmiError(last_error())
        return cls._from_handle(h, path, main_gpu), [cls._from_handle(out[i], path, devices[i]) for i in range(n)]

    @classmethod
    def _from_handle(cls, h, path: str, device: int) -> "Model":
        self = cls.__new__(cls)
        L = lib()
        self._h = h
        self.path = path
        self.device = device
        v = L.llama_model_get_vocab(h)
        self._vocab = v
        self.n_vocab = L.llama_vocab_n_tokens(v)
        self.bos, self.eos = L.llama_vocab_bos(v), L.llama_vocab_eos(v)
        self.n_embd, self.n_layer = L.llama_model_n_embd(h), L.llama_model_n_layer(h)
        self.n_head, self.n_head_kv = L.llama_model_n_head(h), L.llama_model_n_head_kv(h)
        self.n_ctx_train = L.llama_model_n_ctx_train(h)
        self.size = int(L.llama_model_size(h))
        self.desc = ""
        self.numerics = int(L.llmi_model_numerics(h))
        return self

    @property
    def vocab(self) -> Vocab:
        """The model's native tokenizer (owned by the model)."""
        return Vocab(self._vocab, owned=False, keep=self)

    def token_text(self, t: int) -> str:
        s = lib().llama_vocab_get_text(self._vocab, int(t))
        return s.decode("utf-8", "replace") if s is not None else ""

    @property
    def upload_s(self) -> float:
        """Seconds of the weight upload (chunked pinned H2D + on-device repack)."""
        return float(lib().llmi_model_upload_s(self._h))

    def bytes_per_token(self, n_kv: int) -> float:
        return float(lib().llmi_bytes_per_token(self._h, int(n_kv)))

    @property
    def prefill_supported(self) -> bool:
        """Whether llama_decode prefills prompts with the batched MFMA path (a flash-attention
        numerics model: only while LLMI_FA_PREFILL=1 is in the environment)."""
        return bool(lib().llmi_prefill_supported(self._h))

    def arena(self) -> tuple[int, int]:
        p, n = C.c_void_p(), C.c_uint64()
        lib().llmi_model_arena(self._h, C.byref(p), C.byref(n))
        return int(p.value or 0), int(n.value)

    def arena_hash(self) -> int:
        """Order-independent 64-bit hash of the device arena (llmi_model_arena_hash): equal
        on every replica of the same weights (the fan-out's replica check)."""
        h = C.c_uint64()
        if lib().llmi_model_arena_hash(self._h, C.byref(h)) != 0:
            raise LlmiError(last_error())
        return int(h.value)

    def replicate(self, devices: Sequence[int]) -> list["Model"]:
        """In-process RCCL broadcast of the arena to `devices`."""
        n = len(devices)
        devs = (C.c_int32 * n)(*devices)
        out = (C.c_void_p * n)()
        if lib().llmi_replicate(self._h, devs, n, out) != 0:
            raise LlmiError(last_error())
        return [Model._from_handle(out[i], self.path, devices[i]) for i in range(n)]

    def fanout(self, uid: bytes, nranks: int, rank: int) -> None:
        """Multi-process replica fan-out: RCCL broadcast of rank 0's arena."""
        if lib().llmi_model_fanout(self._h, uid, int(nranks), int(rank)) != 0:
            raise LlmiError(last_error())

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().llama_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sampler_params(params: Sequence):
    """A ctypes array of llmi_sampler_params from SamplingParams-like objects."""
    from ._lib import llmi_sampler_params

    arr = (llmi_sampler_params * len(params))()
    for a, p in zip(arr, params):
        a.temperature, a.top_p, a.min_p = float(p.temperature), float(p.top_p), float(p.min_p)
        a.repeat_penalty, a.presence_penalty = float(p.repeat_penalty), float(p.presence_penalty)
        a.frequency_penalty, a.top_k, a.repeat_last_n = float(p.frequency_penalty), int(p.top_k), int(p.repeat_last_n)
    return arr


def sample_logits(logits, history, params: Sequence, uniforms, want_penalized: bool = True):
    """llmi_sample_logits: k_sample alone over crafted rows.  logits [rows][V] f32, history
    [rows][n_hist] int32 (n_hist may be 0), params one SamplingParams per row, uniforms
    [rows].  Returns (tokens, candidates, penalized, usec): the chosen token per row, each
    row's final candidate ids (empty for a greedy row), the rows' values at their history
    tokens after the kernel, and the launch's device microseconds."""
    from ._lib import SAMPLE_MAX_TOP_K

    lg = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    rows, V = lg.shape
    hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32).reshape(rows, -1))
    n_hist = hist.shape[1]
    un = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64).reshape(rows))
    tok = np.zeros(rows, dtype=np.int32)
    cand = np.zeros((rows, SAMPLE_MAX_TOP_K), dtype=np.int32)
    ncand = np.zeros(rows, dtype=np.int32)
    pen = np.zeros((rows, n_hist), dtype=np.float32)
    us = C.c_double()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    r = lib().llmi_sample_logits(vp(lg), rows, V, vp(hist) if n_hist else None, n_hist, sampler_params(params), vp(un),
                                 vp(tok), vp(cand), vp(ncand), vp(pen) if want_penalized else None, C.byref(us))
    if r != 0:
        raise LlmiError(f"llmi_sample_logits returned {r}: {last_error()}")
    return ([int(t) for t in tok], [[int(c) for c in cand[i, :ncand[i]]] for i in range(rows)], pen, us.value)


def logprob_rows(logits, history, params: Sequence, uniforms, n_top: Sequence[int], want_rows: bool = True):
    """llmi_logprob_rows: k_logprob, k_sample, k_logprob_pick in step order over crafted rows.
    logits, history, params, uniforms as sample_logits; n_top one of -1, 0..20 per row.
    Returns a dict: tokens [rows], tok_logprob and lse float64 [rows] (NaN for a row with n_top
    -1: the kernels left it alone), top_ids int32 and top_logprobs float64 [rows][20] (unused
    entries -1 and -inf), rows the logits after the kernels (None unless wanted), usec the
    event-timed microseconds of (k_logprob, k_sample, k_logprob_pick)."""
    from ._lib import LOGPROBS_MAX_TOP

    lg = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    rows, V = lg.shape
    hist = np.ascontiguousarray(np.asarray(history, dtype=np.int32).reshape(rows, -1))
    n_hist = hist.shape[1]
    un = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64).reshape(rows))
    nt = np.ascontiguousarray(np.asarray(n_top, dtype=np.int32).reshape(rows))
    tok = np.zeros(rows, dtype=np.int32)
    tok_lp, lse = np.full(rows, np.nan), np.full(rows, np.nan)
    top_id = np.full((rows, LOGPROBS_MAX_TOP), -2, dtype=np.int32)
    top_lp = np.full((rows, LOGPROBS_MAX_TOP), np.nan)
    after = np.zeros((rows, V), dtype=np.float32) if want_rows else None
    us = (C.c_double * 3)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    r = lib().llmi_logprob_rows(vp(lg), rows, V, vp(hist) if n_hist else None, n_hist, sampler_params(params), vp(un),
                                vp(nt), vp(tok), vp(tok_lp), vp(lse), vp(top_id), vp(top_lp),
                                vp(after) if want_rows else None, C.cast(us, C.c_void_p))
    if r != 0:
        raise LlmiError(f"llmi_logprob_rows returned {r}: {last_error()}")
    return {"tokens": [int(t) for t in tok], "tok_logprob": tok_lp, "lse": lse, "top_ids": top_id, "top_logprobs": top_lp,
            "rows": after, "usec": tuple(us)}


def kv_seq_copy(n_planes: int, head_dim: int, n_ctx: int, p0: int, p1: int, kc_src: int, vc_src: int, hist_src: int,
                kc_dst: int, vc_dst: int, hist_dst: int) -> float:
    """llmi_kv_seq_copy: k_kv_seq_cp alone (Context.seq_cp's launch) over device addresses:
    positions [p0, p1) of the src K cache [n_planes][n_ctx][head_dim] f16, transposed V cache
    [n_planes][head_dim][n_ctx] f16 and history [n_ctx] int32 into the dst ones.  Returns the
    launch's event-timed device microseconds; bad arguments raise before any device call."""
    us = C.c_double()
    vp = lambda a: C.c_void_p(int(a)) if a else None  # noqa: E731
    r = lib().llmi_kv_seq_copy(int(n_planes), int(head_dim), int(n_ctx), int(p0), int(p1), vp(kc_src), vp(vc_src),
                               vp(hist_src), vp(kc_dst), vp(vc_dst), vp(hist_dst), C.byref(us))
    if r != 0:
        raise LlmiError(f"llmi_kv_seq_copy returned {r}: {last_error()}")
    return us.value


def embd_pool(x_dev: int, ldx: int, n_tok: int, n_embd: int, norm_w_dev: int, eps: float, pooling: int, n_total: int,
              t0: int, acc_dev: int, out_dev: int) -> float:
    """llmi_embd_pool: k_embd_rows / k_embd_mean alone (llama_decode's embeddings launch) over
    device addresses: x [n_tok][ldx] f32, the final hidden states of tokens t0 .. t0 + n_tok - 1
    of a sequence of n_total; norm_w [n_embd]; acc [n_embd] float64 (mean; 0 otherwise); out
    [n_tok][n_embd] for POOLING_NONE, else [n_embd].  Returns the launches' event-timed device
    microseconds; bad arguments raise before any device call."""
    us = C.c_double()
    vp = lambda a: C.c_void_p(int(a)) if a else None  # noqa: E731
    r = lib().llmi_embd_pool(vp(x_dev), int(ldx), int(n_tok), int(n_embd), vp(norm_w_dev), float(eps), int(pooling),
                             int(n_total), int(t0), vp(acc_dev), vp(out_dev), C.byref(us))
    if r != 0:
        raise LlmiError(f"llmi_embd_pool returned {r}: {last_error()}")
    return us.value


# the device's StepState (llmi_step_state) as a NumPy record
STEP_STATE = np.dtype([("token_in", "<i4"), ("token_in_pos", "<i4"), ("pos_next", "<i4"), ("pos", "<i4"), ("token", "<i4"),
                       ("seq", "<u4"), ("key", "<u8", (2, 64))])


def step_entry(kernel: int, qtype: int, w_dev: int, vocab: int, cols: int, n_ctx: int, states=None, hist=None, tseq=None,
               tpos=None, tokens=None, pos0: int = 0):
    """llmi_step_entry: one step-entry launch (kernel 0 k_embed, 1 k_bembed, 2 k_pf_embed, 3
    k_embed_row) over the [vocab][cols] weight at device address w_dev.  states: STEP_STATE
    records, one per sequence (kernels 0 / 1 / 3); hist int32 [n_seq][n_ctx] (kernels 0 / 1 /
    2); tseq the slots' sequences and tpos int32 [8] (kernel 1); tokens and pos0 (kernel 2).
    The inputs are left alone.  Returns (x, states, hist, tpos, guard_bad): x uint32
    [slots][cols] (the f32 bits; a slot the launch did not write holds STEP_SENTINEL), the
    states, hist and tpos after the launch (None where the kernel has none), and the
    changed guard words of the hook's x, hist and state buffers."""
    from ._lib import llmi_step_entry_args, llmi_step_state

    a = llmi_step_entry_args()
    a.kernel, a.type, a.w_dev, a.vocab, a.cols, a.n_ctx, a.pos0 = kernel, qtype, w_dev, vocab, cols, n_ctx, pos0
    i32p = lambda v: v.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    st = hs = tp = ts = tk = None
    a.n_seq = 1
    if kernel != 2:
        st = np.array(states, dtype=STEP_STATE).reshape(-1)
        a.states, a.n_seq = st.ctypes.data_as(C.POINTER(llmi_step_state)), len(st)
    if kernel != 3:
        hs = np.array(hist, dtype=np.int32).reshape(a.n_seq, n_ctx)
        a.hist = i32p(hs)
    a.nt = 1
    if kernel == 1:
        ts, tp = np.array(tseq, dtype=np.int32).reshape(-1), np.array(tpos, dtype=np.int32).reshape(8)
        a.tseq, a.tpos, a.nt = i32p(ts), i32p(tp), len(ts)
    elif kernel == 2:
        tk = np.array(tokens, dtype=np.int32).reshape(-1)
        a.tokens, a.nt = i32p(tk), len(tk)
    x = np.zeros((8 if kernel == 1 else a.nt, cols), dtype=np.uint32)
    bad = np.full(3, -1, dtype=np.int32)
    a.x_out, a.guard_bad = x.ctypes.data_as(C.POINTER(C.c_uint32)), i32p(bad)
    r = lib().llmi_step_entry(C.byref(a))
    if r != 0:
        raise LlmiError(f"llmi_step_entry returned {r}: {last_error()}")
    return x, st, hs, tp, [int(b) for b in bad]


class Context:
    """llama_init_from_model: KV cache + scratch + step graphs on the model's device."""

    def __init__(self, model: Model, n_ctx: int = 0, use_graphs: bool = True, n_seq: int = 1):
        L = lib()
        p = L.llama_context_default_params()
        p.n_ctx = n_ctx
        p.use_graphs = use_graphs
        p.n_seq_max = n_seq
        self.n_seq = n_seq
        self._h = L.llama_init_from_model(model._h, p)
        if not self._h:
            raise LlmiError(last_error())
        self.model = model
        self.n_ctx = int(L.llama_n_ctx(self._h))

    def decode(self, tokens: Sequence[int], pos: Optional[Sequence[int]] = None, logits_all: bool = False,
               seq: Optional[Sequence[int]] = None) -> int:
        """llama_decode: returns 0 ok, 1 no KV slot, <0 error (same codes as upstream).
        seq: per-token sequence id (llama_batch.seq_id[i][0]); None = sequence 0."""
        n = len(tokens)
        toks = (C.c_int32 * n)(*tokens)
        b = lib().llama_batch_get_one(toks, n)
        keep = [toks]
        if seq is not None:
            ids = [(C.c_int32 * 1)(int(s)) for s in seq]
            ptrs = (C.POINTER(C.c_int32) * n)(*[C.cast(a, C.POINTER(C.c_int32)) for a in ids])
            nsi = (C.c_int32 * n)(*([1] * n))
            b.seq_id = C.cast(ptrs, C.POINTER(C.POINTER(C.c_int32)))
            b.n_seq_id = C.cast(nsi, C.POINTER(C.c_int32))
            keep += [ids, ptrs, nsi]
        if pos is not None:
            pa = (C.c_int32 * n)(*pos)
            b.pos = C.cast(pa, C.POINTER(C.c_int32))
            keep.append(pa)
        if logits_all:
            la = (C.c_int8 * n)(*([1] * n))
            b.logits = C.cast(la, C.POINTER(C.c_int8))
            keep.append(la)
        rc = int(lib().llama_decode(self._h, b))
        del keep
        return rc

    @property
    def prefill_tokens(self) -> int:
        """Tokens this context has sent through the batched prefill path (llmi_prefill_token_count)."""
        return int(lib().llmi_prefill_token_count(self._h))

    def eval(self, tokens: Sequence[int], n_past: int) -> int:
        n = len(tokens)
        toks = (C.c_int32 * n)(*tokens)
        return int(lib().llama_eval(self._h, toks, n, n_past))

    def logits(self, i: int = -1) -> np.ndarray:
        p = lib().llama_get_logits_ith(self._h, i)
        if not p:
            raise LlmiError(last_error())
        return np.ctypeslib.as_array(p, shape=(self.model.n_vocab,)).copy()

    def tap(self, which: int, n: int) -> np.ndarray:
        """llmi_debug_tap of the last decode step (the oracle's or_tap numbering): 0
        embedding row, 1 residual x after the last layer, 2 roped q, 3 attention output,
        4 SwiGLU output (the last layer's); 7 / 8 the last layer's raw f16 K / V cache.
        n = element count (f32; u16 for 7 / 8)."""
        out = np.empty(n, dtype=np.uint16 if which in (7, 8) else np.float32)
        if lib().llmi_debug_tap(self._h, int(which), out.ctypes.data_as(C.c_void_p)) != 0:
            raise LlmiError(last_error())
        return out

    def greedy(self, i: int = -1) -> int:
        t = int(lib().llmi_greedy_ith(self._h, i))
        if t < 0:
            raise LlmiError(last_error())
        return t

    def generate_greedy(self, first: int, pos0: int, n: int) -> list[int]:
        out = (C.c_int32 * n)()
        r = lib().llmi_generate_greedy(self._h, int(first), int(pos0), int(n), out)
        if r != n:
            raise LlmiError(f"llmi_generate_greedy returned {r}: {last_error()}")
        return list(out)

    def generate_greedy_batch(self, seqs: Sequence[int], first: Sequence[int], pos0: Sequence[int], n: int) -> list[list[int]]:
        """llmi_generate_greedy_batch: sequences seqs advance together, one batched step
        per token (continuous batching); returns each sequence's n tokens."""
        k = len(seqs)
        sa, fa, pa = (C.c_int32 * k)(*seqs), (C.c_int32 * k)(*first), (C.c_int32 * k)(*pos0)
        out = (C.c_int32 * (k * n))()
        r = lib().llmi_generate_greedy_batch(self._h, k, sa, fa, pa, int(n), out)
        if r != n:
            raise LlmiError(f"llmi_generate_greedy_batch returned {r}: {last_error()}")
        return [list(out[i * n:(i + 1) * n]) for i in range(k)]

    def generate_sampled_batch(self, seqs: Sequence[int], first: Sequence[int], pos0: Sequence[int], n: int,
                               params: Sequence, uniforms) -> list[list[int]]:
        """llmi_generate_sampled_batch: generate_greedy_batch with each sequence's sampler
        chain (params[k]: a SamplingParams) run on the device after every step; uniforms[k]
        holds sequence k's n draws (ignored for a greedy chain).  Tokens equal
        sampling.sample_with_uniform on each step's logits."""
        k = len(seqs)
        sa, fa, pa = (C.c_int32 * k)(*seqs), (C.c_int32 * k)(*first), (C.c_int32 * k)(*pos0)
        un = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64).reshape(k, n))
        out = (C.c_int32 * (k * n))()
        r = lib().llmi_generate_sampled_batch(self._h, k, sa, fa, pa, int(n), sampler_params(params),
                                              un.ctypes.data_as(C.POINTER(C.c_double)), out)
        if r != n:
            raise LlmiError(f"llmi_generate_sampled_batch returned {r}: {last_error()}")
        return [list(out[i * n:(i + 1) * n]) for i in range(k)]

    def generate_logprobs_batch(self, seqs: Sequence[int], first: Sequence[int], pos0: Sequence[int], n: int,
                                params: Sequence, uniforms, n_top: Sequence[int]):
        """llmi_generate_logprobs_batch: generate_sampled_batch that also returns, for each
        sequence k with n_top[k] >= 0, the log-probabilities of its tokens under each step's raw
        distribution and the n_top[k] most likely alternatives (sampling.token_logprobs on
        the device).  Returns (tokens, logprobs): tokens as generate_sampled_batch; logprobs[k]
        None for n_top[k] == -1, else a list of n entries (token_logprob, top_ids,
        top_logprobs) with n_top[k] alternatives (fewer when the vocabulary is smaller)."""
        from ._lib import LOGPROBS_MAX_TOP as T

        k = len(seqs)
        sa, fa, pa = (C.c_int32 * k)(*seqs), (C.c_int32 * k)(*first), (C.c_int32 * k)(*pos0)
        na = (C.c_int32 * k)(*[int(t) for t in n_top])
        un = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64).reshape(k, n))
        out = (C.c_int32 * (k * n))()
        tok_lp = np.full((k, n), np.nan)
        top_id = np.full((k, n, T), -2, dtype=np.int32)
        top_lp = np.full((k, n, T), np.nan)
        r = lib().llmi_generate_logprobs_batch(self._h, k, sa, fa, pa, int(n), sampler_params(params),
                                               un.ctypes.data_as(C.POINTER(C.c_double)), na, out,
                                               tok_lp.ctypes.data_as(C.POINTER(C.c_double)),
                                               top_id.ctypes.data_as(C.POINTER(C.c_int32)),
                                               top_lp.ctypes.data_as(C.POINTER(C.c_double)))
        if r != n:
            raise LlmiError(f"llmi_generate_logprobs_batch returned {r}: {last_error()}")
        lps = []
        for i in range(k):
            if na[i] < 0:
                lps.append(None)
                continue
            m = [int((top_id[i, j] >= 0).sum()) for j in range(n)]
            lps.append([(float(tok_lp[i, j]), [int(t) for t in top_id[i, j, :m[j]]], [float(v) for v in top_lp[i, j, :m[j]]])
                        for j in range(n)])
        return [list(out[i * n:(i + 1) * n]) for i in range(k)], lps

    def set_embeddings(self, on: bool) -> None:
        """llama_set_embeddings: while on, decode also pools the final hidden states of each
        sequence's tokens (embeddings_seq / embeddings_ith).  Off by default."""
        lib().llama_set_embeddings(self._h, bool(on))

    def set_pooling(self, pooling: int) -> None:
        """llmi_set_pooling_type: POOLING_NONE / MEAN / CLS / LAST (RANK is refused)."""
        if lib().llmi_set_pooling_type(self._h, int(pooling)) != 0:
            raise LlmiError(last_error())

    @property
    def pooling(self) -> int:
        """llama_pooling_type: the model's GGUF default unless set_pooling changed it."""
        return int(lib().llama_pooling_type(self._h))

    def embeddings_seq(self, seq: int = 0) -> np.ndarray:
        """llama_get_embeddings_seq: the pooled (not normalised) vector of sequence seq from the
        last decode."""
        p = lib().llama_get_embeddings_seq(self._h, int(seq))
        if not p:
            raise LlmiError(last_error())
        return np.ctypeslib.as_array(p, shape=(self.model.n_embd,)).copy()

    def embeddings_ith(self, i: int = -1) -> np.ndarray:
        """llama_get_embeddings_ith (pooling none): batch token i's normed row, -1 the last."""
        p = lib().llama_get_embeddings_ith(self._h, int(i))
        if not p:
            raise LlmiError(last_error())
        return np.ctypeslib.as_array(p, shape=(self.model.n_embd,)).copy()

    def seq_rm(self, seq: int, p0: int = 0, p1: int = -1) -> bool:
        """llama_kv_self_seq_rm (tail removal)."""
        return bool(lib().llama_kv_self_seq_rm(self._h, int(seq), int(p0), int(p1)))

    def seq_cp(self, src: int, dst: int, p0: int = 0, p1: int = -1) -> bool:
        """llama_kv_self_seq_cp: positions [p0, p1) of sequence src into sequence dst on the
        device (p1 < 0: all src holds); dst's past becomes p1.  False (last_error() says why) for
        a bad sequence, src == dst, a range src does not hold or one that would leave a hole."""
        return bool(lib().llama_kv_self_seq_cp(self._h, int(src), int(dst), int(p0), int(p1)))

    def seq_pos_max(self, seq: int) -> int:
        return int(lib().llmi_seq_pos_max(self._h, int(seq)))

    def stats(self) -> tuple[float, float]:
        b, u = C.c_double(), C.c_double()
        lib().llmi_last_step_stats(self._h, C.byref(b), C.byref(u))
        return b.value, u.value

    KERNEL_CLASSES = ("embed", "qkv", "attention", "attn_output", "ffn_gate_up", "ffn_down", "output", "layer")

    def profile_kernels(self, first: int, pos0: int, n_steps: int) -> dict:
        """Per-kernel-class mean kernel execution time / algorithmic bytes per launch:
        each class's launches of n_steps steps at pos0, every launch bracketed by HIP
        events recorded at kernel start/end (llmi_profile_kernels).  Consumes no tokens."""
        n = len(self.KERNEL_CLASSES)
        us, by, nl = (C.c_double * n)(), (C.c_double * n)(), (C.c_int32 * n)()
        if lib().llmi_profile_kernels(self._h, int(first), int(pos0), int(n_steps), us, by, nl) != 0:
            raise LlmiError(last_error())
        return {k: {"us": us[i], "bytes": by[i], "launches_per_step": nl[i],
                    "GBps": (by[i] / (us[i] * 1e-6) / 1e9) if us[i] > 0 else 0.0}
                for i, k in enumerate(self.KERNEL_CLASSES)}

    def engine_trace(self, first: int, pos0: int, layer: int) -> np.ndarray:
        """llmi_engine_trace: s_memrealtime stamps (10 ns ticks) of layer `layer`'s layer-engine
        launch in one eager step at pos0, shaped [CUs][16 wave slots][32] (tools/letrace.py)."""
        n = 256 * 16 * 32 * 4
        out = (C.c_uint64 * n)()
        g = int(lib().llmi_engine_trace(self._h, int(first), int(pos0), int(layer), out, n))
        if g < 0:
            raise LlmiError(last_error())
        return np.ctypeslib.as_array(out)[: g * 16 * 32].reshape(g, 16, 32).copy()

    def kv_clear(self) -> None:
        lib().llama_kv_self_clear(self._h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().llama_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
