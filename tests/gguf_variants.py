"""Pure-Python GGUF rewriter (test infrastructure): the GGUF shapes the loader accepts
but csrc/synth_writer.cpp never writes.

load() keeps every KV's value type and raw bytes and every tensor's bytes as a view of
the mapped file; save() writes them back with the offsets recomputed at the file's
alignment exactly as synth_writer.cpp lays a file out (every tensor, the last one too,
padded with zeros to the alignment), so an unedited file comes back byte for byte.
Tensor data is only ever moved as whole buffers (no per-element Python loops).

Named variants, each a function of a base path that writes one file into `out_dir` (the
session's synth_dir) and returns its path:
  ropefreqs     + F32 rope_freqs.weight of n_rot/2 factors (rope_factors)
  nrot(k)       llama.rope.dimension_count = k
  tied(T)       no output.weight; token_embd.weight = random_blocks of type T
  mha           head_count_kv = head_count; attn_k / attn_v random at [E, E], own type
  llama32like   ropefreqs + tied
  ties(rows)    row `src` of the output matrix copied over `rows` (equal logits)
"""
from __future__ import annotations

import mmap
import os
import struct

import numpy as np

import gguf_reader as gr
from helpers import F32, Q4_K, Q5_K, Q6_K, Q8_0, TNAME, random_blocks

U32, F32_KV, STR = gr.U32, gr.F32, gr.STR


class Tensor:
    def __init__(self, name, ne, type_, data):
        self.name, self.ne, self.type, self.data = name, list(ne), int(type_), data

    @property
    def nbytes(self):
        _, be, bb = gr.GGML_TYPES[self.type]
        return int(np.prod(self.ne, dtype=np.int64)) // be * bb


class Gguf:
    """version, KVs as [key, value type, raw value bytes] in file order, tensors in file order."""

    def __init__(self, version, kvs, tensors):
        self.version, self.kvs, self.tensors = version, kvs, tensors

    # ---- reading ----
    def kv(self, key, default=None):
        for k, t, raw in self.kvs:
            if k == key:
                return gr.Reader(raw).value(t)
        return default

    @property
    def alignment(self):
        return int(self.kv("general.alignment", 32))

    def tensor(self, name):
        for t in self.tensors:
            if t.name == name:
                return t
        return None

    # ---- edits ----
    def set_kv(self, key, vtype, value):
        """Set (in place) or append a scalar or string KV."""
        if vtype == STR:
            b = value.encode("utf-8")
            raw = struct.pack("<Q", len(b)) + b
        else:
            raw = struct.pack(gr._SCALAR[vtype], value)
        for e in self.kvs:
            if e[0] == key:
                e[1], e[2] = vtype, raw
                return
        self.kvs.append([key, vtype, raw])

    def drop_tensor(self, name):
        assert self.tensor(name) is not None, name
        self.tensors = [t for t in self.tensors if t.name != name]

    def add_tensor(self, name, ne, type_, data):
        assert self.tensor(name) is None, name
        t = Tensor(name, ne, type_, data)
        assert len(memoryview(data).cast("B")) == t.nbytes, name
        self.tensors.append(t)

    def replace_tensor(self, name, ne, type_, data):
        t = self.tensor(name)
        assert t is not None, name
        t.ne, t.type, t.data = list(ne), int(type_), data
        assert len(memoryview(data).cast("B")) == t.nbytes, name


def load(path: str) -> Gguf:
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    view = memoryview(mm)
    r = gr.Reader(mm)
    if mm[:4] != gr.GGUF_MAGIC:
        raise ValueError("not a GGUF file")
    r.o = 4
    version = r.take("<I")
    n_tensors, n_kv = r.take("<Q"), r.take("<Q")
    kvs = []
    for _ in range(n_kv):
        k = r.string()
        t = r.take("<I")
        o = r.o
        r.value(t)
        kvs.append([k, t, bytes(view[o:r.o])])
    infos = []
    for _ in range(n_tensors):
        name = r.string()
        nd = r.take("<I")
        ne = [r.take("<Q") for _ in range(nd)]
        typ = r.take("<I")
        infos.append((name, ne, typ, r.take("<Q")))
    g = Gguf(version, kvs, [])
    align = g.alignment
    start = (r.o + align - 1) // align * align
    for name, ne, typ, off in infos:
        t = Tensor(name, ne, typ, None)
        t.data = view[start + off: start + off + t.nbytes]
        g.tensors.append(t)
    return g


def _s(x: str) -> bytes:
    b = x.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def save(g: Gguf, path: str) -> str:
    align = g.alignment
    up = lambda n: (n + align - 1) // align * align  # noqa: E731
    head = [gr.GGUF_MAGIC, struct.pack("<IQQ", g.version, len(g.tensors), len(g.kvs))]
    for k, t, raw in g.kvs:
        head += [_s(k), struct.pack("<I", t), raw]
    off = 0
    for t in g.tensors:
        head += [_s(t.name), struct.pack("<I", len(t.ne)), struct.pack(f"<{len(t.ne)}Q", *t.ne),
                 struct.pack("<IQ", t.type, off)]
        off = up(off + t.nbytes)
    head = b"".join(head)
    with open(path, "wb") as f:
        f.write(head)
        f.write(b"\0" * (up(len(head)) - len(head)))
        for t in g.tensors:
            f.write(t.data)
            f.write(b"\0" * (up(t.nbytes) - t.nbytes))
    return path


# ---- the edits behind the named variants ------------------------------------------------
def head_dim(g: Gguf) -> int:
    return g.kv("llama.embedding_length") // g.kv("llama.attention.head_count")


def n_rot(g: Gguf) -> int:
    return g.kv("llama.rope.dimension_count", head_dim(g))


def rope_factors(n: int) -> np.ndarray:
    """n frequency factors shaped like Llama-3.1's: 1.0 on the first third (the high
    frequencies), 8.0 on the last third, and between them 1 + 7 (2 j - 1) / (2 m), j = 1..m,
    none of which is a power of two for the n used here (so theta / ff rounds;
    test_gguf_variants.py asserts it)."""
    lo = n // 3
    m = n - 2 * lo
    mid = 1.0 + 7.0 * (2.0 * np.arange(1, m + 1, dtype=np.float64) - 1.0) / (2.0 * m)
    return np.concatenate([np.ones(lo), mid, np.full(lo, 8.0)]).astype(np.float32)


def edit_ropefreqs(g: Gguf, n: int | None = None):
    n = n_rot(g) // 2 if n is None else n
    g.add_tensor("rope_freqs.weight", [n], F32, rope_factors(n).tobytes())


def edit_nrot(g: Gguf, k: int):
    g.set_kv("llama.rope.dimension_count", U32, k)


def _random_embd(g: Gguf, qtype: int, seed: int = 1234):
    """token_embd.weight replaced by random_blocks of qtype at its own shape (one draw per
    type: tied(T) and embd_only(T) hold the same embedding)."""
    cols, rows = g.tensor("token_embd.weight").ne
    g.replace_tensor("token_embd.weight", [cols, rows], qtype,
                     random_blocks(qtype, rows, cols, np.random.default_rng(seed + qtype)).tobytes())


def edit_tied(g: Gguf, qtype: int):
    g.drop_tensor("output.weight")
    _random_embd(g, qtype)


def edit_mha(g: Gguf, seed: int = 4321):
    E = g.kv("llama.embedding_length")
    g.set_kv("llama.attention.head_count_kv", U32, g.kv("llama.attention.head_count"))
    for i, t in enumerate(g.tensors):
        if t.name.endswith(("attn_k.weight", "attn_v.weight")):
            g.replace_tensor(t.name, [E, E], t.type, random_blocks(t.type, E, E, np.random.default_rng(seed + i)).tobytes())


def row_bytes(t: Tensor) -> int:
    _, be, bb = gr.GGML_TYPES[t.type]
    return t.ne[0] // be * bb


def output_tensor(g: Gguf) -> Tensor:
    return g.tensor("output.weight") or g.tensor("token_embd.weight")


def edit_ties(g: Gguf, src: int, rows):
    """Row `src` of the output matrix (token_embd when tied) over every row of `rows`."""
    t = output_tensor(g)
    rb = row_bytes(t)
    m = np.frombuffer(t.data, dtype=np.uint8).reshape(t.ne[1], rb).copy()
    m[[r for r in rows if r != src]] = m[src]
    t.data = m.tobytes()


# ---- named variants ---------------------------------------------------------------------
def _variant(base: str, out_dir, tag: str, *edits) -> str:
    """base + edits -> out_dir/<base stem>-<tag>.gguf, written once per session directory."""
    out = os.path.join(str(out_dir), f"{os.path.splitext(os.path.basename(base))[0]}-{tag}.gguf")
    if not os.path.exists(out):
        g = load(base)
        for e in edits:
            e(g)
        save(g, out + ".tmp")
        os.replace(out + ".tmp", out)
    return out


def identity(base, out_dir):
    return _variant(base, out_dir, "identity")


def ropefreqs(base, out_dir):
    return _variant(base, out_dir, "ropefreqs", edit_ropefreqs)


def nrot(base, out_dir, k: int):
    return _variant(base, out_dir, f"nrot{k}", lambda g: edit_nrot(g, k))


def nrot_ropefreqs(base, out_dir, k: int):
    """nrot(k) with a rope_freqs.weight of the k/2 factors it needs."""
    return _variant(base, out_dir, f"nrot{k}-ropefreqs", lambda g: edit_nrot(g, k), edit_ropefreqs)


def tied(base, out_dir, qtype: int):
    return _variant(base, out_dir, f"tied-{TNAME[qtype]}", lambda g: edit_tied(g, qtype))


def mha(base, out_dir):
    return _variant(base, out_dir, "mha", edit_mha)


def llama32like(base, out_dir, qtype: int = Q6_K):
    return _variant(base, out_dir, f"llama32like-{TNAME[qtype]}", edit_ropefreqs, lambda g: edit_tied(g, qtype))


def ties(base, out_dir, src: int, rows):
    return _variant(base, out_dir, "ties-" + "-".join(str(r) for r in sorted(rows)), lambda g: edit_ties(g, src, rows))


def embd_only(base, out_dir, qtype: int):
    """tied(T)'s token_embd with the base's separate output.weight kept (the control that
    shows what tying changes)."""
    return _variant(base, out_dir, f"embd-{TNAME[qtype]}", lambda g: _random_embd(g, qtype))


# name -> (base, out_dir, head_dim) -> path: every variant the parity tests run on the tiny presets
VARIANTS = {
    "ropefreqs": lambda b, o, D: ropefreqs(b, o),
    "nrot-half": lambda b, o, D: nrot(b, o, D // 2),
    "nrot-last-pair": lambda b, o, D: nrot(b, o, D - 2),
    "tied-q4_K": lambda b, o, D: tied(b, o, Q4_K),
    "tied-q5_K": lambda b, o, D: tied(b, o, Q5_K),
    "tied-q6_K": lambda b, o, D: tied(b, o, Q6_K),
    "tied-q8_0": lambda b, o, D: tied(b, o, Q8_0),
    "mha": lambda b, o, D: mha(b, o),
    "llama32like": lambda b, o, D: llama32like(b, o),
}
TINY_HEAD_DIM = {"tiny-mixed": 64, "tiny-mixed-d128": 128}

# ---- greedy ties ------------------------------------------------------------------------
TIE_PROMPT = [1, 5, 9, 400, 77, 33, 250, 611, 18, 96, 305, 42]
TIE_SETS = ("pair", "spread", "last-pair")


_ARGMAX = {}  # (path, prompt) -> oracle_argmax, computed once per process


def oracle_argmax(path: str, prompt) -> int:
    """np.argmax of the oracle's logits after the prompt's last token."""
    import pyoracle as po

    key = (path, tuple(prompt))
    if key not in _ARGMAX:
        om = po.OracleModel(path, n_ctx=64)
        try:
            for pos, t in enumerate(prompt[:-1]):
                om.decode(t, pos, logits=False)
            _ARGMAX[key] = int(np.argmax(om.decode(prompt[-1], len(prompt) - 1)))
        finally:
            om.close()
    return _ARGMAX[key]


def tie_rows(kind: str, r: int, n_vocab: int, prompt) -> list[int]:
    """The tie set of `kind` around the argmax row r: 'pair' the two rows of r's LOGITS
    pair; 'spread' {a, r, b} with a < 64 and b > V/2 (other workgroups and argmax slots);
    'last-pair' {r, V-1}, the single-row last pair of an odd vocabulary.  No copied row is
    a prompt token (on a tied file the copies are embedding rows too)."""
    if kind == "pair":
        rows = [r & ~1, (r & ~1) + 1]
    elif kind == "spread":
        a = next(i for i in range(37, 64) if i != r and i not in prompt)
        b = next(i for i in range(n_vocab - 70, n_vocab // 2, -1) if i != r and i not in prompt)
        rows = sorted({a, r, b})
    else:
        assert n_vocab % 2 == 1
        rows = [r, n_vocab - 1]
    assert len(set(rows)) == len(rows) >= 2 and max(rows) < n_vocab, (kind, r, rows)
    assert not (set(rows) - {r}) & set(prompt), (kind, rows)
    return rows


def tie_file(base, out_dir, kind: str, prompt=TIE_PROMPT):
    """(path, rows): `base` with its argmax row after `prompt` copied over the tie set."""
    g = load(base)
    r = oracle_argmax(base, prompt)
    rows = tie_rows(kind, r, output_tensor(g).ne[1], prompt)
    return ties(base, out_dir, r, rows), rows
