"""llama-server-compatible HTTP front end over libllmi.so.

The reference launches `/app/llama-server -m PATH --host 127.0.0.1 --port N -c CTX
-ngl NGL --api-key-file FILE [-t THREADS] [EXTRA...]` (scripts/start.sh:473-494),
probes `GET /health` (scripts/start.sh:600-635, scripts/gateway.py:326-376) and
proxies `/v1/*` to it (scripts/gateway.py:699-804).  The gateway sends one request per
TCP connection with `Connection: close` and copies the response until EOF.  This
module answers that contract:

  GET  /health                 200 {"status":"ok"} when ready, 503 while loading (no auth)
  GET  /v1/models              OpenAI model list
  POST /v1/completions         prompt: str | [token ids]; non-stream or SSE
  POST /v1/chat/completions    messages -> chat template -> tokens; non-stream or SSE
  POST /v1/embeddings          501 not_supported_error unless started with --embeddings (the
                               reference starts llama-server without embedding support)
  Authorization: Bearer <key> required on every route but /health when a key is
  configured (401 otherwise; llama-server's public endpoints are /health and /v1/health)

  GET /health adds per-replica serving metrics: active/queued requests, generated
  tokens, tok/s over decode time, HBM GB/s of the last decode call (the gateway passes
  the body through, scripts/gateway.py:360-363)

Sampling follows llama-server (llmi/sampling.py): temperature / top_k / top_p / min_p /
repeat, presence and frequency penalties / seed per request, llama-server's defaults
(temperature 0.8, top_k 40, top_p 0.95, min_p 0.05) or the --temp / --top-k / ... flags;
`stop` strings end the generation (the text stops before them); `ignore_eos` and
`n_predict` follow llama-server; `n` > 1 is rejected with a 400.

Log-probabilities are opt-in: `--max-logprobs N` (LLMI_MAX_LOGPROBS; default 0, at most 20).
With the default every request for them gets a 400, as before; with N > 0

  POST /v1/chat/completions    logprobs: true, top_logprobs: 0..N -> choices[0].logprobs.content =
                               [{token, logprob, bytes, top_logprobs: [{token, logprob, bytes}]}]
  POST /v1/completions         logprobs: k -> choices[0].logprobs = {tokens, token_logprobs,
                               top_logprobs: [{text: logprob}], text_offset}
  POST /completion             n_probs: k -> completion_probabilities: [{id, token, bytes, logprob,
                               top_logprobs: [{id, token, bytes, logprob}]}]

report each generated token's log-probability under the raw distribution (no penalties, no
temperature: llama-server's post_sampling_probs off; llmi/sampling.py token_logprobs) and the
k most likely alternatives; non-finite values are written as -9999.0.  Streamed chunks carry
the entries of the tokens consumed since the previous chunk, and entries end where a stop
string cuts the text.  Requests decoded on the device get them from the device
(llmi_generate_logprobs_batch, still one batched call per step and no logits copy); a
request's first token, requests on the host sampler path, and all of them with
LLMI_DEVICE_SAMPLING=0, from the copied logits.
Greedy requests (temperature 0 or top_k 1, no penalties) decode on the device with
on-device argmax feedback.  Sampled requests within the device sampler's limits (top_k
1..256, a penalty window of at most 256 tokens) join them in the same batched call: the
chain runs on the device logits (llmi_generate_sampled_batch), driven by uniforms drawn
from the request's seeded generator, and only their first token after prefill is sampled
on the host.  Other sampled requests, and all of them with LLMI_DEVICE_SAMPLING=0 (read
when a replica starts; A/B), copy each step's logits to the host sampler.  Every GPU
replica is one llmi Context with `--parallel` sequences (llama-server's slots) driven by
one scheduler thread: requests go to the least-loaded replica and are decoded there
together, one batched step per token for up to 8 sequences (continuous batching,
SURVEY.md §8f row 3).

Prompt cache (llama-server's cache_prompt; opt-in here: `--cache-prompt` or
LLMI_CACHE_PROMPT=1, because it adds a field to `usage`): a replica remembers, for each of
its sequences, the tokens whose KV rows the sequence holds, and a new request prefills only
what differs.  It goes to the free sequence that shares the longest prefix with its prompt
(ties: the least recently used); if another sequence of the replica, free or busy, shares a
longer one, the difference is copied on the device (llama_kv_self_seq_cp, one launch) instead
of prefilled; at least the prompt's last token is always decoded.  A request served from the
cache gets the logits and tokens of the same request served cold, bit for bit.  `cache_prompt:
false` in a request, `--no-cache-prompt` or LLMI_CACHE_PROMPT=0 (the variable is read when a
replica starts and, when set, wins over the flags; A/B) prefill the whole prompt as before.
While the cache is on, responses carry
usage.prompt_tokens_details.cached_tokens (native /completion: tokens_cached) and each
replica's /health entry the totals prompt_tokens and cached_tokens; among equally loaded
replicas a request goes to the one that holds the longest prefix of its prompt.

Embeddings are opt-in, as llama-server's: `--embeddings` (or `--embedding`, LLMI_EMBEDDINGS=1)
and `--pooling none|mean|cls|last` (default: the model's GGUF pooling_type, else none).  Then

  POST /v1/embeddings          input: str | [str] | [token ids] | [[token ids] | str, ...]
  POST /embeddings, /embedding the same (upstream's aliases; `content` is upstream's native
                               spelling of `input`)
      -> {"object":"list","data":[{"object":"embedding","embedding":[...],"index":i}],"model":...,
          "usage":{"prompt_tokens":n,"total_tokens":n}}

An input goes through its replica's scheduler thread like any request: a free sequence is
cleared, ONE llama_decode runs the whole input from position 0 with embeddings switched on
around that call only (the final hidden states are normed and pooled on the device as the
prefill chunks and the last decode step pass, embd.hip), the pooled vector is read, and the
sequence is cleared and released; its prompt-cache entry is forgotten, so embedding inputs
neither use nor feed the prompt cache.  The vector is normalised on the host as upstream's
common_embd_normalize does (llmi/embedding.py; `embd_normalize`: 2 Euclidean, the default, or
-1 none; anything else is a 400); `encoding_format: "base64"` gives little-endian f32.  400
invalid_request_error: an empty input, one longer than the context ("input is too large to
process"), pooling none on /v1/embeddings (not OpenAI compatible; the native routes then
return each token's row, not normalised); 500 as on the other routes when the decode fails.
Each replica's /health entry gains embedding_requests and embedding_tokens.

Text: the GGUF's own tokenizer (SPM or byte-level BPE from tokenizer.ggml.*) and chat
template (tokenizer.chat_template, sandboxed Jinja2), llmi/tokenizer.py; streamed text
holds incomplete UTF-8 sequences back until their last byte.
"""
from __future__ import annotations

import argparse
import base64
import json
import os
import queue
import sys
import threading
import time
import uuid
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer
from typing import Callable, Iterable, Optional

import numpy as np

from .embedding import POOLING_NAMES, normalize
from .sampling import Sampler, SamplingParams, StopFilter, device_eligible, find_stop, parse_stop, token_logprobs

# a greedy slot of a sampled batched call: the chain that is an argmax of the raw logits
_GREEDY = SamplingParams(temperature=0.0, top_k=1, top_p=1.0, min_p=0.0)

VERSION = "llmi-server 0.1 (libllmi, gfx950)"
MAX_LOGPROBS = 20     # llmi.h LLMI_LOGPROBS_MAX_TOP: the most --max-logprobs can allow
LOGPROB_FLOOR = -9999.0  # what JSON carries for a non-finite log-probability (OpenAI's documented floor)


def host_logprob_entry(logits: np.ndarray, token: int, n_top: int) -> tuple:
    """A token's entry (logprob, alternative ids, their logprobs) from a copied logits row."""
    _, ids, lp = token_logprobs(logits, n_top)
    return float(lp[token]), [int(i) for i in ids], [float(lp[i]) for i in ids]


# --------------------------------------------------------------------------------------
# text codecs: the GGUF's tokenizer + chat template (llmi/tokenizer.py), or the legacy
# greedy Vocab (kept for stand-in engines)
# --------------------------------------------------------------------------------------
class _SimpleStream:
    def __init__(self, v):
        self.v = v

    def push(self, t: int) -> str:
        return self.v.detokenize([t])

    def flush(self) -> str:
        return ""


class Vocab:
    """Greedy longest match over token texts (stand-in engines and synthetic vocabularies)."""

    def __init__(self, pieces: list[str], bos: int, eos: int):
        self.bos, self.eos = bos, eos
        self.text = [self._surface(p) for p in pieces]
        self.by_text: dict[str, int] = {}
        for i, t in enumerate(self.text):
            if t and not (pieces[i].startswith("<") and pieces[i].endswith(">")):
                self.by_text.setdefault(t, i)
        self.max_len = max((len(t) for t in self.by_text), default=1)
        self.eog = {eos}

    @property
    def n_vocab(self) -> int:
        return len(self.text)

    @staticmethod
    def _surface(p: str) -> str:
        if len(p) == 6 and p.startswith("<0x") and p.endswith(">"):
            try:
                return chr(int(p[3:5], 16))
            except ValueError:
                return p
        return p.replace("▁", " ").replace("Ġ", " ").replace("Ċ", "\n")

    def detokenize(self, ids: Iterable[int]) -> str:
        return "".join(self.text[i] for i in ids if 0 <= i < len(self.text) and i not in (self.bos, self.eos))

    def tokenize(self, s: str, add_bos: bool = True) -> list[int]:
        out = [self.bos] if add_bos and self.bos >= 0 else []
        i = 0
        while i < len(s):
            for n in range(min(self.max_len, len(s) - i), 0, -1):
                t = self.by_text.get(s[i:i + n])
                if t is not None:
                    out.append(t)
                    i += n
                    break
            else:
                i += 1  # no piece covers this character: skipped
        return out

    def chat_ids(self, messages: list[dict]) -> list[int]:
        return self.tokenize(chat_prompt(messages, self), add_bos=True)

    def stream(self):
        return _SimpleStream(self)


def chat_prompt(messages: list[dict], vocab: Vocab) -> str:
    """Llama-3 header template when the vocabulary has its special tokens, else a
    plain role-prefixed transcript ending with the assistant turn (legacy Vocab only)."""
    if "<|start_header_id|>" in vocab.by_text or any(t == "<|start_header_id|>" for t in vocab.text):
        s = ""
        for m in messages:
            s += f"<|start_header_id|>{m.get('role', 'user')}<|end_header_id|>\n\n{m.get('content', '')}<|eot_id|>"
        return s + "<|start_header_id|>assistant<|end_header_id|>\n\n"
    return "".join(f"{m.get('role', 'user')}: {m.get('content', '')}\n" for m in messages) + "assistant:"


class TextCodec:
    """The GGUF's own tokenizer (SPM / byte-level BPE / greedy for synthetic vocabularies)
    and chat template (tokenizer.chat_template; llama.cpp's chatml default), as
    llama-server applies them: prompts tokenized with parse_special, BOS added unless the
    rendered chat already starts with it, generation stops at any end-of-generation token."""

    EOG_TEXTS = ("<|eot_id|>", "<|eom_id|>", "<|end_of_text|>", "<|im_end|>", "<|endoftext|>", "</s>", "<|end|>")

    def __init__(self, tok, template: Optional[str]):
        from . import tokenizer as T

        self.T = T
        self.tok = tok
        self.template = template
        self.bos, self.eos = tok.bos, tok.eos
        self.bos_text = tok.tokens[tok.bos] if 0 <= tok.bos < tok.n_vocab else ""
        self.eos_text = tok.tokens[tok.eos] if 0 <= tok.eos < tok.n_vocab else ""
        self.eog = {tok.eos} | {tok.by_text[t] for t in self.EOG_TEXTS
                                if t in tok.by_text and tok.types[tok.by_text[t]] == T.CONTROL}
        self.eog.discard(-1)

    @property
    def n_vocab(self) -> int:
        return self.tok.n_vocab

    def tokenize(self, s: str, add_bos: bool = True) -> list[int]:
        return self.tok.tokenize(s, add_special=add_bos, parse_special=True)

    def detokenize(self, ids: Iterable[int]) -> str:
        return self.tok.detokenize(ids)

    def chat_ids(self, messages: list[dict]) -> list[int]:
        for m in messages:
            if not isinstance(m, dict) or not isinstance(m.get("content", ""), str):
                raise ValueError("each message must be an object with string 'content'")
        try:
            text = self.T.render_chat(self.template, messages, self.bos_text, self.eos_text)
        except self.T.TemplateError as e:
            raise ValueError(str(e)) from e
        add_bos = not (self.bos_text and text.startswith(self.bos_text))
        return self.tokenize(text, add_bos=add_bos)

    def stream(self):
        return self.tok.stream()


# --------------------------------------------------------------------------------------
# engine: replicas of one GGUF; each replica = one llmi Context with `slots` sequences,
# driven by one scheduler thread (continuous batching)
# --------------------------------------------------------------------------------------
class Request:
    """One generation: prompt ids in, token lists out through `q` (None terminates).
    `sampling` None or greedy: device argmax; else a Sampler: its chain runs on the device
    fed by its generator's uniforms, or on the host over each step's logits (Replica._step).
    `stop`: strings that end the generation (checked on the detokenized output).
    `n_top` >= 0: every token comes with its log-probability entry (host_logprob_entry's
    shape) in `lp`, parallel to `out`.  `cached`: how many of the prompt's positions the
    replica's prompt cache supplied (set at admission)."""

    def __init__(self, prompt: list[int], max_tokens: int, ignore_eos: bool,
                 sampling: Optional[SamplingParams] = None, stop: Optional[list[str]] = None, n_top: int = -1,
                 cache_prompt: bool = True):
        self.prompt, self.max_tokens, self.ignore_eos = list(prompt), max_tokens, ignore_eos
        self.n_top = n_top
        self.cache_prompt = cache_prompt  # False: the whole prompt is prefilled (llama-server's field)
        self.cached = 0                   # prompt positions served from the replica's prompt cache
        self.lp: list[tuple] = []
        self.sampler = Sampler(sampling) if sampling is not None and not sampling.greedy else None
        self.stop = list(stop or [])
        self.out: list[int] = []
        self.q: "queue.Queue" = queue.Queue()
        self.finish: Optional[str] = None
        self.error: Optional[str] = None
        self.t_submit = time.perf_counter()
        self.t_first: Optional[float] = None
        self.replica = -1
        # scheduler state
        self.seq = -1
        self.last = -1
        self.pos = 0

    def emit(self, toks: list[int], entries: Optional[list[tuple]] = None) -> None:
        if toks:
            if self.t_first is None:
                self.t_first = time.perf_counter()
            self.out += toks
            if self.n_top >= 0:  # before the tokens are announced: a reader of q finds them in lp
                self.lp += entries[:len(toks)]
            self.q.put(list(toks))

    def done(self, finish: str) -> None:
        self.finish = finish
        self.q.put(None)

    def fail(self, err: str) -> None:
        self.error = err
        self.q.put(None)


class EmbedRequest:
    """One embedding input: token ids in, through `q` the pooled vector (pooling none: the
    tokens' rows) or None with `error` set."""

    def __init__(self, tokens: list[int]):
        self.tokens = list(tokens)
        self.q: "queue.Queue" = queue.Queue()
        self.error: Optional[str] = None
        self.replica = -1

    def fail(self, err: str) -> None:
        self.error = err
        self.q.put(None)


def _common_prefix(a: list[int], b: list[int]) -> int:
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    i = 0
    while a[i] == b[i]:
        i += 1
    return i


class Replica:
    """One context (device) serving up to `slots` requests at once.  Its thread admits
    queued requests into free sequences (prefill through llama_decode with their seq id)
    and advances all active ones together with llmi_generate_greedy_batch (one weight
    stream per step for up to 8 sequences), `chunk` tokens per call.  With the prompt cache
    (cache_prompt) it keeps what each sequence holds and prefills only what a prompt adds."""

    def __init__(self, idx: int, ctx, slots: int, eog: set, chunk: int, n_ctx: int, device: int = 0,
                 detok: Optional[Callable[[list[int]], str]] = None, cache_prompt: bool = False):
        self.idx, self.ctx, self.slots, self.eog, self.chunk, self.n_ctx = idx, ctx, slots, eog, chunk, n_ctx
        self.device = device
        self.detok = detok
        self.pending: "queue.Queue[Request]" = queue.Queue()
        self.active: list[Request] = []
        self.free = list(range(slots))
        self.lock = threading.Lock()
        self.n_queued = 0
        self.tokens = 0          # generated tokens served
        self.busy_s = 0.0        # time inside decode calls
        self.last_gbps = 0.0     # HBM GB/s of the last decode call (algorithmic bytes / device time)
        self.requests = 0
        self.stop = False
        # device sampling: the context has the call, and LLMI_DEVICE_SAMPLING is not 0
        self.device_sampling = hasattr(ctx, "generate_sampled_batch") and os.environ.get("LLMI_DEVICE_SAMPLING", "1") != "0"
        # device log-probabilities: the same, and the context has that call too
        self.device_logprobs = self.device_sampling and hasattr(ctx, "generate_logprobs_batch")
        # prompt cache: asked for (--cache-prompt; LLMI_CACHE_PROMPT, when set, decides instead:
        # 0 off, else on), and the context can copy between sequences
        env = os.environ.get("LLMI_CACHE_PROMPT")
        self.cache_prompt = (cache_prompt if env is None else env != "0") and hasattr(ctx, "seq_cp")
        # per sequence: the tokens whose KV rows it holds (never more than what was fed), and
        # when it was last admitted into or released (the scheduler's admission count)
        self.held: list[list[int]] = [[] for _ in range(slots)]
        self.used = [0] * slots
        self.tick = 0
        self.prompt_tokens = 0   # prompt tokens admitted / of them served from the cache
        self.cached_tokens = 0
        self.embedding_requests = 0  # embedding inputs served / their tokens
        self.embedding_tokens = 0
        self.th = threading.Thread(target=self._run, name=f"llmi-replica-{idx}", daemon=True)
        self.th.start()

    def load(self) -> int:
        with self.lock:
            return self.n_queued + len(self.active)

    def submit(self, r) -> None:
        with self.lock:
            self.n_queued += 1
            self.requests += 1
        r.replica = self.idx
        self.pending.put(r)

    def _stats(self) -> None:
        try:
            b, us = self.ctx.stats()
            if us > 0:
                self.last_gbps = b / (us * 1e-6) / 1e9
        except Exception:
            pass

    # -- the prompt cache's bookkeeping
    def prefix_len(self, prompt: list[int]) -> int:
        """The longest prefix of prompt that one of this replica's sequences holds."""
        with self.lock:
            return max(_common_prefix(prompt, h) for h in self.held)

    def _touch(self, seq: int) -> None:
        self.tick += 1
        self.used[seq] = self.tick

    def _remember(self, r: Request) -> None:
        """r's sequence holds (r.prompt + r.out)[:r.pos]: tokens a chunk fed past the
        request's end are not part of it."""
        if not self.cache_prompt:
            return
        n = min(r.pos, len(r.prompt) + len(r.out)) - len(r.prompt)
        with self.lock:
            h = self.held[r.seq]
            h += r.out[len(h) - len(r.prompt):n]

    def _forget(self, seq: int) -> None:
        with self.lock:
            self.held[seq] = []

    def _release(self, r: Request) -> None:
        self._touch(r.seq)
        self.free.append(r.seq)

    def _place(self, r: Request) -> tuple[int, int, int, int]:
        """Takes the free sequence r goes to off the free list: the one sharing the longest
        prefix with its prompt (ties: least recently used, then the last of the free list).
        Returns it, the length of that prefix, and the sequence of this replica (free or
        decoding) that shares the longest prefix of all, with its length.  (cache_prompt
        false: the sequence the request always went to, nothing shared.)"""
        if not r.cache_prompt:
            return self.free.pop(), 0, -1, 0
        lens = [_common_prefix(r.prompt, h) for h in self.held]
        seq = max(self.free, key=lambda s: (lens[s], -self.used[s], self.free.index(s)))
        self.free.remove(seq)
        t = max(range(self.slots), key=lambda s: (lens[s], -s))
        return seq, lens[seq], t, lens[t]

    # -- an embedding input: one decode of the whole input in a free sequence, then release
    def _embed(self, r: EmbedRequest) -> None:
        with self.lock:
            self.n_queued -= 1
        seq = self.free.pop()
        try:
            c, n = self.ctx, len(r.tokens)
            # the sequence starts empty and ends empty; what it held is not there afterwards
            self._forget(seq)
            c.seq_rm(seq)
            t0 = time.perf_counter()
            c.set_embeddings(True)
            try:
                rc = c.decode(r.tokens, pos=list(range(n)), seq=[seq] * n)
                if rc != 0:
                    raise RuntimeError(f"llama_decode returned {rc}")
                if c.pooling == POOLING_NAMES["none"]:
                    vec = np.stack([c.embeddings_ith(i) for i in range(n)])
                else:
                    vec = c.embeddings_seq(seq)
            finally:
                c.set_embeddings(False)
                self.busy_s += time.perf_counter() - t0
            c.seq_rm(seq)
            self.embedding_requests += 1
            self.embedding_tokens += n
            r.q.put(vec)
        except Exception as e:  # this input fails; the replica keeps serving
            r.fail(str(e))
        finally:
            self._touch(seq)
            self.free.append(seq)

    # -- admission: prefill into a free sequence, emit the first token
    def _admit(self, r) -> None:
        if isinstance(r, EmbedRequest):
            return self._embed(r)
        with self.lock:
            self.n_queued -= 1
        cache = self.cache_prompt
        seq = -1
        try:
            c = self.ctx
            if not cache:
                seq, have = self.free.pop(), 0
                c.seq_rm(seq)
            max_tokens = r.max_tokens
            if len(r.prompt) + max_tokens > self.n_ctx:
                max_tokens = max(0, self.n_ctx - len(r.prompt))
            r.max_tokens = max_tokens
            if not r.prompt or max_tokens <= 0:
                if seq >= 0:
                    self.free.append(seq)
                r.done("length")
                return
            if cache:
                seq, have, t, upto = self._place(r)
                # another sequence holds more of the prompt: the difference is copied on the
                # device.  t may be decoding: its prefix rows are stable, and this thread alone
                # uses the context.  (A refused copy leaves seq as it was: prefilled instead.)
                if upto > have and len(r.prompt) > 1 and c.seq_cp(t, seq, have, upto):
                    have = upto
                    with self.lock:
                        self.held[seq] = list(r.prompt[:have])
            # at least the last token is decoded: the first token is sampled from its logits
            n = min(have, len(r.prompt) - 1)
            if cache:
                self._touch(seq)
                self._forget(seq)  # until the decode below has succeeded
                c.seq_rm(seq, n, -1) if n > 0 else c.seq_rm(seq)
            t0 = time.perf_counter()
            if n > 0:
                rc = c.decode(r.prompt[n:], pos=list(range(n, len(r.prompt))), seq=[seq] * (len(r.prompt) - n))
            else:
                rc = c.decode(r.prompt, seq=[seq] * len(r.prompt))
            self.busy_s += time.perf_counter() - t0
            if rc != 0:
                raise RuntimeError(f"llama_decode returned {rc}")
            first = c.greedy(-1) if r.sampler is None else r.sampler.sample(c.logits(-1), r.prompt)
            # the first token's entry: from the prompt's logits on the host, on every path
            entries = [host_logprob_entry(c.logits(-1), first, r.n_top)] if r.n_top >= 0 else None
            r.seq, r.pos = seq, len(r.prompt)
            if cache:
                r.cached = n
                with self.lock:
                    self.held[seq] = list(r.prompt)
                    self.prompt_tokens += len(r.prompt)
                    self.cached_tokens += n
            if self._take(r, [first], entries):
                self._release(r)
            else:
                r.last = first
                self.active.append(r)
        except Exception as e:  # this request fails; the replica keeps serving
            if seq >= 0:
                self._forget(seq)
                self.free.append(seq)
            r.fail(str(e))

    def _take(self, r: Request, toks: list[int], entries: Optional[list[tuple]] = None) -> bool:
        """Emit generated tokens (with their logprob entries, toks' parallel) up to EOS /
        max_tokens; True when the request is done."""
        emit = []
        for t in toks:
            if t in self.eog and not r.ignore_eos:
                r.emit(emit, entries)
                self.tokens += len(emit)
                r.done("stop")
                return True
            emit.append(t)
            if len(r.out) + len(emit) >= r.max_tokens:
                break
        r.emit(emit, entries)
        self.tokens += len(emit)
        if r.stop and self.detok is not None and emit and self._stop_seen(r, len(emit)):
            r.done("stop")
            return True
        if len(r.out) >= r.max_tokens:
            r.done("length")
            return True
        return False

    def _stop_seen(self, r: Request, n_new: int) -> bool:
        """Did the n_new tokens just emitted complete a stop string?  Earlier text was
        checked when it was new, so only a window is detokenized: the new tokens plus
        enough older ones to hold a stop string that starts before them (every token is at
        least one byte, so max(len(stop)) + 4 tokens cover any stop string plus a split
        UTF-8 sequence) -- O(1) per call instead of the whole output."""
        tail = max(len(x.encode("utf-8")) for x in r.stop) + 4
        return find_stop(self.detok(r.out[-(n_new + tail):]), r.stop) is not None

    def _step(self) -> None:
        batch = self.active[:8]
        k = max(1, min(self.chunk, min(r.max_tokens - len(r.out) for r in batch)))
        if any(r.stop for r in batch):
            k = min(k, 4)  # stop strings are checked between decode calls
        c = self.ctx
        t0 = time.perf_counter()
        # a request that wants log-probabilities where the device cannot give them (no such
        # call on this context, LLMI_DEVICE_SAMPLING=0, a chain outside the device limits)
        # takes the host path below, greedy ones included: its entries come from copied logits
        hostlp = [r for r in batch if r.n_top >= 0 and not (
            self.device_logprobs and (r.sampler is None or device_eligible(r.sampler.p)))]
        greedy = [r for r in batch if r.sampler is None and r not in hostlp]
        ondev = [r for r in batch if r.sampler is not None and self.device_sampling and device_eligible(r.sampler.p)
                 and r not in hostlp]
        sampled = [r for r in batch if r not in greedy and r not in ondev]
        outs: dict[int, list[int]] = {}
        lps: dict[int, list[tuple]] = {}
        want_lp = any(r.n_top >= 0 for r in greedy + ondev)
        if ondev or want_lp:
            # sampled requests within the device sampler's limits and the greedy ones advance
            # k tokens in one call (one weight pass per step for all of them): each sampled
            # request's chain runs on the device logits, fed the next k draws of its own
            # generator -- the draws the host path would make, so a seed gives the same text
            # on either path (draws past a request's end are discarded with it).  If any of
            # them wants log-probabilities the call is the one that computes them next to the
            # sampler, with -1 for the others: still one call and one weight pass
            group = greedy + ondev
            params = [_GREEDY] * len(greedy) + [r.sampler.p for r in ondev]
            unis = [np.zeros(k)] * len(greedy) + [r.sampler.rng.random(k) if r.sampler.p.temperature > 0.0 else np.zeros(k)
                                                  for r in ondev]

            def call(rs, ps, us):
                seqs, last, pos = [r.seq for r in rs], [r.last for r in rs], [r.pos for r in rs]
                if want_lp:
                    return c.generate_logprobs_batch(seqs, last, pos, k, ps, us, [r.n_top for r in rs])
                return c.generate_sampled_batch(seqs, last, pos, k, ps, us), [None] * len(rs)

            try:
                got, ent = call(group, params, unis)
            except Exception:  # not batchable here: one sequence at a time, same results
                one = [call([r], [p], [u]) for r, p, u in zip(group, params, unis)]
                got, ent = [o[0][0] for o in one], [o[1][0] for o in one]
            for r, toks, e in zip(group, got, ent):
                outs[id(r)] = toks
                if e is not None:
                    lps[id(r)] = e
        elif greedy:
            # greedy slots decode k tokens per call with the argmax fed back on the device,
            # whether or not sampled requests share the replica
            try:
                got = c.generate_greedy_batch([r.seq for r in greedy], [r.last for r in greedy],
                                              [r.pos for r in greedy], k)
            except Exception:
                # not batchable here (e.g. a context past the batched attention's bound):
                # one sequence at a time, same results
                got = [c.generate_greedy_batch([r.seq], [r.last], [r.pos], k)[0] for r in greedy]
            for r, toks in zip(greedy, got):
                outs[id(r)] = toks
        if sampled:
            # one token per call: every sampled slot's logits (llama_decode with one token
            # per sequence = one batched step), sampled on the host
            rc = c.decode([r.last for r in sampled], pos=[r.pos for r in sampled], seq=[r.seq for r in sampled],
                          logits_all=True)
            if rc != 0:
                raise RuntimeError(f"llama_decode returned {rc}")
            for i, r in enumerate(sampled):
                lg = c.logits(i)
                # (a greedy request is here for its entries only: first max wins, as on the device)
                tok = int(np.argmax(lg)) if r.sampler is None else r.sampler.sample(lg, r.prompt + r.out)
                outs[id(r)] = [tok]
                if r.n_top >= 0:
                    lps[id(r)] = [host_logprob_entry(lg, tok, r.n_top)]
        self.busy_s += time.perf_counter() - t0
        self._stats()
        done = []
        for r in batch:
            toks = outs[id(r)]
            r.pos += len(toks)
            r.last = toks[-1]
            fin = self._take(r, toks, lps.get(id(r)))
            self._remember(r)
            if fin:
                done.append(r)
        for r in done:
            self.active.remove(r)
            self._release(r)
        # rotate so more than 8 active requests share the steps fairly
        if len(self.active) > 8:
            self.active = self.active[len(batch):] + self.active[:len(batch)]

    def _run(self) -> None:
        while not self.stop:
            try:
                while self.free and (not self.pending.empty() or not self.active):
                    r = self.pending.get(timeout=0.5 if not self.active else None) if not self.active else \
                        self.pending.get_nowait()
                    self._admit(r)
            except queue.Empty:
                pass
            if not self.active:
                continue
            try:
                self._step()
            except Exception as e:  # the context failed: every active request fails
                for r in self.active:
                    self._forget(r.seq)  # its rows are not to be trusted
                    r.fail(str(e))
                    self.free.append(r.seq)
                self.active = []


class Engine:
    """Owns the GPU replicas.  Requests go to the least-loaded replica (active + queued;
    ties to the one whose prompt cache holds the longest prefix of the prompt, then to the
    lowest index) and are served there with continuous batching."""

    def __init__(self, path: str, n_ctx: int, n_gpu_layers: int, devices: list[int], slots: int = 4,
                 chunk: int = 8, contexts=None, sampling: Optional[SamplingParams] = None, numerics: int = 0,
                 max_logprobs: int = 0, cache_prompt: bool = False, embeddings: bool = False,
                 pooling: Optional[int] = None):
        self.path, self.n_ctx, self.ngl, self.devices = path, n_ctx, n_gpu_layers, devices
        # /v1/embeddings (--embeddings; off: the routes answer 501) and the pooling type
        # (--pooling; None: the model's own, known once the contexts exist)
        self.embeddings = bool(embeddings)
        self.pooling = pooling
        # the replicas' prompt cache (--cache-prompt); whether it is active is decided per
        # replica when it starts (Replica.cache_prompt), see prompt_cache
        self.cache_prompt = cache_prompt
        # alternatives a request may ask for (--max-logprobs); 0: logprobs are refused with a 400
        self.max_logprobs = max(0, min(int(max_logprobs), MAX_LOGPROBS))
        self.numerics = numerics  # llmi.NUMERICS_GENERIC / NUMERICS_X86
        self.sampling = sampling or SamplingParams()  # server defaults (llama-server's)
        self.slots, self.chunk = max(1, slots), max(1, chunk)
        self.ready = False
        self.error: Optional[str] = None
        self.vocab = None
        self.model_id = os.path.basename(path)
        self.replicas: list[Replica] = []
        self._models = []
        self._contexts = contexts  # test hook: (list of context-like objects, codec)
        self.t_ready: Optional[float] = None
        self.load_s = 0.0

    def load(self) -> None:
        t0 = time.perf_counter()
        try:
            if self._contexts is not None:
                ctxs, self.vocab = self._contexts
            else:
                import llmi
                from . import tokenizer as T

                if len(self.devices) > 1:  # replicas: RCCL pieces pipelined behind the upload
                    m0, reps = llmi.Model.load_replicated(self.path, self.devices[0], self.devices[1:],
                                                          n_gpu_layers=self.ngl, numerics=self.numerics)
                else:
                    m0, reps = llmi.Model(self.path, n_gpu_layers=self.ngl, main_gpu=self.devices[0],
                                          numerics=self.numerics), []
                models = [m0] + reps
                self._models = models
                ctxs = [llmi.Context(m, n_ctx=self.n_ctx, n_seq=self.slots) for m in models]
                self.n_ctx = ctxs[0].n_ctx
                meta = T.read_gguf_meta(self.path)
                tok = T.make_tokenizer(meta, tokens=[m0.token_text(i) for i in range(m0.n_vocab)],
                                       bos=m0.bos, eos=m0.eos) if not meta.get("tokenizer.ggml.tokens") \
                    else T.make_tokenizer(meta)
                self.vocab = TextCodec(tok, meta.get("tokenizer.chat_template"))
            if self.embeddings:
                if self.pooling is not None:
                    for c in ctxs:
                        c.set_pooling(self.pooling)
                self.pooling = int(ctxs[0].pooling)
            eog = getattr(self.vocab, "eog", {self.vocab.eos})
            detok = getattr(self.vocab, "detokenize", None)
            self.replicas = [Replica(i, c, self.slots, eog, self.chunk, self.n_ctx,
                                     self.devices[i] if i < len(self.devices) else i, detok, self.cache_prompt)
                             for i, c in enumerate(ctxs)]
            self.load_s = time.perf_counter() - t0
            self.t_ready = time.perf_counter()
            self.ready = True
        except Exception as e:  # reported by /health
            self.error = str(e)

    def submit(self, prompt: list[int], max_tokens: int, ignore_eos: bool,
               sampling: Optional[SamplingParams] = None, stop: Optional[list[str]] = None, n_top: int = -1,
               cache_prompt: bool = True) -> Request:
        r = Request(prompt, max_tokens, ignore_eos, sampling, stop, n_top, cache_prompt)
        loads = [x.load() for x in self.replicas]
        tied = [x for x, n in zip(self.replicas, loads) if n == min(loads)]
        if len(tied) > 1 and cache_prompt and self.prompt_cache:
            rep = min(tied, key=lambda x: (-(x.prefix_len(r.prompt) if x.cache_prompt else 0), x.idx))
        else:
            rep = tied[0]
        rep.submit(r)
        return r

    def embed(self, tokens: list[int]) -> np.ndarray:
        """One embedding input on the least-loaded replica: its pooled vector, not normalised
        (pooling none: the tokens' rows [n][n_embd])."""
        r = EmbedRequest(tokens)
        min(self.replicas, key=lambda x: (x.load(), x.idx)).submit(r)
        vec = r.q.get()
        if r.error:
            raise RuntimeError(r.error)
        return vec

    @property
    def prompt_cache(self) -> bool:
        """Is the prompt cache active on a replica?  (Then responses report cached tokens.)"""
        return any(x.cache_prompt for x in self.replicas)

    def run(self, prompt: list[int], max_tokens: int, ignore_eos: bool,
            on_tokens: Callable[[list[int], Optional[list[tuple]]], None], sampling: Optional[SamplingParams] = None,
            stop: Optional[list[str]] = None, n_top: int = -1, cache_prompt: bool = True) -> Request:
        """Serve one request to its end, handing its tokens (and, with n_top >= 0, their logprob
        entries) to on_tokens as they come; returns the finished Request (out, finish, lp, cached)."""
        r = self.submit(prompt, max_tokens, ignore_eos, sampling, stop, n_top, cache_prompt)
        seen = 0
        while True:
            toks = r.q.get()
            if toks is None:
                break
            on_tokens(toks, r.lp[seen:seen + len(toks)] if n_top >= 0 else None)
            seen += len(toks)
        if r.error:
            raise RuntimeError(r.error)
        return r

    def generate(self, prompt: list[int], max_tokens: int, ignore_eos: bool, on_tokens: Callable[[list[int]], None],
                 chunk: int = 8, sampling: Optional[SamplingParams] = None,
                 stop: Optional[list[str]] = None) -> tuple[list[int], str]:
        ids, finish, _ = self.generate_logprobs(prompt, max_tokens, ignore_eos, lambda toks, _e: on_tokens(toks), chunk,
                                                sampling, stop, -1)
        return ids, finish

    def generate_logprobs(self, prompt: list[int], max_tokens: int, ignore_eos: bool,
                          on_tokens: Callable[[list[int], Optional[list[tuple]]], None], chunk: int = 8,
                          sampling: Optional[SamplingParams] = None, stop: Optional[list[str]] = None,
                          n_top: int = -1) -> tuple[list[int], str, list[tuple]]:
        """generate with each token's logprob entry (n_top >= 0; else None) handed to
        on_tokens along with the tokens; returns (tokens, finish, entries)."""
        r = self.run(prompt, max_tokens, ignore_eos, on_tokens, sampling, stop, n_top)
        return r.out, r.finish or "length", r.lp

    def health(self) -> dict:
        """Per-replica serving metrics for /health (kept well under the gateway's 4 KB read,
        scripts/gateway.py:350)."""
        up = max(1e-9, time.perf_counter() - (self.t_ready or time.perf_counter()))
        reps = []
        for r in self.replicas:
            reps.append({"id": r.idx, "device": r.device, "active": len(r.active), "queued": r.n_queued,
                         "tokens": r.tokens, "tok_s": round(r.tokens / max(r.busy_s, 1e-9), 1) if r.tokens else 0.0,
                         "hbm_gbps": round(r.last_gbps, 1), "busy": round(r.busy_s / up, 3)})
            if r.cache_prompt:
                reps[-1].update(prompt_tokens=r.prompt_tokens, cached_tokens=r.cached_tokens)
            if self.embeddings:
                reps[-1].update(embedding_requests=r.embedding_requests, embedding_tokens=r.embedding_tokens)
        busy = sum(len(r.active) for r in self.replicas)
        return {"slots_idle": self.slots * len(self.replicas) - busy, "slots_processing": busy,
                "load_s": round(self.load_s, 2), "replicas": reps[:16]}


# --------------------------------------------------------------------------------------
# HTTP
# --------------------------------------------------------------------------------------
def _error(code: int, msg: str, typ: str) -> dict:
    return {"error": {"message": msg, "type": typ, "code": code}}


class Handler(BaseHTTPRequestHandler):
    protocol_version = "HTTP/1.1"
    server_version = "llmi-server"
    engine: Engine = None  # set by make_server
    api_key: Optional[str] = None

    def log_message(self, fmt, *args):  # quiet; the gateway logs requests
        if os.environ.get("LLMI_SERVER_LOG"):
            sys.stderr.write("[llmi-server] " + fmt % args + "\n")

    # ---- plumbing
    def _send_json(self, code: int, obj: dict) -> None:
        body = json.dumps(obj).encode()
        self.send_response(code)
        self.send_header("Content-Type", "application/json")
        self.send_header("Content-Length", str(len(body)))
        self.send_header("Connection", "close")
        self.end_headers()
        self.wfile.write(body)
        self.close_connection = True

    PUBLIC = ("/health", "/v1/health")

    def _authorized(self, route: str) -> bool:
        if not self.api_key or route in self.PUBLIC:
            return True
        return self.headers.get("Authorization", "") == f"Bearer {self.api_key}"

    def _body(self) -> Optional[dict]:
        n = int(self.headers.get("Content-Length") or 0)
        raw = self.rfile.read(n) if n > 0 else b""
        try:
            return json.loads(raw or b"{}")
        except json.JSONDecodeError:
            return None

    @staticmethod
    def _logprobs_wanted(req: dict, route: str, limit: int) -> int:
        """The alternatives a request asks for with its route's fields (-1: no logprobs);
        ValueError for what the route or the server's --max-logprobs does not take."""
        def count(name):
            v = req.get(name)
            if v is None:
                return None
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"'{name}' must be a non-negative integer")
            return v

        n = -1
        if route == "/v1/chat/completions":
            lp = req.get("logprobs")
            if lp == 0 and lp is not None:
                lp = False  # (0 has always been taken for false here)
            if lp not in (None, False) and lp is not True:
                raise ValueError("'logprobs' must be a boolean")
            top = count("top_logprobs")
            if top is not None and not lp:
                raise ValueError("'top_logprobs' requires 'logprobs' to be true")
            if lp:
                n = top or 0
        else:
            if req.get("top_logprobs") not in (None, 0):
                raise ValueError("'top_logprobs' belongs to /v1/chat/completions; this route takes 'logprobs': k")
            lp = req.get("logprobs")
            k = None if lp is False else 0 if lp is True else count("logprobs")
            if route == "/completion" and count("n_probs"):
                k = max(k or 0, count("n_probs"))
            if k is not None and (k > 0 or lp is True or limit > 0):
                n = k  # (logprobs: 0 on a server without --max-logprobs stays what it was: nothing)
        if n >= 0 and limit <= 0:
            raise ValueError("logprobs are not supported (the server runs without --max-logprobs)")
        if n > limit:
            raise ValueError(f"at most {limit} top logprobs are served (--max-logprobs {limit})")
        return n

    def _logprob_json(self, route: str, ids: list[int], entries: list[tuple], starts: list[int]) -> dict:
        """The route's response fields for tokens `ids` with their entries and text offsets."""
        v = self.engine.vocab
        fin = lambda x: float(x) if np.isfinite(x) else LOGPROB_FLOOR  # noqa: E731
        text = lambda t: v.detokenize([t])  # noqa: E731
        raw = lambda t: list(text(t).encode("utf-8"))  # noqa: E731
        if route == "/v1/chat/completions":
            return {"logprobs": {"content": [
                {"token": text(t), "logprob": fin(lp), "bytes": raw(t),
                 "top_logprobs": [{"token": text(a), "logprob": fin(x), "bytes": raw(a)} for a, x in zip(alt, alp)]}
                for t, (lp, alt, alp) in zip(ids, entries)]}}
        out = {"logprobs": {"tokens": [text(t) for t in ids], "token_logprobs": [fin(e[0]) for e in entries],
                            "top_logprobs": [{text(a): fin(x) for a, x in zip(alt, alp)} for _, alt, alp in entries],
                            "text_offset": list(starts)}}
        if route == "/completion":
            out["completion_probabilities"] = [
                {"id": t, "token": text(t), "bytes": raw(t), "logprob": fin(lp),
                 "top_logprobs": [{"id": a, "token": text(a), "bytes": raw(a), "logprob": fin(x)} for a, x in zip(alt, alp)]}
                for t, (lp, alt, alp) in zip(ids, entries)]
        return out

    def _embedding_inputs(self, req: dict) -> list[list[int]]:
        """The request's inputs as token lists; ValueError for what the route does not take."""
        v = self.engine.vocab
        inp = req.get("input", req.get("content"))
        is_ids = lambda x: isinstance(x, list) and bool(x) and all(  # noqa: E731
            isinstance(t, int) and not isinstance(t, bool) for t in x)
        if isinstance(inp, str) or is_ids(inp):
            items = [inp]
        elif isinstance(inp, list) and inp and all(isinstance(x, str) or is_ids(x) for x in inp):
            items = inp
        else:
            raise ValueError("'input' must be a non-empty string, a list of strings, a list of token ids or a list of those")
        out = []
        for x in items:
            ids = v.tokenize(x, add_bos=True) if isinstance(x, str) else list(x)
            if not x or not ids:
                raise ValueError("'input' is empty")
            if not (0 <= min(ids) and max(ids) < v.n_vocab):
                raise ValueError("token ids out of range")
            if len(ids) > self.engine.n_ctx:
                raise ValueError(f"input is too large to process ({len(ids)} tokens, the context holds "
                                 f"{self.engine.n_ctx}); increase the context size")
            out.append(ids)
        return out

    def _embeddings(self, route: str):
        eng = self.engine
        # the reference launches llama-server without embedding support (start.sh passes no
        # --embeddings; docs/API_REFERENCE.md:537-540 "only available if ... started with
        # embedding support"): upstream then answers 501 not_supported_error
        if not getattr(eng, "embeddings", False):
            return self._send_json(501, _error(
                501, "This server does not support embeddings. Start it with `--embeddings`", "not_supported_error"))
        if not eng.ready:
            return self._send_json(503, _error(503, "Loading model", "unavailable_error"))
        req = self._body()
        if req is None or not isinstance(req, dict):
            return self._send_json(400, _error(400, "invalid JSON body", "invalid_request_error"))
        none = getattr(eng, "pooling", POOLING_NAMES["mean"]) == POOLING_NAMES["none"]
        try:
            if none and route == "/v1/embeddings":
                raise ValueError("Pooling type 'none' is not OAI compatible. Please use a different pooling type")
            inputs = self._embedding_inputs(req)
            norm = req.get("embd_normalize", 2)
            if isinstance(norm, bool) or norm not in (2, -1):
                raise ValueError("'embd_normalize' must be 2 (euclidean) or -1 (none)")
            fmt = req.get("encoding_format", "float")
            if fmt not in ("float", "base64"):
                raise ValueError("'encoding_format' must be \"float\" or \"base64\"")
        except (ValueError, TypeError) as e:
            return self._send_json(400, _error(400, str(e), "invalid_request_error"))

        def encode(vec: np.ndarray):
            vec = np.ascontiguousarray(vec, dtype="<f4")
            if fmt == "base64":
                return base64.b64encode(vec.tobytes()).decode("ascii")
            return vec.tolist()
        data = []
        try:
            for i, ids in enumerate(inputs):
                vec = np.asarray(eng.embed(ids), dtype=np.float32)
                # pooling none (native routes only): each token's row, as it is (upstream's)
                emb = [encode(row) for row in vec] if none else encode(normalize(vec, norm))
                data.append({"object": "embedding", "embedding": emb, "index": i})
        except Exception as e:  # a failed llama_decode: OpenAI-shaped 500, not a dropped socket
            return self._send_json(500, _error(500, str(e), "server_error"))
        n = sum(len(ids) for ids in inputs)
        return self._send_json(200, {"object": "list", "data": data, "model": req.get("model") or eng.model_id,
                                     "usage": {"prompt_tokens": n, "total_tokens": n}})

    # ---- routes
    def do_GET(self):
        eng = self.engine
        route = self.path.split("?")[0]
        if route in self.PUBLIC:
            if eng.error:
                return self._send_json(500, {"status": "error", "error": eng.error})
            if not eng.ready:
                return self._send_json(503, _error(503, "Loading model", "unavailable_error"))
            h = {"status": "ok"}
            if hasattr(eng, "health"):
                h.update(eng.health())
            return self._send_json(200, h)
        if not self._authorized(route):
            return self._send_json(401, _error(401, "Invalid API Key", "authentication_error"))
        if route == "/v1/models":
            return self._send_json(200, {"object": "list", "data": [
                {"id": eng.model_id, "object": "model", "created": int(time.time()), "owned_by": "llmi"}]})
        return self._send_json(404, _error(404, "File Not Found", "not_found_error"))

    def do_POST(self):
        eng = self.engine
        route = self.path.split("?")[0]
        if not self._authorized(route):
            return self._send_json(401, _error(401, "Invalid API Key", "authentication_error"))
        if route in ("/v1/embeddings", "/embeddings", "/embedding"):
            return self._embeddings(route)
        if route not in ("/v1/completions", "/v1/chat/completions", "/completion"):
            return self._send_json(404, _error(404, "File Not Found", "not_found_error"))
        if not eng.ready:
            return self._send_json(503, _error(503, "Loading model", "unavailable_error"))
        req = self._body()
        if req is None:
            return self._send_json(400, _error(400, "invalid JSON body", "invalid_request_error"))
        chat = route == "/v1/chat/completions"
        v = eng.vocab
        try:
            if chat:
                msgs = req.get("messages")
                if not isinstance(msgs, list) or not msgs:
                    raise ValueError("'messages' must be a non-empty list")
                prompt = v.chat_ids(msgs)
            else:
                p = req.get("prompt", "")
                if isinstance(p, list) and all(isinstance(t, int) for t in p):
                    prompt = list(p)
                    if not prompt or not (0 <= min(prompt) and max(prompt) < v.n_vocab):
                        raise ValueError("token ids out of range")
                elif isinstance(p, str):
                    prompt = v.tokenize(p, add_bos=True)
                else:
                    raise ValueError("'prompt' must be a string or a list of token ids")
            max_tokens = int(req.get("max_tokens", req.get("n_predict", 16 if not chat else 256)))
            if max_tokens < 0:
                max_tokens = eng.n_ctx
            if int(req.get("n", 1)) != 1:
                raise ValueError("only n = 1 is supported")
            n_top = self._logprobs_wanted(req, route, getattr(eng, "max_logprobs", 0))
            sampling = getattr(eng, "sampling", SamplingParams()).with_request(req)
            stop = parse_stop(req.get("stop"))
            cache_prompt = req.get("cache_prompt", True)
            if not isinstance(cache_prompt, bool):
                raise ValueError("'cache_prompt' must be a boolean")
        except (ValueError, TypeError) as e:
            return self._send_json(400, _error(400, str(e), "invalid_request_error"))
        # the prompt cache is on: the engine's run() also tells how much of the prompt it served
        cache_on = bool(getattr(eng, "prompt_cache", False))

        def usage(n_out: int, cached: Optional[int]) -> dict:
            u = {"prompt_tokens": len(prompt), "completion_tokens": n_out, "total_tokens": len(prompt) + n_out}
            if cached is not None:
                u["prompt_tokens_details"] = {"cached_tokens": cached}
            return u
        ignore_eos = bool(req.get("ignore_eos", False))
        stream = bool(req.get("stream", False))
        rid = ("chatcmpl-" if chat else "cmpl-") + uuid.uuid4().hex[:24]
        created = int(time.time())
        obj = "chat.completion" if chat else "text_completion"
        if not stream:
            entries, cached = None, None
            try:
                if cache_on:
                    r = eng.run(prompt, max_tokens, ignore_eos, lambda _t, _e: None, sampling=sampling, stop=stop,
                                n_top=n_top, cache_prompt=cache_prompt)
                    ids, finish, cached = r.out, r.finish or "length", r.cached
                    entries = r.lp if n_top >= 0 else None
                elif n_top >= 0:
                    ids, finish, entries = eng.generate_logprobs(prompt, max_tokens, ignore_eos, lambda _t, _e: None,
                                                                 chunk=32, sampling=sampling, stop=stop, n_top=n_top)
                else:
                    ids, finish = eng.generate(prompt, max_tokens, ignore_eos, lambda _t: None, chunk=32,
                                               sampling=sampling, stop=stop)
            except Exception as e:  # a failed llama_decode: OpenAI-shaped 500, not a dropped socket
                return self._send_json(500, _error(500, str(e), "server_error"))
            text = v.detokenize(ids)
            cut = find_stop(text, stop)
            if cut is not None:
                text, finish = text[:cut], "stop"
            choice = ({"index": 0, "message": {"role": "assistant", "content": text}, "finish_reason": finish}
                      if chat else {"index": 0, "text": text, "logprobs": None, "finish_reason": finish})
            extra = {}
            if entries is not None:
                # where each token's text begins (the streaming decoder's offsets); the entries
                # end with the last token that begins before a stop string's cut
                sd, starts, at = v.stream(), [], 0
                for t in ids:
                    starts.append(at)
                    at += len(sd.push(t))
                keep = len(ids) if cut is None else sum(1 for b in starts if b < cut)
                lj = self._logprob_json(route, ids[:keep], entries[:keep], starts[:keep])
                choice["logprobs"] = lj.pop("logprobs")
                extra = lj
            if cached is not None and route == "/completion":
                extra["tokens_cached"] = cached
            return self._send_json(200, {
                "id": rid, "object": obj, "created": created, "model": eng.model_id, "choices": [choice],
                "usage": usage(len(ids), cached),
                "llmi": {"tokens": ids}, **extra})
        # SSE: headers, one data: line per token batch, final chunk, [DONE], close
        self.send_response(200)
        self.send_header("Content-Type", "text/event-stream")
        self.send_header("Cache-Control", "no-cache")
        self.send_header("Connection", "close")
        self.end_headers()
        self.close_connection = True
        cobj = "chat.completion.chunk" if chat else "text_completion"

        def event(payload: dict) -> None:
            self.wfile.write(b"data: " + json.dumps(payload).encode() + b"\n\n")
            self.wfile.flush()

        if chat:
            event({"id": rid, "object": cobj, "created": created, "model": eng.model_id,
                   "choices": [{"index": 0, "delta": {"role": "assistant"}, "finish_reason": None}]})

        sd = v.stream()
        sf = StopFilter(stop)

        held: list[tuple] = []  # (token, entry, text offset) consumed since the last sent chunk

        def chunk_of(piece: str) -> None:
            ch = ({"index": 0, "delta": {"content": piece}, "finish_reason": None} if chat
                  else {"index": 0, "text": piece, "logprobs": None, "finish_reason": None})
            extra = {}
            if n_top >= 0:
                # the entries travel with the chunk that releases their text; those whose text
                # begins at or after a stop string's cut (sf.sent once stopped) are dropped
                live = [h for h in held if not sf.stopped or h[2] < sf.sent]
                lj = self._logprob_json(route, [h[0] for h in live], [h[1] for h in live], [h[2] for h in live])
                ch["logprobs"] = lj.pop("logprobs")
                extra = lj
                held.clear()
            event({"id": rid, "object": cobj, "created": created, "model": eng.model_id, "choices": [ch], **extra})

        def on_tokens(ts: list[int], entries=None) -> None:
            for i, t in enumerate(ts):
                if n_top >= 0 and not sf.stopped:
                    held.append((t, entries[i], len(sf.text)))
                piece = sf.push(sd.push(t))
                if not piece:
                    continue  # an incomplete UTF-8 sequence, or a possible stop-string prefix: held back
                chunk_of(piece)

        try:
            cached = None
            if cache_on:
                r = eng.run(prompt, max_tokens, ignore_eos, on_tokens, sampling=sampling, stop=stop, n_top=n_top,
                            cache_prompt=cache_prompt)
                ids, finish, cached = r.out, r.finish or "length", r.cached
            elif n_top >= 0:
                ids, finish, _ = eng.generate_logprobs(prompt, max_tokens, ignore_eos, on_tokens, chunk=4,
                                                       sampling=sampling, stop=stop, n_top=n_top)
            else:
                ids, finish = eng.generate(prompt, max_tokens, ignore_eos, on_tokens, chunk=4, sampling=sampling, stop=stop)
            tail = sf.push(sd.flush()) + sf.flush()
            if sf.stopped:
                finish = "stop"
            if tail or any(not sf.stopped or h[2] < sf.sent for h in held):
                chunk_of(tail)
            last = ({"index": 0, "delta": {}, "finish_reason": finish} if chat
                    else {"index": 0, "text": "", "logprobs": None, "finish_reason": finish})
            event({"id": rid, "object": cobj, "created": created, "model": eng.model_id, "choices": [last],
                   "usage": usage(len(ids), cached), **({"tokens_cached": cached} if cached is not None and
                                                        route == "/completion" else {})})
            self.wfile.write(b"data: [DONE]\n\n")
            self.wfile.flush()
        except (BrokenPipeError, ConnectionResetError):
            pass
        except Exception as e:  # decode failed mid-stream: an error event, then close
            try:
                event(_error(500, str(e), "server_error"))
            except (BrokenPipeError, ConnectionResetError):
                pass


def make_server(engine: Engine, host: str, port: int, api_key: Optional[str]) -> ThreadingHTTPServer:
    handler = type("LlmiHandler", (Handler,), {"engine": engine, "api_key": api_key})
    srv = ThreadingHTTPServer((host, port), handler)
    srv.daemon_threads = True
    return srv


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="llama-server", add_help=True)
    ap.add_argument("--version", action="store_true")
    ap.add_argument("-m", "--model")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8080)
    ap.add_argument("-c", "--ctx-size", type=int, default=4096)
    ap.add_argument("-ngl", "--n-gpu-layers", "--gpu-layers", dest="ngl", type=int, default=999)
    ap.add_argument("--api-key-file")
    ap.add_argument("--api-key")
    ap.add_argument("-t", "--threads", type=int, default=0)
    ap.add_argument("--replicas", type=int, default=int(os.environ.get("LLMI_REPLICAS", "1")),
                    help="GPU replicas (devices 0..N-1), one context each")
    ap.add_argument("-np", "--parallel", type=int, default=int(os.environ.get("LLMI_SLOTS", "4")),
                    help="sequences (slots) per replica decoded together (continuous batching)")
    ap.add_argument("--decode-chunk", type=int, default=8, help="tokens per batched decode call")
    ap.add_argument("--max-logprobs", type=int, default=int(os.environ.get("LLMI_MAX_LOGPROBS", "0")),
                    help=f"most top_logprobs / logprobs / n_probs a request may ask for, at most {MAX_LOGPROBS} "
                         "(0, the default: requests for logprobs get a 400)")
    ap.add_argument("--cache-prompt", dest="cache_prompt", action="store_true", default=False,
                    help="prompt cache: prefill only what a prompt adds to what a slot already holds, copy a "
                         "prefix another slot holds (also LLMI_CACHE_PROMPT=1); responses then report cached_tokens")
    ap.add_argument("--no-cache-prompt", dest="cache_prompt", action="store_false",
                    help="prefill every prompt in full (the default; also LLMI_CACHE_PROMPT=0, or "
                         "cache_prompt: false in a request)")
    ap.add_argument("--embeddings", "--embedding", dest="embeddings", action="store_true",
                    default=os.environ.get("LLMI_EMBEDDINGS", "0") == "1",
                    help="serve /v1/embeddings (also LLMI_EMBEDDINGS=1); without it the route answers 501")
    ap.add_argument("--pooling", choices=sorted(POOLING_NAMES), default=None,
                    help="pooling of the embeddings (default: the model's GGUF pooling_type, else none)")
    ap.add_argument("--numerics", choices=NUMERICS_CHOICES, default=None,
                    help="fp32 association of every kernel: ggml's generic order, or the oracle's model of "
                         "upstream's x86 AVX2 association (non-repack); '-fa': decode attention in ggml's CPU "
                         "flash-attention numerics (match with the reference's CPU image unpinned)")
    # llama-server's sampling flags and defaults (per-request fields override them)
    d = SamplingParams()
    ap.add_argument("--temp", type=float, default=d.temperature)
    ap.add_argument("--top-k", type=int, default=d.top_k)
    ap.add_argument("--top-p", type=float, default=d.top_p)
    ap.add_argument("--min-p", type=float, default=d.min_p)
    ap.add_argument("--repeat-penalty", type=float, default=d.repeat_penalty)
    ap.add_argument("--repeat-last-n", type=int, default=d.repeat_last_n)
    ap.add_argument("--presence-penalty", type=float, default=d.presence_penalty)
    ap.add_argument("--frequency-penalty", type=float, default=d.frequency_penalty)
    ap.add_argument("-s", "--seed", type=int, default=d.seed)
    args, extra = ap.parse_known_args(argv)
    if args.numerics is None:
        # argparse does not check a default against `choices`: validate the env value here
        env = os.environ.get("LLMI_NUMERICS", "generic").strip().lower()
        if env not in NUMERICS_CHOICES:
            ap.error(f"LLMI_NUMERICS={os.environ.get('LLMI_NUMERICS')!r}: expected one of {', '.join(NUMERICS_CHOICES)}")
        args.numerics = env
    return args, extra


# --numerics values -> llama_model_params.numerics (llmi.h LLMI_NUMERICS_*)
NUMERICS_CHOICES = ("generic", "x86", "generic-fa", "x86-fa")


def numerics_value(name: str) -> int:
    return (1 if name.startswith("x86") else 0) | (2 if name.endswith("-fa") else 0)


def main(argv=None) -> int:
    args, extra = parse_args(argv)
    if args.version:
        print(VERSION)
        return 0
    if extra:
        print(f"[llmi-server] ignoring unsupported arguments: {' '.join(extra)}", file=sys.stderr)
    if not args.model:
        print("error: -m/--model is required", file=sys.stderr)
        return 2
    key = args.api_key
    if args.api_key_file:
        key = open(args.api_key_file).read().strip()
    sp = SamplingParams(temperature=args.temp, top_k=args.top_k, top_p=args.top_p, min_p=args.min_p,
                        repeat_penalty=args.repeat_penalty, repeat_last_n=args.repeat_last_n,
                        presence_penalty=args.presence_penalty, frequency_penalty=args.frequency_penalty, seed=args.seed)
    eng = Engine(args.model, args.ctx_size, args.ngl, list(range(max(1, args.replicas))), slots=args.parallel,
                 chunk=args.decode_chunk, sampling=sp, numerics=numerics_value(args.numerics),
                 max_logprobs=args.max_logprobs, cache_prompt=args.cache_prompt, embeddings=args.embeddings,
                 pooling=POOLING_NAMES[args.pooling] if args.pooling else None)
    srv = make_server(eng, args.host, args.port, key)
    threading.Thread(target=eng.load, daemon=True).start()
    print(f"[llmi-server] listening on {args.host}:{args.port}", file=sys.stderr, flush=True)
    try:
        srv.serve_forever()
    except KeyboardInterrupt:
        pass
    return 0


if __name__ == "__main__":
    sys.exit(main())
