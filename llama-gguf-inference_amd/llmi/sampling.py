"""Token sampling for the HTTP front end: llama-server's default sampler chain.

The reference's backend is llama-server (scripts/start.sh:235); its request fields
temperature / top_p / frequency_penalty / presence_penalty / stop are documented in
docs/API_REFERENCE.md:363-379 and forwarded verbatim by scripts/gateway.py:699-804.
Upstream llama-server (not vendored) samples each token with the chain

    penalties -> top_k -> top_p -> min_p -> temperature -> dist

restated here on the host over the logits of llama_get_logits_ith:

  penalties  for every token t among the last `repeat_last_n` generated/prompt tokens,
             with c = its count there: logit <= 0 ? logit * repeat_penalty
             : logit / repeat_penalty, then logit -= c * frequency_penalty +
             presence_penalty
  top_k      keep the k largest logits (k <= 0: all); of equal logits across the k-th
             place, the lower token ids
  top_p      softmax over the kept ones, keep the smallest prefix (by logit, descending)
             whose probability mass reaches p (at least one)
  min_p      keep the tokens with p >= min_p * p_max
  temp       logits / temperature; temperature <= 0 keeps only the largest (greedy,
             first max wins as llama_sampler_greedy)
  dist       softmax, one draw from a seeded generator (per request; seed < 0 or
             absent: a fresh random seed)

Defaults are llama-server's (temperature 0.8, top_k 40, top_p 0.95, min_p 0.05,
repeat_penalty 1.0 over the last 64 tokens, no frequency/presence penalty); the server's
--temp/--top-k/... flags change them as llama-server's do.  Requests whose chain reduces
to an argmax of the raw logits (temperature <= 0 or top_k == 1, no penalties) decode on
the device (llmi_generate_greedy_batch) with no logits copy.  The chain's one random
decision is a single uniform (sample_with_uniform: numpy's Generator.choice draws one
random() double and searches it in the normalised cdf), so a sampled request within the
device limits (device_eligible) decodes on the device as well: the host draws the chunk's
uniforms from the request's generator and llmi_generate_sampled_batch runs this chain on
the device logits (csrc/sample.hip), the same seed giving the same tokens as the host
path; other requests are sampled here over copied logits.  token_logprobs is the host
definition of what a request for logprobs gets (the raw distribution, before this chain), which
llmi_generate_logprobs_batch restates on the device (csrc/logprob.hip).  The random stream is
numpy's PCG64, not llama.cpp's mt19937: sampled text with a given seed is reproducible
here but not token-identical to llama-server's (parity of sampled output is unpinned;
greedy output is the parity bar, tests/test_gpu_*.py).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional, Sequence

import numpy as np


@dataclass(frozen=True)
class SamplingParams:
    temperature: float = 0.8
    top_k: int = 40
    top_p: float = 0.95
    min_p: float = 0.05
    repeat_penalty: float = 1.0
    repeat_last_n: int = 64
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    seed: int = -1

    @property
    def penalized(self) -> bool:
        return self.repeat_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    @property
    def greedy(self) -> bool:
        """The whole chain is an argmax of the raw logits (the device fast path)."""
        return (self.temperature <= 0.0 or self.top_k == 1) and not self.penalized

    def with_request(self, req: dict) -> "SamplingParams":
        """These defaults overridden by a request's fields (llama-server / OpenAI names);
        ValueError for a value llama-server would reject."""
        kw = {}

        def num(name, cast, lo=None, hi=None, alias=None):
            v = req.get(name, req.get(alias) if alias else None)
            if v is None:
                return
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"'{name}' must be a number")
            v = cast(v)
            if (lo is not None and v < lo) or (hi is not None and v > hi):
                raise ValueError(f"'{name}' out of range [{lo}, {hi}]")
            kw[name] = v

        num("temperature", float, 0.0, 100.0)
        num("top_k", int, None, None)
        num("top_p", float, 0.0, 1.0)
        num("min_p", float, 0.0, 1.0)
        num("repeat_penalty", float, 0.0, None)
        num("repeat_last_n", int, -1, None)
        num("presence_penalty", float, -2.0, 2.0)
        num("frequency_penalty", float, -2.0, 2.0)
        num("seed", int, None, None)
        return replace(self, **kw)


def _softmax(x: np.ndarray) -> np.ndarray:
    e = np.exp(x - x.max())
    return e / e.sum()


@dataclass(frozen=True)
class SampleTrace:
    """What sample_with_uniform decided, for tests: the final candidate ids in order and the
    smallest distance of any decision from its threshold (inf where the stage did not run):
    |cumsum - top_p|, |pr - min_p * pr[0]| over the candidates not tied with the first,
    |cdf - u| short of the last entry (which is 1 exactly)."""
    token: int
    candidates: tuple
    margin_top_p: float = float("inf")
    margin_min_p: float = float("inf")
    margin_dist: float = float("inf")

    @property
    def margin(self) -> float:
        return min(self.margin_top_p, self.margin_min_p, self.margin_dist)


def penalized_logits(p: SamplingParams, logits: np.ndarray, history: Sequence[int]) -> np.ndarray:
    """A float32 copy of the row with the repeat / frequency / presence penalties applied
    over the last repeat_last_n tokens of history."""
    lg = np.array(logits, dtype=np.float32, copy=True)
    if p.penalized:
        n = len(history) if p.repeat_last_n < 0 else min(p.repeat_last_n, len(history))
        if n > 0:
            toks, counts = np.unique(np.asarray(history[len(history) - n:], dtype=np.int64), return_counts=True)
            toks, counts = toks[(toks >= 0) & (toks < lg.size)], counts[(toks >= 0) & (toks < lg.size)]
            v = lg[toks]
            v = np.where(v <= 0, v * p.repeat_penalty, v / p.repeat_penalty)
            v = v - counts * p.frequency_penalty - (counts > 0) * p.presence_penalty
            lg[toks] = v.astype(np.float32)
    return lg


def token_logprobs(logits: np.ndarray, n_top: int):
    """(lse, ids, logprobs) of one raw float32 logits row: no penalties and no temperature,
    what llama-server reports with post_sampling_probs off.  This is the definition the
    device restates (csrc/logprob.hip).

      x = logits.astype(float64), m = x.max(), lse = m + log(sum(exp(x - m)))
      logprobs[t] = x[t] - lse for EVERY token t (a float64 array of the row's length) --
      never log(p): a token more than 745 below the maximum keeps a finite value
      ids = the top min(n_top, V) token ids in argmax_key order, logit descending and the
      lower id first on ties (np.lexsort((ids, -logits)), sample_trace's ordering)

    -inf entries are legal and yield -inf.  A row with a NaN, or whose maximum is not finite,
    is outside the definition: nothing is promised for it, here or on the device."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    m = x.max()
    lse = float(m + np.log(np.sum(np.exp(x - m))))
    k = max(0, min(int(n_top), x.size))
    if k == 0:
        ids = np.zeros(0, dtype=np.int64)
    elif k < x.size:
        # the k largest; of a run of equal logits that straddles the k-th place, the lower ids
        kth = x[np.argpartition(-x, k - 1)[k - 1]]
        above = np.flatnonzero(x > kth)
        ids = np.concatenate([above, np.flatnonzero(x == kth)[:k - above.size]])
    else:
        ids = np.arange(x.size)
    ids = ids[np.lexsort((ids, -x[ids]))]
    return lse, ids, x - lse


def sample_trace(p: SamplingParams, logits: np.ndarray, history: Sequence[int], u: Optional[float]) -> SampleTrace:
    """The chain on one logits row, its one random decision made by the uniform u in [0, 1)
    (None when temperature <= 0: nothing is drawn).  This is the definition the device
    sampler (csrc/sample.hip) restates."""
    lg = penalized_logits(p, logits, history)
    if p.temperature <= 0.0:
        t = int(np.argmax(lg))
        return SampleTrace(t, (t,))
    # candidates sorted by logit, descending (stable: lower ids first on ties)
    k = lg.size if p.top_k <= 0 else min(p.top_k, lg.size)
    if k < lg.size:
        # the k largest; of a run of equal logits that straddles the k-th place, the lower
        # ids (argpartition alone leaves that choice to its pivots)
        kth = lg[np.argpartition(-lg, k - 1)[k - 1]]
        above = np.flatnonzero(lg > kth)
        idx = np.concatenate([above, np.flatnonzero(lg == kth)[:k - above.size]])
    else:
        idx = np.arange(lg.size)
    idx = idx[np.lexsort((idx, -lg[idx]))]
    cand = lg[idx].astype(np.float64)
    m_top_p = m_min_p = float("inf")
    if p.top_p < 1.0:
        cs = np.cumsum(_softmax(cand))
        m_top_p = float(np.min(np.abs(cs - p.top_p)))
        keep = int(np.searchsorted(cs, p.top_p) + 1)
        idx, cand = idx[:max(1, keep)], cand[:max(1, keep)]
    if p.min_p > 0.0 and cand.size > 1:
        pr = _softmax(cand)
        # (a candidate tied with the first has its probability bit for bit, and min_p <= 1:
        # that comparison involves no rounding and has no margin)
        m_min_p = float(np.min(np.abs(pr[cand != cand[0]] - p.min_p * pr[0]), initial=np.inf))
        m = pr >= p.min_p * pr[0]
        m[0] = True
        idx, cand = idx[m], cand[m]
    pr = _softmax(cand / p.temperature)
    # Generator.choice(n, p=pr): one random() double searched in the normalised cdf
    cdf = np.cumsum(pr)
    cdf /= cdf[-1]
    i = min(int(np.searchsorted(cdf, u, side="right")), cdf.size - 1)
    # (cdf[-1] is x / x = 1 exactly and u < 1: the last entry decides nothing)
    return SampleTrace(int(idx[i]), tuple(int(t) for t in idx), m_top_p, m_min_p,
                       float(np.min(np.abs(cdf[:-1] - u), initial=np.inf)))


def sample_with_uniform(p: SamplingParams, logits: np.ndarray, history: Sequence[int], u: Optional[float]) -> int:
    return sample_trace(p, logits, history, u).token


# what the device sampler takes (kSampleMaxTopK / kSampleMaxLastN, csrc/kernels.h); the rest
# (top_k <= 0, a larger top_k, a whole-context or longer penalty window) stays on the host
DEVICE_MAX_TOP_K = 256
DEVICE_MAX_LAST_N = 256


def device_eligible(p: SamplingParams) -> bool:
    return 1 <= p.top_k <= DEVICE_MAX_TOP_K and 0 <= p.repeat_last_n <= DEVICE_MAX_LAST_N and all(
        np.isfinite(v) for v in (p.temperature, p.top_p, p.min_p, p.repeat_penalty, p.presence_penalty,
                                 p.frequency_penalty))


class Sampler:
    """One request's sampler (its own generator).  The generator's only use is one uniform
    per sampled token: rng.random(k) hands the device the draws the next k sample() calls
    would have made."""

    def __init__(self, params: SamplingParams):
        self.p = params
        self.rng = np.random.default_rng(params.seed if params.seed >= 0 else None)

    def sample(self, logits: np.ndarray, history: Sequence[int]) -> int:
        u = self.rng.random() if self.p.temperature > 0.0 else None
        return sample_with_uniform(self.p, logits, history, u)


def find_stop(text: str, stops: Sequence[str]) -> Optional[int]:
    """Index of the earliest occurrence of any stop string in text, or None."""
    best = None
    for s in stops:
        if s:
            i = text.find(s)
            if i >= 0 and (best is None or i < best):
                best = i
    return best


class StopFilter:
    """Streams text while holding back any tail that could still begin a stop string;
    `done` truncates at the stop string (llama-server's partial-stop handling)."""

    def __init__(self, stops: Sequence[str]):
        self.stops = [s for s in stops if s]
        self.hold = max((len(s) for s in self.stops), default=1) - 1
        self.text = ""
        self.sent = 0
        self.stopped = False

    def push(self, piece: str) -> str:
        if self.stopped:
            return ""
        self.text += piece
        i = find_stop(self.text, self.stops)
        if i is not None:
            self.stopped = True
            out = self.text[self.sent:i]
            self.sent = i
            return out
        safe = max(self.sent, len(self.text) - self.hold)
        out = self.text[self.sent:safe]
        self.sent = safe
        return out

    def flush(self) -> str:
        if self.stopped:
            return ""
        out = self.text[self.sent:]
        self.sent = len(self.text)
        return out


def parse_stop(v) -> list[str]:
    if v is None:
        return []
    if isinstance(v, str):
        return [v]
    if isinstance(v, list) and all(isinstance(s, str) for s in v):
        return list(v)
    raise ValueError("'stop' must be a string or a list of strings")
