#!/usr/bin/env python3
"""Cost of log-probabilities on the device (csrc/logprob.hip), next to what they sit beside.

  kernel   k_logprob, k_sample and k_logprob_pick (llmi_logprob_rows, each event-timed in the
           same run) on rows of 128256 logits: 1 and 8 rows, n_top 0 and 20, the server's
           default chain
  decode   tokens/s of llmi_generate_logprobs_batch (n_top 20 for every sequence), of
           llmi_generate_sampled_batch (the same call without them) and of the host alternative
           the call replaces (llama_decode with every slot's logits copied + Sampler.sample +
           token_logprobs, one token per call) on a synthetic preset (default llama3-8b-q4km,
           bench.py's model file), 1 and 8 sequences over bench.py's timed window

Each leg runs in a child process of its own under a time limit; a leg that fails or runs
out of time ends the run.  One JSON line per leg on stdout.

    python tools/logprob_bench.py [--preset llama3-8b-q4km] [--steps 256] [--legs kernel,decode1,decode8]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "llama-gguf-inference_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LIMITS = {"kernel": 240, "decode1": 600, "decode8": 600}  # seconds per leg


def leg_kernel(args) -> dict:
    import numpy as np

    import llmi
    from llmi.sampling import SamplingParams

    V = 128256
    rng = np.random.default_rng(1)
    out = {}
    for rows in (1, 8):
        lg = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
        hist = rng.integers(0, V, (rows, 64)).astype(np.int32)
        for n_top in (0, 20):
            us = []
            for _ in range(12):  # the first two launches warm the code objects and the allocator
                us.append(llmi.logprob_rows(lg, hist, [SamplingParams(top_k=40)] * rows, rng.random(rows), [n_top] * rows,
                                            want_rows=False)["usec"])
            med = lambda i: round(sorted(u[i] for u in us[2:])[5], 2)  # noqa: E731
            out[f"n_top{n_top}_rows{rows}"] = {"k_logprob_us": med(0), "k_sample_us": med(1), "k_logprob_pick_us": med(2)}
        # k_sample alone on the same rows, freshly uploaded as k_logprob finds them
        alone = sorted(llmi.sample_logits(lg, hist, [SamplingParams(top_k=40)] * rows, rng.random(rows), want_penalized=False)[3]
                       for _ in range(12))
        out[f"k_sample_alone_rows{rows}"] = {"us_median": round(alone[5], 2)}
    return {"leg": "kernel", "V": V, "us_median": out,
            "note": "event-timed launches in step order on a freshly uploaded row (k_logprob reads it cold in L2, "
                    "k_sample after it warm), 10 runs after 2 warm ones"}


def leg_decode(args, k: int) -> dict:
    import numpy as np
    import torch  # noqa: F401  (before libllmi: one HIP runtime per process)

    import llmi
    from bench import window_start
    from llmi.sampling import Sampler, SamplingParams, token_logprobs

    path = os.path.join(args.model_dir, f"{args.preset}-s{args.seed}.gguf")
    if not os.path.exists(path):
        os.makedirs(args.model_dir, exist_ok=True)
        llmi.write_synthetic_gguf(path + ".tmp", args.preset, seed=args.seed)
        os.replace(path + ".tmp", path)
    m = llmi.Model(path)
    start = window_start(args.prompt, args.steps, args.warmup)
    n_ctx = (start + args.steps + 30 + 255) // 256 * 256
    ctx = llmi.Context(m, n_ctx=n_ctx, n_seq=max(2, k))
    rng = np.random.default_rng(40)
    bos = m.bos if m.bos >= 0 else 1
    prompts = [[bos] + [int(t) for t in rng.integers(0, min(128000, m.n_vocab), args.prompt - 1)] for _ in range(k)]
    seqs = list(range(k))
    firsts = []
    for s, p in enumerate(prompts):
        assert ctx.decode(p, seq=[s] * len(p)) == 0
        firsts.append(ctx.greedy(-1))
    params = [SamplingParams(seed=100 + s) for s in seqs]  # the server's defaults
    pre = start - args.prompt

    def rewind():
        for s in seqs:
            ctx.seq_rm(s, args.prompt, -1)

    def timed(fn):
        """fn(first tokens, positions, n) -> last tokens; `pre` untimed steps to the window, then the timed ones"""
        rewind()
        nxt = fn(firsts, [args.prompt] * k, pre)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(nxt, [start] * k, args.steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def unis(n):
        return [np.random.default_rng(7 + s).random(n) for s in seqs]

    def sampled(first, pos, n):
        return [t[-1] for t in ctx.generate_sampled_batch(seqs, first, pos, n, params, unis(n))]

    def logprobs(n_top):
        def fn(first, pos, n):
            return [t[-1] for t in ctx.generate_logprobs_batch(seqs, first, pos, n, params, unis(n), [n_top] * k)[0]]
        return fn

    def host(first, pos, n):  # what the call replaces: one llama_decode per token, logits copied, numpy on the host
        samplers = [Sampler(p) for p in params]
        hist = [list(pr) + [f] for pr, f in zip(prompts, first)]
        last, pos = list(first), list(pos)
        for _ in range(n):
            assert ctx.decode(last, pos=pos, seq=seqs, logits_all=True) == 0
            for i in range(k):
                lg = ctx.logits(i)
                last[i] = samplers[i].sample(lg, hist[i])
                token_logprobs(lg, 20)
                hist[i].append(last[i])
                pos[i] += 1
        return last

    res = {}
    for name, fn in (("device_sampled", sampled), ("device_logprobs_top20", logprobs(20)), ("device_sampled_again", sampled),
                     ("device_logprobs_top20_again", logprobs(20)), ("device_logprobs_top0", logprobs(0)),
                     ("host_sampled_logprobs_top20", host)):
        dt = timed(fn)
        res[name] = {"tok_s": round(k * args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 4)}
    gap_us = (min(res["device_logprobs_top20"]["ms_per_step"], res["device_logprobs_top20_again"]["ms_per_step"]) -
              min(res["device_sampled"]["ms_per_step"], res["device_sampled_again"]["ms_per_step"])) * 1e3
    return {"leg": f"decode{k}", "preset": args.preset, "sequences": k, "window": [start, start + args.steps], **res,
            "gap_to_sampled_us_per_step": round(gap_us, 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama3-8b-q4km")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--model-dir", default=os.environ.get("LLMI_BENCH_DIR", "/tmp/llmi_bench"))
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--legs", default="kernel,decode1,decode8")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        r = leg_kernel(args) if args.leg == "kernel" else leg_decode(args, int(args.leg[len("decode"):]))
        print(json.dumps(r), flush=True)
        return 0
    for leg in [x for x in args.legs.split(",") if x]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--preset", args.preset, "--seed", str(args.seed),
               "--model-dir", args.model_dir, "--prompt", str(args.prompt), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=LIMITS.get(leg, 600)).returncode
        except subprocess.TimeoutExpired:
            print(f"logprob_bench: leg {leg} ran out of time; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"logprob_bench: leg {leg} ended with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
