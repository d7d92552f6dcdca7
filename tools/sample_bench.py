#!/usr/bin/env python3
"""Cost of sampling on the device (csrc/sample.hip), next to the two paths it sits between.

  kernel   k_sample alone (llmi_sample_logits, event-timed) on rows of 128256 logits: top_k 40
           and 256, 1 and 8 rows; the server's default chain, and the same with a penalty
           window of 64 tokens
  decode   tokens/s of llmi_generate_sampled_batch, of llmi_generate_greedy_batch (the ceiling)
           and of the host path (llama_decode with every slot's logits copied + Sampler.sample,
           one token per call) on a synthetic preset (default llama3-8b-q4km, bench.py's model
           file), 1 and 8 sequences over bench.py's timed window; the per-step gap to greedy
           beside the K_OUTPUT launch time (llmi_profile_kernels)

Each leg runs in a child process of its own under a time limit; a leg that fails or runs
out of time ends the run.  One JSON line per leg on stdout.

    python tools/sample_bench.py [--preset llama3-8b-q4km] [--steps 256] [--legs kernel,decode1,decode8]
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
        for name, p in (("top_k40", SamplingParams(top_k=40)), ("top_k256", SamplingParams(top_k=256)),
                        ("top_k40_penalties", SamplingParams(top_k=40, repeat_penalty=1.1, frequency_penalty=0.1)),
                        ("argmax_penalties", SamplingParams(temperature=0.0, repeat_penalty=1.1))):
            us = []
            for _ in range(12):  # the first two launches warm the code object and the allocator
                us.append(llmi.sample_logits(lg, hist, [p] * rows, rng.random(rows), want_penalized=False)[3])
            t = sorted(us[2:])
            out[f"{name}_rows{rows}"] = {"us_median": round(t[len(t) // 2], 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2)}
    return {"leg": "kernel", "V": V, "us": out,
            "note": "event-timed launch of k_sample on a freshly uploaded row (cold in L2), 10 launches after 2 warm ones"}


def leg_decode(args, k: int) -> dict:
    import numpy as np
    import torch  # noqa: F401  (before libllmi: one HIP runtime per process)

    import llmi
    from bench import window_start
    from llmi.sampling import Sampler, SamplingParams

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

    def greedy(first, pos, n):
        return [t[-1] for t in ctx.generate_greedy_batch(seqs, first, pos, n)]

    def device(first, pos, n):
        unis = [np.random.default_rng(7 + s).random(n) for s in seqs]
        return [t[-1] for t in ctx.generate_sampled_batch(seqs, first, pos, n, params, unis)]

    def host(first, pos, n):  # the scheduler's host path: one llama_decode per token, logits copied, numpy sampler
        samplers = [Sampler(p) for p in params]
        hist = [list(pr) + [f] for pr, f in zip(prompts, first)]  # (the window's history: the penalties are off)
        last, pos = list(first), list(pos)
        for _ in range(n):
            assert ctx.decode(last, pos=pos, seq=seqs, logits_all=True) == 0
            last = [samplers[i].sample(ctx.logits(i), hist[i]) for i in range(k)]
            for i in range(k):
                hist[i].append(last[i])
                pos[i] += 1
        return last

    res = {}
    for name, fn in (("greedy", greedy), ("device_sampled", device), ("greedy_again", greedy), ("device_sampled_again", device),
                     ("host_sampled", host)):
        dt = timed(fn)
        res[name] = {"tok_s": round(k * args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 4)}
    gap_us = (min(res["device_sampled"]["ms_per_step"], res["device_sampled_again"]["ms_per_step"]) -
              min(res["greedy"]["ms_per_step"], res["greedy_again"]["ms_per_step"])) * 1e3
    out = {"leg": f"decode{k}", "preset": args.preset, "sequences": k, "window": [start, start + args.steps], **res,
           "gap_to_greedy_us_per_step": round(gap_us, 2)}
    if k == 1:  # the single-sequence step's logits launch, in its place in the step
        ctx1 = llmi.Context(m, n_ctx=n_ctx)
        assert ctx1.decode(prompts[0]) == 0
        f = ctx1.greedy(-1)
        ctx1.generate_greedy(f, args.prompt, pre)
        out["k_output_us"] = round(ctx1.profile_kernels(f, start, 20)["output"]["us"], 2)
    return out


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
            print(f"sample_bench: leg {leg} ran out of time; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"sample_bench: leg {leg} ended with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
