#!/usr/bin/env python3
"""What the prompt cache costs and saves (csrc/kvcopy.hip, llmi/server.py).

  kernel   k_kv_seq_cp (llmi_kv_seq_copy, event-timed) on Llama-3-8B's cache shape (256 planes,
           head_dim 128) in a context of 16384 positions, copying 128, 2048 and 16384 positions,
           next to the same copy done with the runtime's calls it replaces: two
           hipMemcpy2DAsync (K, V) and one hipMemcpyAsync (hist) between the same two events.
           Successive runs of a size move through the context, so that a run does not find its
           source in a cache the run before it filled (the caches are far larger than L2 only
           at 16384 positions, where every run copies all of them).
  ttft     time to the first token of a request of 2048 + 32 prompt tokens on a synthetic
           preset (default llama3-8b-q4km, bench.py's model file) through the server's Engine:
           cold (LLMI_CACHE_PROMPT=0: the whole prompt is prefilled), with the first 2048 held
           by the slot the request goes to (`same_slot`), with them held by a slot that is busy
           decoding, so that the free slot gets them by the device copy (`other_slot`), and of
           a cold 32-token prompt.  `admit_ms` is the scheduler's admission (copy, prefill of the
           rest, first token); `ttft_ms` the wall time from submit to the first token, which in
           `other_slot` also waits for the busy slot's running decode call.

Each leg runs in a child process of its own under a time limit; a leg that fails or runs
out of time ends the run.  One JSON line per leg on stdout.

    python tools/prompt_cache_bench.py [--preset llama3-8b-q4km] [--legs kernel,ttft]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "llama-gguf-inference_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LIMITS = {"kernel": 300, "ttft": 600}  # seconds per leg
N_PLANES, HEAD_DIM, N_CTX = 256, 128, 16384  # Llama-3-8B: 32 layers x 8 KV heads
WARM, REPS = 3, 15


def _hip_runtime() -> C.CDLL:
    """The HIP runtime this process has loaded already (torch's)."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    if not paths:
        raise RuntimeError("no HIP runtime is loaded")
    return C.CDLL(paths[0])


def _median(v):
    s = sorted(v)
    return s[len(s) // 2]


def leg_kernel(args) -> dict:
    import torch

    import llmi

    torch.zeros(1, device="cuda")
    hip = _hip_runtime()
    vp, sz = C.c_void_p, C.c_size_t
    hip.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, C.c_int, vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]
    hip.hipEventCreate.argtypes = [C.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    D2D = 3  # hipMemcpyDeviceToDevice
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

    kv = N_PLANES * N_CTX * HEAD_DIM
    gen = torch.Generator(device="cuda").manual_seed(1)
    mk = lambda n, dt: torch.randint(-30000, 30000, (n,), dtype=dt, device="cuda", generator=gen)  # noqa: E731
    ks, vs, kd, vd = (mk(kv, torch.int16) for _ in range(4))
    hs, hd = mk(N_CTX, torch.int32), mk(N_CTX, torch.int32)
    torch.cuda.synchronize()

    def memcpy_us(p0, p1):
        n = p1 - p0
        assert hip.hipEventRecord(e0, None) == 0
        rc = hip.hipMemcpy2DAsync(kd.data_ptr() + p0 * HEAD_DIM * 2, N_CTX * HEAD_DIM * 2, ks.data_ptr() + p0 * HEAD_DIM * 2,
                                  N_CTX * HEAD_DIM * 2, n * HEAD_DIM * 2, N_PLANES, D2D, None)
        rc |= hip.hipMemcpy2DAsync(vd.data_ptr() + p0 * 2, N_CTX * 2, vs.data_ptr() + p0 * 2, N_CTX * 2, n * 2,
                                   N_PLANES * HEAD_DIM, D2D, None)
        rc |= hip.hipMemcpyAsync(hd.data_ptr() + p0 * 4, hs.data_ptr() + p0 * 4, n * 4, D2D, None)
        assert rc == 0 and hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        return ms.value * 1e3

    def kernel_us(p0, p1):
        return llmi.kv_seq_copy(N_PLANES, HEAD_DIM, N_CTX, p0, p1, ks.data_ptr(), vs.data_ptr(), hs.data_ptr(),
                                kd.data_ptr(), vd.data_ptr(), hd.data_ptr())

    out = {}
    for n in (128, 2048, 16384):
        nbytes = 2 * (2 * N_PLANES * HEAD_DIM * 2 + 4) * n
        res = {"bytes": nbytes}
        # the two interleaved, run by run, each at the next window of the context
        us = {"kernel": [], "memcpy": []}
        for r in range(WARM + REPS):
            for j, (name, fn) in enumerate((("kernel", kernel_us), ("memcpy", memcpy_us))):
                p0 = (2 * r + j) % (N_CTX // n) * n
                t = fn(p0, p0 + n)
                if r >= WARM:
                    us[name].append(t)
        for name, v in us.items():
            m = _median(v)
            res[name] = {"us_median": round(m, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                         "GBps": round(nbytes / (m * 1e-6) / 1e9, 1)}
        res["kernel_over_memcpy"] = round(res["kernel"]["us_median"] / res["memcpy"]["us_median"], 3)
        out[f"n{n}"] = res
    # (the runs at 16384 positions copied everything)
    ok = bool(torch.equal(kd, ks) and torch.equal(vd, vs) and torch.equal(hd, hs))
    return {"leg": "kernel", "n_planes": N_PLANES, "head_dim": HEAD_DIM, "n_ctx": N_CTX, "copies_equal": ok, **out,
            "note": f"event-timed on the null stream, {REPS} runs after {WARM} warm ones, kernel and memcpy alternating; "
                    "bytes = 2 * (2 * n_planes * head_dim * 2 + 4) * n (read + written)"}


def leg_ttft(args) -> dict:
    import numpy as np
    import torch  # noqa: F401  (before libllmi: one HIP runtime per process)

    import llmi
    from llmi.server import Engine

    path = os.path.join(args.model_dir, f"{args.preset}-s{args.seed}.gguf")
    if not os.path.exists(path):
        os.makedirs(args.model_dir, exist_ok=True)
        llmi.write_synthetic_gguf(path + ".tmp", args.preset, seed=args.seed)
        os.replace(path + ".tmp", path)
    rng = np.random.default_rng(5)
    toks = lambda n: [int(t) for t in rng.integers(3, 100000, n)]  # noqa: E731
    shared, n_new = [1] + toks(args.cached - 1), args.new
    quiet = lambda t, e: None  # noqa: E731

    def engine(cache: bool):
        os.environ["LLMI_CACHE_PROMPT"] = "1" if cache else "0"
        eng = Engine(path, 4096, 99, [0], slots=2, chunk=8)
        eng.load()
        assert eng.ready, eng.error
        assert eng.prompt_cache == cache
        rep = eng.replicas[0]
        inner, spans = rep._admit, []

        def timed(r):
            t0 = time.perf_counter()
            inner(r)
            spans.append(time.perf_counter() - t0)

        rep._admit = timed
        return eng, spans

    def one(eng, spans, prompt, **kw):
        r = eng.run(prompt, 1, True, quiet, **kw)
        return r, {"ttft_ms": (r.t_first - r.t_submit) * 1e3, "admit_ms": spans[-1] * 1e3}

    def close(eng):
        for rep in eng.replicas:
            rep.stop = True

    def summary(rows):
        return {k: {"median": round(_median([x[k] for x in rows]), 3), "min": round(min(x[k] for x in rows), 3),
                    "max": round(max(x[k] for x in rows), 3)} for k in ("ttft_ms", "admit_ms")}

    res = {}
    # the parent's path: every prompt prefilled in full
    eng, spans = engine(False)
    for name, head in (("cold", shared), ("cold_short", [])):
        rows = [one(eng, spans, head + toks(n_new))[1] for _ in range(WARM + args.reps)]
        res[name] = {"prompt_tokens": len(head) + n_new, **summary(rows[WARM:])}
    close(eng)
    # the cache: the slot that holds the prefix takes the request
    eng, spans = engine(True)
    rows = []
    for _ in range(WARM + args.reps + 1):
        r, row = one(eng, spans, shared + toks(n_new))
        rows.append((r.cached, row))
    assert all(c == len(shared) for c, _ in rows[1:]), [c for c, _ in rows]
    res["same_slot"] = {"cached_tokens": len(shared), **summary([row for _, row in rows[1 + WARM:]])}
    close(eng)
    # the slot that holds the prefix is busy decoding: the other one gets it by the device copy
    eng, spans = engine(True)
    ctx = eng.replicas[0].ctx
    inner, copies = ctx.seq_cp, []

    def counted(src, dst, p0=0, p1=-1):
        copies.append((p0, p1))
        return inner(src, dst, p0, p1)

    ctx.seq_cp = counted
    busy = eng.submit(shared + toks(n_new), 1800, True, None, None)
    busy.q.get(timeout=300)
    rows = []
    for _ in range(WARM + args.reps):
        one(eng, spans, toks(8))  # an unrelated prompt (no shared first token) takes the free slot's rows
        n_cp = len(copies)
        r, row = one(eng, spans, shared + toks(n_new))
        assert busy.finish is None and r.cached == len(shared) and copies[n_cp:] == [(0, len(shared))], (r.cached, copies[n_cp:])
        rows.append(row)
    res["other_slot"] = {"cached_tokens": len(shared), "copied_positions": len(shared), **summary(rows[WARM:])}
    while busy.q.get(timeout=300) is not None:
        pass
    close(eng)
    return {"leg": "ttft", "preset": args.preset, "cached": len(shared), "new": n_new, "reps": args.reps, **res,
            "note": "max_tokens 1, greedy; other_slot's ttft_ms includes the wait for the busy slot's decode call"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llama3-8b-q4km")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--model-dir", default=os.environ.get("LLMI_BENCH_DIR", "/tmp/llmi_bench"))
    ap.add_argument("--cached", type=int, default=2048)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="kernel,ttft")
    ap.add_argument("--leg", default=None, help="(internal) run this one leg in this process")
    args = ap.parse_args()
    if args.leg:
        r = leg_kernel(args) if args.leg == "kernel" else leg_ttft(args)
        print(json.dumps(r), flush=True)
        return 0
    for leg in [x for x in args.legs.split(",") if x]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--preset", args.preset, "--seed", str(args.seed),
               "--model-dir", args.model_dir, "--cached", str(args.cached), "--new", str(args.new), "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=LIMITS.get(leg, 600)).returncode
        except subprocess.TimeoutExpired:
            print(f"prompt_cache_bench: leg {leg} ran out of time; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"prompt_cache_bench: leg {leg} ended with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
