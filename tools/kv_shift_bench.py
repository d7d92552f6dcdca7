"""k_kv_shift next to k_kv_seq_cp of the same positions (context shift): Llama-3-8B's
cache shape (256 planes, head_dim 128, n_ctx 16384), event-timed through the llmi_kv_shift and
llmi_kv_seq_copy hooks, the two alternating, 15 runs after 3 warm ones.  Prints one JSON line per
case; --out FILE also writes them all."""
import json, os, statistics, sys
sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama-gguf-inference_amd")]
import numpy as np
import torch
import llmi

PL, D, N_CTX = 256, 128, 16384
dev = "cuda"
torch.zeros(1, device=dev)
def cache():
    return torch.randint(-20000, 20000, (PL * N_CTX * D,), dtype=torch.int16, device=dev)
k, v, k2, v2 = cache(), cache(), cache(), cache()
h = torch.randint(0, 1000, (N_CTX,), dtype=torch.int32, device=dev)
h2 = torch.zeros_like(h)
half = D // 2
theta = 500000.0 ** (-2.0 * np.arange(half) / D)
ang = np.arange(N_CTX)[:, None] * theta[None, :]
tab = torch.from_numpy(np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)).to(dev)
out = {}
def med(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}
for name, (n_keep, d, n_past) in {"half": (0, 8192, 16384), "half_keep256": (256, 8064, 16384), "odd": (0, 8191, 16384),
                                  "d1": (0, 1, 16384), "slot2048": (0, 1024, 2048), "slot2048_odd": (4, 1021, 2047)}.items():
    tail = n_past - n_keep - d
    nbytes = 2 * (2 * PL * D * 2 + 4) * tail
    sh, cp = [], []
    for i in range(18):
        a = llmi.kv_shift(PL, D, D, N_CTX, n_keep, d, n_past, tab.data_ptr(), k.data_ptr(), v.data_ptr(), h.data_ptr())
        b = llmi.kv_seq_copy(PL, D, N_CTX, n_keep + d, n_past, k.data_ptr(), v.data_ptr(), h.data_ptr(), k2.data_ptr(),
                             v2.data_ptr(), h2.data_ptr())
        if i >= 3:
            sh.append(a); cp.append(b)
    out[name] = {"n_keep": n_keep, "d": d, "n_past": n_past, "tail": tail, "bytes": nbytes, "shift": med(sh), "copy": med(cp),
                 "shift_GBps": nbytes / statistics.median(sh) / 1e3, "copy_GBps": nbytes / statistics.median(cp) / 1e3}
    print(name, json.dumps(out[name]), flush=True)
if "--out" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--out") + 1], "w"), indent=1)
