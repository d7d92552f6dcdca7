"""Child process of tests/test_gpu_context_lifetime.py: create / exercise / close cycles of a
context, and the device's free memory around them.

    python context_lifetime_child.py ROOT GGUF_SINGLE GGUF_BATCHED

ROOT is the repository tree whose library runs.  One warm-up cycle, a reading of
torch.cuda.mem_get_info(), three more cycles, a second reading; prints one JSON line
{"before": free bytes, "after": free bytes, "cycles": 3}.

A cycle makes one call of every path that allocates context memory on first use: greedy,
sampled and logprob generation, a 70-token prefill, embeddings and the engine trace on
GGUF_SINGLE's model, and a two-sequence batched generation on GGUF_BATCHED's (a model whose
layers have a batched step)."""
import json
import os
import sys

root = sys.argv[1]
for p in (os.path.join(root, "llama-gguf-inference_amd"), os.path.join(root, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.zeros(1, device="cuda")  # torch's HIP state before any libllmi call, as the suite's gpu fixture

import llmi  # noqa: E402
from llmi.sampling import SamplingParams  # noqa: E402

SAMPLED = SamplingParams(temperature=1.5, top_k=40, top_p=1.0, min_p=0.0)


def cycle(m1, m2):
    rng = np.random.default_rng(11)
    c = llmi.Context(m1, n_ctx=256, n_seq=3)
    c.generate_greedy(1, 0, 4)
    c.generate_sampled_batch([0], [1], [0], 4, [SAMPLED], rng.random((1, 4)))
    c.generate_logprobs_batch([0], [1], [0], 4, [SAMPLED], rng.random((1, 4)), [3])
    assert c.decode([1] + [int(t) for t in rng.integers(3, m1.n_vocab - 1, 69)], pos=list(range(70))) == 0
    assert c.prefill_tokens == 69
    c.set_embeddings(True)
    c.set_pooling(llmi.POOLING_MEAN)
    assert c.decode([1, 5, 9], pos=[0, 1, 2]) == 0
    c.embeddings_seq(0)
    c.set_embeddings(False)
    c.engine_trace(1, 0, 0)
    c.close()
    b = llmi.Context(m2, n_ctx=256, n_seq=3)
    b.generate_greedy_batch([0, 1], [1, 42], [0, 0], 4)
    b.close()


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def main():
    m1, m2 = llmi.Model(sys.argv[2]), llmi.Model(sys.argv[3])
    assert m1.prefill_supported
    cycle(m1, m2)
    before = free_bytes()
    for _ in range(3):
        cycle(m1, m2)
    after = free_bytes()
    print(json.dumps({"before": before, "after": after, "cycles": 3}))


if __name__ == "__main__":
    main()
