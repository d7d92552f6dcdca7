"""Embedding post-processing on the host, as llama-server's (upstream common_embd_normalize).

The device pools (embd.hip); normalisation is the server's job.  Everything here restates
upstream's arithmetic operation for operation, so a vector served by /v1/embeddings has the
bits upstream's server would give for the same pooled vector.
"""
from __future__ import annotations

import numpy as np

from ._lib import POOLING_CLS, POOLING_LAST, POOLING_MEAN, POOLING_NONE

POOLING_NAMES = {"none": POOLING_NONE, "mean": POOLING_MEAN, "cls": POOLING_CLS, "last": POOLING_LAST}


def normalize(v, embd_normalize: int = 2) -> np.ndarray:
    """common_embd_normalize for the two modes the server offers.

    2 (default), Euclidean: sum = sum of (double)(v[i]*v[i]) with the product in f32, in index
    order; norm = (float)(1.0 / sqrt(sum)) if sum > 0 else 0; out[i] = v[i] * norm in f32.
    -1: no normalisation.  Any other value raises ValueError."""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
    if embd_normalize == -1:
        return v.copy()
    if embd_normalize != 2:
        raise ValueError(f"embd_normalize {embd_normalize!r} is not supported (2 euclidean, -1 none)")
    total = 0.0
    for p in (v * v).tolist():  # the f32 products, widened and summed in order
        total += p
    norm = np.float32(1.0 / np.sqrt(total)) if total > 0.0 else np.float32(0.0)
    return v * norm
