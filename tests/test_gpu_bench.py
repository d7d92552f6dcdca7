"""bench.py's plain run, --dump-outputs and --full, in-process on a tiny preset.

A plain run times its window and nothing else; --dump-outputs writes what the last timed
step computed (tokens / hidden / logits), the same arrays from run to run (bench.py itself
reruns the last step and refuses to write arrays the rerun does not reproduce).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402

PRESET = "tiny-mixed-d128"
STEPS, WARMUP, PROMPT = 5, 3, 128
FULL_ONLY = ("c2_full", "roofline", "prefill", "other_numerics", "continuous_batching", "cpu_baseline")


def _bench(model_dir, *extra):
    return bench.main(["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--prompt", str(PROMPT),
                       "--preset", PRESET, "--model-dir", str(model_dir), *extra])


def test_full_and_dump_outputs_are_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(gpu, tmp_path):
    r = _bench(tmp_path / "m", "--dump-outputs", str(tmp_path / "a"))
    assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["full"] is False
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(1e3 / r["ms_per_step"], rel=2e-3)
    for k in FULL_ONLY:
        assert r[k] is None, f"{k} ran in a plain run"
    assert r["kernels"] == {}
    w0, w1 = r["config"]["timed_window"]
    assert w1 - w0 == STEPS and w0 == bench.window_start(PROMPT, STEPS, WARMUP)

    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("tokens", "hidden", "logits")}
    assert r["outputs"] == {n: list(v.shape) for n, v in a.items()}
    assert a["tokens"].dtype == np.float64 and a["tokens"].shape == (STEPS,)
    assert a["hidden"].dtype == np.float32 and a["logits"].dtype == np.float32
    assert int(np.argmax(a["logits"])) == int(a["tokens"][-1])

    # the same arguments again: the same inputs, so the same arrays
    _bench(tmp_path / "m", "--dump-outputs", str(tmp_path / "b"))
    for n, v in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / f"{n}.npy"), v), f"{n} differs between two runs"


@pytest.mark.gpu
def test_full_run_reports_the_other_legs(gpu, tmp_path):
    import llmi

    r = _bench(tmp_path / "m", "--full", "--no-cpu-baseline", "--no-other-numerics", "--batch-seqs", "2",
               "--batch-steps", "4", "--profile-steps", "2")
    assert r["full"] is True and r["steps"] == STEPS and r["outputs"] is None
    assert r["c2_full"]["tokens"] == bench.C2_DECODE and r["c2_full"]["tok_s"] > 0
    assert r["prefill"]["tokens"] == PROMPT and r["prefill"]["ttft_ms"] > 0
    assert set(r["kernels"]) == set(llmi.Context.KERNEL_CLASSES)
    assert r["roofline"]["bound"] == "hbm" and any(v["us"] > 0 for v in r["kernels"].values())
    assert r["continuous_batching"]["sequences"]["2"]["tok_s"] > 0
