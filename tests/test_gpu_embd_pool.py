"""k_embd_rows / k_embd_mean at kernel level (llmi_embd_pool over torch tensors as device
memory): the normed rows and every pooling equal, bit for bit, pyoracle.rms_norm_mul per row
followed by the pooling of include/llmi.h restated in NumPy with an explicit sequential FP64
loop over the tokens; feeding the tokens in chunks with the accumulator carried gives the bits
of one call; and `out` is written exactly where the header says and nowhere else.

Inputs.  rms_norm_mul sums a row's squares sequentially, the device in the logits prologue's
parallel order (mv_norm_scale).  The two agree for certain only when no partial sum rounds, so
every row is built to make its sum of squares exact in any order, and the test asserts that
on the CPU for every row before anything runs (no row is skipped): the rows are normal draws
rounded to multiples of 2^-6 (squares: multiples of 2^-12 with at most 20 significant bits,
exact in f32) times a power of two 2^k per row, k in [-8, 8]; one row of zeros; one row that is
zero but for one huge element (2^60).  A continuous normal row cannot pass at these widths: a
few elements per thousand are below 2^-8, and their squares carry bits below the ulp of a
double near the row's total.  The columns past n_embd of a wider buffer (ldx > n_embd) hold
NaNs: nothing may read them."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import llmi
import pyoracle as po
from helpers import to_dev

pytestmark = pytest.mark.gpu

EPS = 1e-5
SENT = np.uint32(0x7FC5A5A5)  # a NaN no computation produces
EMBD = (256, 1280, 8192)      # fewer sub-blocks than threads, an odd count of 256-blocks, > 1 sub-block per thread
NTOK = (1, 2, 63, 64, 65, 513)
POOLINGS = {"none": llmi.POOLING_NONE, "mean": llmi.POOLING_MEAN, "cls": llmi.POOLING_CLS, "last": llmi.POOLING_LAST}
SEED = 20240


def _ulp32(v: float) -> float:
    return float(np.spacing(np.float32(v)))


@functools.lru_cache(maxsize=None)
def case(n_embd: int, n_tok: int):
    """(x [n_tok][n_embd], w, y the normed rows) -- computed once, shared, read-only."""
    rng = np.random.default_rng(SEED + 7 * n_embd + n_tok)
    x = np.round(rng.standard_normal((n_tok, n_embd)) * 64.0) / 64.0
    x = (x * np.exp2(rng.integers(-8, 9, size=(n_tok, 1)))).astype(np.float32)
    if n_tok >= 2:
        x[n_tok // 2] = 0.0                                # a row of zeros
    if n_tok >= 3:
        x[n_tok // 3] = 0.0                                # a row with one huge element
        x[n_tok // 3, int(rng.integers(0, n_embd))] = np.float32(2.0 ** 60)
    # the exactness of every row's sum of squares, in any order
    sq = x * x                                             # f32 products, as the device's and the oracle's
    seq = np.cumsum(sq.astype(np.float64), axis=1)[:, -1]  # the sequential FP64 sum
    for t in range(n_tok):
        row = sq[t].astype(np.float64)
        assert math.fsum(row.tolist()) == float(seq[t]), f"row {t}: the sequential sum of squares rounds"
        nz = row[row > 0.0]
        if nz.size:
            assert float(seq[t]) < 2.0 ** 53 * _ulp32(float(nz.min())), f"row {t}: a partial sum can round"
    w = rng.standard_normal(n_embd).astype(np.float32)
    y = np.stack([po.rms_norm_mul(x[t], w, EPS) for t in range(n_tok)])
    for a in (x, w, y):
        a.setflags(write=False)
    return x, w, y


def reference(y: np.ndarray, pooling: int):
    """(out, acc): include/llmi.h's pooling of the normed rows y; acc the mean's FP64 sums."""
    n = y.shape[0]
    if pooling == llmi.POOLING_NONE:
        return y, None
    if pooling == llmi.POOLING_CLS:
        return y[0], None
    if pooling == llmi.POOLING_LAST:
        return y[-1], None
    inv = np.float32(1.0) / np.float32(n)
    acc = np.zeros(y.shape[1], dtype=np.float64)
    for t in range(n):                                     # strictly in token order
        acc = acc + (y[t] * inv).astype(np.float64)        # the product in f32, the sum in FP64
    return acc.astype(np.float32), acc


class Device:
    """x (rows ldx apart, NaN padding), w, a sentinel-filled out with one row to spare, and
    acc (garbage, one sentinel past the end) on the device."""

    def __init__(self, x, w, ldx, pooling):
        n_tok, E = x.shape
        xp = np.full((n_tok, ldx), np.nan, dtype=np.float32)
        xp[:, :E] = x
        self.n_tok, self.E, self.ldx, self.pooling = n_tok, E, ldx, pooling
        self.x, self.w = to_dev(xp), to_dev(np.array(w))
        self.rows = n_tok if pooling == llmi.POOLING_NONE else 1
        self.out = to_dev(np.full((self.rows + 1, E), SENT, dtype=np.uint32))
        self.acc = to_dev(np.full(E + 1, 1e300, dtype=np.float64))

    def run(self, t0, n, n_total=None):
        out = self.out.data_ptr() + (4 * self.E * t0 if self.pooling == llmi.POOLING_NONE else 0)
        acc = self.acc.data_ptr() if self.pooling == llmi.POOLING_MEAN else 0
        return llmi.embd_pool(self.x.data_ptr() + 4 * self.ldx * t0, self.ldx, n, self.E, self.w.data_ptr(), EPS,
                              self.pooling, self.n_tok if n_total is None else n_total, t0, acc, out)

    def out_bits(self):
        return self.out.cpu().numpy()

    def acc_host(self):
        return self.acc.cpu().numpy()


def check(dev: Device, y: np.ndarray, what: str):
    want, acc = reference(y, dev.pooling)
    got = dev.out_bits()
    wb = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32).reshape(dev.rows, dev.E)
    bad = np.flatnonzero(got[:dev.rows] != wb)
    assert bad.size == 0, f"{what}: {bad.size} of {wb.size} values differ, first at {int(bad[0])}"
    assert np.all(got[dev.rows] == SENT), f"{what}: the row past the end was written"
    a = dev.acc_host()
    assert a[dev.E] == 1e300, f"{what}: acc was written past its end"
    if acc is not None:
        assert np.array_equal(a[:dev.E].view(np.uint64), acc.view(np.uint64)), f"{what}: the FP64 sums differ"
    else:
        assert np.all(a == 1e300), f"{what}: acc was written by a pooling that has none"


CASES = [(E, E + pad, n) for E in EMBD for pad in (0, 256) for n in NTOK]


@pytest.mark.parametrize("pooling", list(POOLINGS))
@pytest.mark.parametrize("n_embd,ldx,n_tok", CASES, ids=[f"e{e}-ld{l}-t{n}" for e, l, n in CASES])
def test_one_call_and_chunked_equal_the_reference(gpu, n_embd, ldx, n_tok, pooling):
    x, w, y = case(n_embd, n_tok)
    p = POOLINGS[pooling]
    dev = Device(x, w, ldx, p)
    us = dev.run(0, n_tok)
    assert us > 0.0
    check(dev, y, "one call")
    # the same tokens in chunks, acc carried: each cut alone, then all of them at once
    cuts = sorted({c for c in (1, 64, n_tok - 1) if 0 < c < n_tok})
    for cs in [[c] for c in cuts] + ([cuts] if len(cuts) > 1 else []):
        dev = Device(x, w, ldx, p)
        edges = [0] + cs + [n_tok]
        for a, b in zip(edges, edges[1:]):
            dev.run(a, b - a)
        check(dev, y, f"chunks cut at {cs}")


@pytest.mark.parametrize("pooling", ["mean", "cls", "last"])
def test_out_is_written_only_by_the_deciding_chunk(gpu, pooling):
    """CLS writes out with the chunk at t0 == 0 only, LAST and MEAN with the chunk that ends
    the sequence only: every other chunk leaves a sentinel-filled out as it was."""
    n_embd, n_tok = 1280, 65
    x, w, y = case(n_embd, n_tok)
    p = POOLINGS[pooling]
    for t0, n in ((0, 64), (1, 63), (1, 64), (64, 1)):
        dev = Device(x, w, n_embd, p)
        dev.run(t0, n)
        decides = t0 == 0 if p == llmi.POOLING_CLS else t0 + n == n_tok
        written = bool(np.any(dev.out_bits()[0] != SENT))
        assert written == decides, f"chunk [{t0}, {t0 + n}) of {n_tok}: out written = {written}"
        assert np.all(dev.out_bits()[1] == SENT)
    if p != llmi.POOLING_MEAN:  # the deciding chunk alone gives the row, whatever the others were
        dev = Device(x, w, n_embd, p)
        dev.run(*((0, 1) if p == llmi.POOLING_CLS else (64, 1)))
        check(dev, y, "the deciding chunk alone")


def test_timing_hook_reports_microseconds(gpu):
    """The hook's usec for the shapes DESIGN.md quotes, printed (nothing asserts a time)."""
    for n_embd in (4096, 8192):
        rng = np.random.default_rng(n_embd)
        x = rng.standard_normal((512, n_embd)).astype(np.float32)
        dev = Device(x, rng.standard_normal(n_embd).astype(np.float32), n_embd, llmi.POOLING_MEAN)
        dev.run(0, 512)
        us = [dev.run(0, 512) for _ in range(5)]
        print(f"llmi_embd_pool 512 x {n_embd} mean: {min(us):.1f} us (min of 5), {sorted(us)[2]:.1f} us (median)")
        assert min(us) > 0.0
