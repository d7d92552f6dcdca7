"""The split-unit matvec geometry (mv_device.h "Split units": two lanes per 256-weight unit,
integer partial sums joined by one DPP add) against the CPU oracle and against the unsplit
geometry, bit for bit on the uint32 views.

The geometry is forced through llmi_test_option("mv_unit_split", v): -1 auto, 0 never, 1
every launch that can, 2 only the Q6_K group of a Q4_K + Q6_K QKV launch; "mv_split_nt"
picks the 256- or 512-thread workgroup.  (ctypes directly: the option's old value may be
-1, which llmi.test_option reads as an error.)

  llmi_matvec  Q4_K and Q6_K; 256, 512, 4096, 8192 and 14336 columns (a row is one lane
               pair; two units; 32 lanes, two rows per task; 64 lanes, one row; two
               sub-items, the second partly filled, chains carried) x 2, 6, 64 and 258 rows
               (a last task with one valid row, odd task counts, more tasks than one
               workgroup); store, accumulate and fused-RMSNorm launches; every weight set
               and activation family of the edge matrix (tests/helpers.py)
  QKV          tiny models whose attn_q / attn_k are Q4_K and attn_v Q6_K, head_dim 64 and
               128: the split-by-workgroup launch with only its Q6_K group split (2) and
               with both groups split (1), RoPE and the f16 KV write behind it
  end to end   16 greedy steps of tests/golden/tiny-mixed.gguf, option on and off
each in generic and x86 numerics and with both workgroup sizes."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import gguf_variants as gv
import llmi
import pyoracle as po
from helpers import BLOCK_BYTES, Q4_K, Q6_K, TNAME, edge_weight_sets, near_saturated_blocks, random_blocks
from test_gpu_matvec_edges import check, gpu_matvec, norm_weight, numerics, oracle, repack

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = (Q4_K, Q6_K)
NUM_IDS = ["generic", "x86"]
ROWS = (2, 6, 64, 258)
COLS = (256, 512, 4096, 8192, 14336)
NTS = (256, 512)


class split:
    """mv_unit_split = v and mv_split_nt = nt inside the block."""

    def __init__(self, v, nt=0):
        self.v, self.nt = v, nt

    def __enter__(self):
        L = llmi.lib()
        self.old = L.llmi_test_option(b"mv_unit_split", self.v)
        assert self.old >= -1, llmi.last_error()
        self.old_nt = L.llmi_test_option(b"mv_split_nt", self.nt)
        assert self.old_nt >= 0, llmi.last_error()
        return self

    def __exit__(self, *exc):
        L = llmi.lib()
        L.llmi_test_option(b"mv_unit_split", self.old)
        L.llmi_test_option(b"mv_split_nt", self.old_nt)
        return False


def test_option_values(gpu):
    L = llmi.lib()
    old = L.llmi_test_option(b"mv_unit_split", 1)
    assert old >= -1
    assert L.llmi_test_option(b"mv_unit_split", 0) == 1
    assert L.llmi_test_option(b"mv_unit_split", -1) == 0
    assert L.llmi_test_option(b"mv_unit_split", 7) < -1  # refused, unchanged
    assert L.llmi_test_option(b"mv_unit_split", old) == -1


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
@pytest.mark.parametrize("qtype", TYPES, ids=[TNAME[t] for t in TYPES])
@pytest.mark.parametrize("cols", COLS)
def test_split_matvec(gpu, qtype, cols, num):
    """Every weight set x activation family: the 258-row oracle once, its leading rows for the
    smaller launches (a row's sum does not depend on the others)."""
    rng = np.random.default_rng(cols * 7 + qtype)
    rmax = max(ROWS)
    rb = cols // 256 * BLOCK_BYTES[qtype]
    with numerics(num):
        for wname, raw, acts in edge_weight_sets(qtype, rmax, cols, rng):
            wds = {rows: repack(qtype, raw[: rows * rb], rows, cols) for rows in ROWS}
            nw = norm_weight(wname, cols, rng)
            for ai, (aname, make) in enumerate(acts):
                x = make(rng)
                ref = oracle(qtype, raw, rmax, cols, x, num)
                extra = ai < 2  # accumulate and fused-norm launches on the first two families
                if extra:
                    y0 = rng.standard_normal(rmax).astype(np.float32)
                    y0[::7] = 0.0
                    ref_add = y0 + ref
                    ref_nw = oracle(qtype, raw, rmax, cols, x, num, nw)
                    assert np.isfinite(ref_add).all()
                for rows in ROWS:
                    with split(0):
                        base = gpu_matvec(qtype, wds[rows], rows, cols, x)
                    check(base, ref[:rows], f"{wname} x {aname}, {rows} rows, unsplit")
                    for nt in NTS:
                        what = f"{wname} x {aname}, {rows} rows, {nt} threads"
                        with split(1, nt):
                            got = gpu_matvec(qtype, wds[rows], rows, cols, x)
                            check(got, ref[:rows], what)
                            check(got, base, what + " vs unsplit")
                            if extra and rows in (6, 258):
                                check(gpu_matvec(qtype, wds[rows], rows, cols, x, y0=y0[:rows]), ref_add[:rows], what + ", add")
                                check(gpu_matvec(qtype, wds[rows], rows, cols, x, nw), ref_nw[:rows], what + ", rmsnorm")
                                check(gpu_matvec(qtype, wds[rows], rows, cols, x, nw, y0=y0[:rows]),
                                      (y0 + ref_nw)[:rows], what + ", rmsnorm + add")


# ---- the Q4_K + Q6_K QKV launch ------------------------------------------------------------
def edit_qkv_q4q6(g: gv.Gguf):
    """attn_q / attn_k Q4_K, attn_v Q6_K in every layer: layer 0 random blocks, the others
    near-saturated ones (quants and scales at the top of their ranges)."""
    for t in list(g.tensors):
        if not t.name.endswith(("attn_q.weight", "attn_k.weight", "attn_v.weight")):
            continue
        cols, rows = t.ne
        qt = Q6_K if t.name.endswith("attn_v.weight") else Q4_K
        rng = np.random.default_rng(len(t.name) + rows + qt)
        raw = random_blocks(qt, rows, cols, rng) if t.name.startswith("blk.0.") else near_saturated_blocks(qt, rows, cols, rng)[0]
        g.replace_tensor(t.name, [cols, rows], qt, raw.tobytes())


def decode_steps(path, toks, num, n_ctx=64):
    m = llmi.Model(path, numerics=llmi.NUMERICS_X86 if num else llmi.NUMERICS_GENERIC)
    c = llmi.Context(m, n_ctx=n_ctx)
    out = []
    for pos, t in enumerate(toks):
        assert c.decode([t], pos=[pos]) == 0, llmi.last_error()
        out.append(c.logits(-1).copy())
    c.close()
    m.close()
    return np.stack(out)


@pytest.fixture(scope="module")
def qkv_models(tiny_models, synth_dir):
    """path and oracle logits (generic, x86) of the two Q4_K + Q6_K QKV models, computed once"""
    toks = [1, 42, 7, 300, 5, 611]
    out = {}
    for preset in ("tiny-mixed", "tiny-mixed-d128"):
        path = gv._variant(tiny_models[preset], synth_dir, "qkvq4q6", edit_qkv_q4q6)
        refs = []
        for x86 in (0, po.X86_ALL):
            om = po.OracleModel(path, n_ctx=64, x86=x86)
            refs.append(np.stack([om.decode(t, p) for p, t in enumerate(toks)]))
            om.close()
        out[preset] = (path, toks, refs)
    return out


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("mode", [2, 1], ids=["q6k-group", "both-groups"])
@pytest.mark.parametrize("preset", ["tiny-mixed", "tiny-mixed-d128"], ids=["d64", "d128"])
def test_split_qkv_two_types(gpu, qkv_models, preset, mode, nt, num):
    path, toks, refs = qkv_models[preset]
    with split(0):
        base = decode_steps(path, toks, num)
    with split(mode, nt):
        got = decode_steps(path, toks, num)
    for p in range(len(toks)):
        check(got[p], refs[num][p], f"step {p} vs oracle")
        check(got[p], base[p], f"step {p} vs unsplit")


@pytest.mark.parametrize("num", [0, 1], ids=NUM_IDS)
def test_split_greedy16_on_and_off(gpu, num):
    path = os.path.join(HERE, "golden", "tiny-mixed.gguf")
    runs = []
    for v in (1, 0):
        with split(v):
            m = llmi.Model(path, numerics=llmi.NUMERICS_X86 if num else llmi.NUMERICS_GENERIC)
            c = llmi.Context(m, n_ctx=64)
            cur, ids, lgs = 1, [], []
            for pos in range(16):
                assert c.decode([cur], pos=[pos]) == 0, llmi.last_error()
                lgs.append(c.logits(-1).copy())
                cur = c.greedy(-1)
                ids.append(cur)
            c.close()
            m.close()
            runs.append((ids, np.stack(lgs)))
    assert runs[0][0] == runs[1][0]
    check(runs[0][1], runs[1][1], "logits, split on vs off")
