"""The QKV, SwiGLU and logits epilogues at kernel level (llmi_mv_epilogue), bit for bit.

The matvec / GEMM parity tests (test_gpu_matvec_edges.py) stop at the row sum and reach only
the STORE and ADD epilogues.  Here the three epilogues that do arithmetic and scattered
writes of their own run without a model, in every kernel that has them:

  kernel 0  launch_matvec: k_matvec, and k_matvec_split under every mv_unit_split value that
            changes the launch of the type set (test_gpu_mv_split.py)
  kernel 1  launch_mvn: k_mvn, nt padded to 1, 2, 4, 8
  kernel 2  launch_bmm: k_bmd, and k_bmm under LLMI_BMM_DMA=0 (generic numerics only)
  kernel 3  launch_pf_gemm: k_pf_gemm's own epilogue (the RoPE partner from the lane beside,
            the q / k / v part from r1 / r2; with the pf_qkv_merge option on and off)
  kernel 4  launch_bmm_qkv2: k_bmd2, the QKV of two type groups in one launch

on the inputs of tests/epilogue_cases.py (checked on the CPU by test_epilogue_inputs.py): row
sums that overflow f16, are f16 subnormals, round to f16 zero and sit on exact f16 ties; gate
values in every band between llmi_expf's and x86_v_expf's switch points; logits that tie
bit for bit in one row pair, across workgroups and key slots, in the odd last row, that are
all negative, and whose maximum is zero.

Reference = the oracle's row sums (bit-equal to the kernels' by test_gpu_matvec_edges.py) +
the NumPy restatement of the epilogue in epilogue_cases.py, compared on the integer views.
q, the caches and y start as a sentinel NaN pattern that no result takes; the expectation is
that image with exactly the written entries replaced, so a write to a wrong position, head,
slot or stride shows, as does a write by a padded slot.  A combination a kernel does not
take is left out of the lists below (test_epilogue_abi.py checks that the hook refuses it).

Scratch builds with an epilogue broken on purpose: V written at the next position fails every
QKV test here (380).  f2h without its asm barrier compiles to the same code in every epilogue
instantiation (k_matvec, k_mvn, k_bmd, k_pf_gemm: the compiler folds only the f2h(a * b) sites of
the attention kernels), and `>=` for `>` in the key reduces changes nothing, since a key holds
its row and no two keys are equal: neither can fail a test.  What the tie sets do catch is a
wrong ORDER of equal logits: with the key's row part stored so that the last row wins, every
tie set but the single-winner one fails in k_matvec, k_mvn, k_bmd and k_bmm (250 of 300).

Wall time of this file alone on the MI355X: about 15 seconds (828 cases)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import epilogue_cases as ec
import llmi
from helpers import Q4_K, Q5_K, Q6_K, Q8_0, TNAME
from helpers import to_dev as _to_dev
from llmi._lib import EPI_LOGITS, EPI_QKV, EPI_SWIGLU, llmi_epilogue_args
from test_gpu_matvec_edges import numerics, repack
from test_gpu_mv_split import split

pytestmark = pytest.mark.gpu

NUM_IDS = ["generic", "x86"]
SENT32 = 0x7FC5A5A5   # f32 NaN with a payload
SENT16 = 0x7E5A       # f16 NaN with a payload
KQUANTS = (Q4_K, Q5_K, Q6_K)


def to_dev(a):
    return _to_dev(np.array(a))  # (a copy: the cases' arrays are read-only)


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def sentinel32(*shape):
    import torch

    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda")


def sentinel16(*shape):
    import torch

    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda")


class Weights:
    """The device-layout weights and the norm weights of a case in the numerics in effect."""

    def __init__(self, types, raws, rows, cols, base):
        self.types, self.rows, self.cols = types, rows, cols
        self.w = [repack(t, np.array(raw), r, cols) for t, raw, r in zip(types, raws, rows)]
        self.nw = [to_dev(ec.family_nw(base, s)) for s in ec.FAMILIES]

    def args(self, kernel, epi, f, xd, nt):
        a = llmi_epilogue_args()
        a.kernel, a.epi, a.cols, a.eps, a.nt = kernel, epi, self.cols, ec.EPS, nt
        for i, (t, w, r) in enumerate(zip(self.types, self.w, self.rows)):
            a.type[i], a.w_dev[i], a.rows[i] = t, w.data_ptr(), r
        a.x_dev, a.norm_w_dev = xd.data_ptr(), self.nw[f].data_ptr()
        return a


def call(a):
    import torch

    torch.cuda.synchronize()
    rc = llmi.lib().llmi_mv_epilogue(C.byref(a))
    assert rc == 0, llmi.last_error()


def diff32(got, ref, what, where=lambda i: f"index {i}"):
    g = np.ascontiguousarray(got).view(np.uint32).reshape(-1)
    r = np.ascontiguousarray(ref).view(np.uint32).reshape(-1)
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ, first at {where(int(bad[0]))}: got 0x{int(g[bad[0]]):08x}, "
                           f"reference 0x{int(r[bad[0]]):08x}")


def diff16(got, ref, what, where):
    g = np.ascontiguousarray(got).view(np.uint16).reshape(-1)
    r = np.ascontiguousarray(ref).view(np.uint16).reshape(-1)
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} differ, first at {where(int(bad[0]))}: got 0x{int(g[bad[0]]):04x}, "
                           f"reference 0x{int(r[bad[0]]):04x}")


# ---- QKV -----------------------------------------------------------------------------------
def run_qkv(c, W, kernel, f, tokens, positions, slots):
    """One hook call over `tokens` (indices into c.X) at `positions`, token i writing cache
    slot slots[i] of `max(slots) + 1` caches; compares q and the whole caches."""
    nt = len(tokens)
    ns = max(slots) + 1
    xd = to_dev(c.X[list(tokens)])
    q = sentinel32(nt, c.nq)
    kc = sentinel16(ns, c.HK, ec.N_CTX, c.D)
    vc = sentinel16(ns, c.HK, c.D, ec.N_CTX)
    rope = to_dev(c.rope)
    a = W.args(kernel, EPI_QKV, f, xd, nt)
    a.head_dim, a.n_rot, a.n_ctx = c.D, c.n_rot, ec.N_CTX
    a.rope_dev, a.q_dev, a.kc_dev, a.vc_dev = rope.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr()
    pos = _i32(positions[:1] if kernel == 3 else positions)
    a.pos = pos
    call(a)
    eq = np.empty((nt, c.nq), dtype=np.float32)
    ek = np.full((ns, c.HK, ec.N_CTX, c.D), SENT16, dtype=np.uint16)
    ev = np.full((ns, c.HK, c.D, ec.N_CTX), SENT16, dtype=np.uint16)
    for i, (t, p, s) in enumerate(zip(tokens, positions, slots)):
        eq[i], k, v = c.token(f, t, p)
        ek[s, :, p, :] = k.view(np.uint16)
        ev[s, :, :, p] = v.view(np.uint16)
    what = f"family {ec.FAMILY_IDS[f]}, nt {nt}, positions {list(positions)[:8]}"
    diff32(q.cpu().numpy(), eq, what + ", q", lambda i: f"(token {i // c.nq}, head {i % c.nq // c.D}, dim {i % c.D})")

    def kw(i):
        s, h, p, d = np.unravel_index(i, ek.shape)
        return f"(slot {s}, head {h}, dim {d}, position {p})"

    def vw(i):
        s, h, d, p = np.unravel_index(i, ev.shape)
        return f"(slot {s}, head {h}, dim {d}, position {p})"

    diff16(kc.cpu().numpy(), ek, what + ", K cache", kw)
    diff16(vc.cpu().numpy(), ev, what + ", V cache", vw)


def qkv_weights(c):
    return Weights(c.tset, c.raw, c.rows, c.cols, c.base)


# mv_unit_split values (and the workgroup threads of a split launch) that change kernel 0's
# launch of a type set: Q4_K / Q6_K alone split under 1 (3 = auto does the same at these
# single-round shapes); Q4_K + Q6_K runs k_matvec's two-type form under 0, only its Q6_K
# group split under 2 (= auto), both under 1; of Q8_0 + Q6_K the Q6_K v launch splits under 1;
# Q5_K and Q8_0 have no split form
QKV_SPLITS = {
    (Q4_K, Q4_K, Q4_K): ((0, 0), (1, 256), (1, 512)),
    (Q5_K, Q5_K, Q5_K): ((-1, 0),),
    (Q6_K, Q6_K, Q6_K): ((0, 0), (1, 256)),
    (Q8_0, Q8_0, Q8_0): ((-1, 0),),
    (Q4_K, Q4_K, Q6_K): ((0, 0), (2, 256), (1, 256), (1, 512)),
    (Q8_0, Q8_0, Q6_K): ((0, 0), (1, 256)),
}
QKV_CASES = [(ts, sh, num) for ts in ec.QKV_TYPE_SETS for sh in ec.QKV_SHAPES for num in (0, 1)]


def _qid(ts, sh, num):
    return f"{ec.tset_id(ts)}-D{sh[0]}-rot{sh[1]}-{sh[2]}-{NUM_IDS[num]}"


@pytest.mark.parametrize("ts,sh,num,sp", [pytest.param(ts, sh, num, sp, id=f"{_qid(ts, sh, num)}-split{sp[0]}-{sp[1]}")
                                          for ts, sh, num in QKV_CASES for sp in QKV_SPLITS[ts]])
def test_qkv_decode(gpu, ts, sh, num, sp):
    """k_matvec / k_matvec_split: one token per launch at positions 0, 1 and n_ctx - 1."""
    c = ec.qkv_case(ts, *sh, num)
    with numerics(num), split(*sp):
        W = qkv_weights(c)
        for f in range(len(ec.FAMILIES)):
            for t, p in enumerate(ec.DECODE_POS):
                run_qkv(c, W, 0, f, (t,), (p,), (0,))


def _batched(c, W, kernel):
    for nt in ec.BATCH_NT:
        for f in range(len(ec.FAMILIES)):
            run_qkv(c, W, kernel, f, tuple(range(nt)), ec.BATCH_POS[nt], tuple(range(nt)))


@pytest.mark.parametrize("ts,sh,num", [pytest.param(*c, id=_qid(*c)) for c in QKV_CASES])
def test_qkv_mvn(gpu, ts, sh, num):
    """k_mvn, one launch per run of same-type segments; padded slots land in the hook's dummy
    cache, two slots at one position in their own caches."""
    c = ec.qkv_case(ts, *sh, num)
    with numerics(num):
        _batched(c, qkv_weights(c), 1)


# the matrix-core kernels take K-quant segments only; k_bmm (LLMI_BMM_DMA=0) has no x86 fold
BMM_QKV = [(ts, sh, num, dma) for ts, sh, num in QKV_CASES if Q8_0 not in ts for dma in (1, 0) if dma or not num]


@pytest.mark.parametrize("ts,sh,num,dma", [pytest.param(*c, id=f"{_qid(*c[:3])}-{'k_bmd' if c[3] else 'k_bmm'}")
                                           for c in BMM_QKV])
def test_qkv_bmm(gpu, monkeypatch, ts, sh, num, dma):
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    c = ec.qkv_case(ts, *sh, num)
    with numerics(num):
        _batched(c, qkv_weights(c), 2)


@pytest.mark.parametrize("ts,sh,num", [pytest.param(*c, id=_qid(*c)) for c in QKV_CASES if c[0] == (Q4_K, Q4_K, Q6_K)])
def test_qkv_bmd2(gpu, ts, sh, num):
    """launch_bmm_qkv2: the q / k rows and the attn_v rows of another type in one k_bmd2 launch."""
    c = ec.qkv_case(ts, *sh, num)
    with numerics(num):
        _batched(c, qkv_weights(c), 4)


@pytest.mark.parametrize("merge", [1, 0], ids=["merge", "nomerge"])
@pytest.mark.parametrize("ts,sh,num", [pytest.param(*c, id=_qid(*c)) for c in QKV_CASES])
def test_qkv_prefill(gpu, ts, sh, num, merge):
    """k_pf_gemm: T tokens at consecutive positions from 0 and up to the last of the context."""
    c = ec.qkv_case(ts, *sh, num)
    old = llmi.test_option("pf_qkv_merge", merge)
    try:
        with numerics(num):
            W = qkv_weights(c)
            for T in ec.PREFILL_T:
                for pos0 in (0, ec.N_CTX - T):
                    for f in range(len(ec.FAMILIES)):
                        run_qkv(c, W, 3, f, tuple(range(T)), tuple(range(pos0, pos0 + T)), (0,) * T)
    finally:
        llmi.test_option("pf_qkv_merge", old)


# ---- SwiGLU --------------------------------------------------------------------------------
def run_swiglu(c, W, kernel, f, tokens):
    nt = len(tokens)
    xd = to_dev(c.X[list(tokens)])
    y = sentinel32(nt, c.rows)
    a = W.args(kernel, EPI_SWIGLU, f, xd, nt)
    a.y_dev = y.data_ptr()
    call(a)
    diff32(y.cpu().numpy(), c.h[f][list(tokens)], f"family {ec.FAMILY_IDS[f]}, tokens {list(tokens)}",
           lambda i: f"(token {tokens[i // c.rows]}, row {i % c.rows}: gate {c.gate[f][tokens[i // c.rows]][i % c.rows]!r}, "
                     f"up {c.up[f][tokens[i // c.rows]][i % c.rows]!r})")


SW_SHAPES = [(r, cl) for r in ec.SWIGLU_ROWS for cl in ec.SWIGLU_COLS]
# kernel 0 and 3 take gate and up of two types of one activation kind (task_any; SWIGLU_UP),
# k_mvn and the matrix-core kernels one type; the latter K-quants only
SW_CASES = [(k, ts, sh, num, dma) for k in (0, 1, 2, 3) for ts in ec.SWIGLU_TYPE_SETS for sh in SW_SHAPES for num in (0, 1)
            for dma in ((1, 0) if k == 2 else (1,))
            if (k in (0, 3) or ts[0] == ts[1]) and (k != 2 or (ts[0] in KQUANTS and (dma or not num)))]


def _swid(k, ts, sh, num, dma):
    kn = {0: "k_matvec", 1: "k_mvn", 2: "k_bmd" if dma else "k_bmm", 3: "k_pf_gemm"}[k]
    return f"{kn}-{ec.tset_id(ts)}-{sh[0]}x{sh[1]}-{NUM_IDS[num]}"


@pytest.mark.parametrize("k,ts,sh,num,dma", [pytest.param(*c, id=_swid(*c)) for c in SW_CASES])
def test_swiglu(gpu, monkeypatch, k, ts, sh, num, dma):
    """silu(gate) * up with gate values on both sides of every switch point of the two expf
    forms (the zero of g / inf * u keeps its sign)."""
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    c = ec.swiglu_case(ts, *sh, num)
    with numerics(num):
        W = Weights(c.tset, c.raw, (c.rows, c.rows), c.cols, c.base)
        for f in range(len(ec.FAMILIES)):
            if k == 0:
                for t in range(ec.SWIGLU_TOKENS):
                    run_swiglu(c, W, 0, f, (t,))
            else:
                for nt in (3, ec.SWIGLU_TOKENS):
                    run_swiglu(c, W, k, f, tuple(range(nt)))


# ---- logits --------------------------------------------------------------------------------
LOGIT_POS = (5, 6, 0, 255, 17, 17, 100, 3)


def run_logits(c, W, kernel, f, tokens):
    nt = len(tokens)
    xd = to_dev(c.X[list(tokens)])
    y = sentinel32(nt, c.rows)
    a = W.args(kernel, EPI_LOGITS, f, xd, nt)
    a.y_dev = y.data_ptr()
    pos, tok, nxt = _i32([LOGIT_POS[t] for t in tokens]), _i32([-7] * nt), _i32([-7] * nt)
    a.pos, a.token_out, a.pos_next_out = pos, tok, nxt
    call(a)
    what = f"{c.lset}, family {ec.FAMILY_IDS[f]}, tokens {list(tokens)}"
    diff32(y.cpu().numpy(), c.logits[f][list(tokens)], what, lambda i: f"(token {tokens[i // c.rows]}, row {i % c.rows})")
    want = [c.winner(f, t) for t in tokens]
    assert list(tok) == want, f"{what}: argmax {list(tok)}, reference {want} (token 0's tied rows: {c.tied[:8]})"
    assert list(nxt) == [LOGIT_POS[t] + 1 for t in tokens], f"{what}: pos_next {list(nxt)}"


LG_CASES = [(k, q, rows, ls, num, dma) for k in (0, 1, 2) for q in (Q4_K, Q5_K, Q6_K, Q8_0)
            for rows in ((80, 1008) if k == 2 else (33, 1001)) for ls in ec.LOGIT_SETS for num in (0, 1)
            for dma in ((1, 0) if k == 2 else (1,)) if k != 2 or (q in KQUANTS and (dma or not num))]


def _lgid(k, q, rows, ls, num, dma):
    kn = {0: "k_matvec", 1: "k_mvn", 2: "k_bmd" if dma else "k_bmm"}[k]
    return f"{kn}-{TNAME[q]}-{rows}-{ls}-{NUM_IDS[num]}"


@pytest.mark.parametrize("k,q,rows,ls,num,dma", [pytest.param(*c, id=_lgid(*c)) for c in LG_CASES])
def test_logits(gpu, monkeypatch, k, q, rows, ls, num, dma):
    """The logits store, the argmax key reduce of each kernel (first maximum wins) and
    pos_next, every slot with its own activations, state and position parity."""
    monkeypatch.setenv("LLMI_BMM_DMA", str(dma))
    c = ec.logit_case(q, rows, ls, num)
    with numerics(num):
        W = Weights((q,), (c.raw,), (rows,), c.cols, c.base)
        for f in range(len(ec.FAMILIES)):
            if k == 0:
                for t in range(ec.LOGIT_TOKENS):
                    run_logits(c, W, 0, f, (t,))
            else:
                for nt in ec.BATCH_NT:
                    run_logits(c, W, k, f, tuple(range(nt)))
