"""The step-entry kernels at kernel level (llmi_step_entry), bit for bit: k_embed, k_bembed,
k_pf_embed, k_embed_row and the dequant_elem they share.

get_rows: dequant_elem is a second inverse of k_repack_*, beside the matvec's unit loads.  Every
element of every row comes back through k_pf_embed (one launch over a permutation of the whole
vocabulary) and is held to pyoracle.dequantize of the raw GGUF bytes (which
test_step_entry_inputs.py holds to a NumPy restatement of ggml's dequantize_row_*), at the
smallest shapes that reach every row-group size and the rows % R fallback, all four types,
generic and x86 byte order, on random, saturated and fp16-scale-edge blocks.  k_embed,
k_bembed and k_embed_row fetch the rows at the group edges and must give the same bits.

Token selection and state: the crafted states of tests/step_entry_cases.py (the host token
against the fed-back one, the maximum in each of the 64 key slots, the key order's edges,
the clamps, the position edges, seq) go through k_embed and k_bembed at a one-workgroup and
a 64-workgroup shape, and the WHOLE state, history, tpos and x after the launch are held to
entry_ref, the restatement of common.h's contract: what must change and what must not.  The
hook's device buffers lie between sentinel guards, and a slot the launch does not own keeps
its sentinel row.  test_step_entry_inputs.py shows on the CPU that these inputs tell a wrong
parity, a signed or half compare, a lane left out of the maximum and a missing clamp from the
contract.

Every comparison is on integer views (signed zeros count), the references are finite.

A scratch build with the kernels broken on purpose (values only, every access in bounds):
k_embed reading key parity pos & 1, wave_max_u64 without its last step (lanes 32..63 never
reach lane 0), the Q5_K fifth bit from the other half, Q6_K without the XOR 2, Q8_0 reading
with rgs = 0, k_pf_embed recording the unclamped id.  131 of the 155 tests fail: every
group-edge test (k_embed's feedback), both k_embed and all six k_bembed state tests, the
prefill history test, and the every-element tests of Q5_K, Q6_K and Q8_0 except the four Q8_0
cases at shapes whose rgs is 0 anyway; Q4_K's every-element tests and k_embed_row pass, as
they should.

Wall time of this file alone on the MI355X: about 4 seconds (155 tests, the slowest 0.12 s)."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import llmi
import step_entry_cases as sc
from helpers import Q4_K, QTYPES, TNAME
from llmi import STEP_STATE
from llmi._lib import STEP_BEMBED, STEP_EMBED, STEP_EMBED_ROW, STEP_PF_EMBED, STEP_SENTINEL
from test_gpu_matvec_edges import numerics, repack

pytestmark = pytest.mark.gpu

NUM_IDS = ["generic", "x86"]
TSEQ = (5, 2, 7, 0, 6, 1, 4, 3)  # slot -> sequence, not the identity


def call(kernel, qtype, wd, table, n_ctx, **kw):
    import torch

    torch.cuda.synchronize()
    V, cols = table.shape
    return llmi.step_entry(kernel, qtype, wd.data_ptr(), V, cols, n_ctx, **kw)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_x(got, ref_bits, what, tokens):
    g, r = got.reshape(-1), np.ascontiguousarray(ref_bits).reshape(-1)
    bad = np.flatnonzero(g != r)
    if bad.size:
        cols = got.shape[-1]
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} x words differ, first at slot {i // cols} (token "
                             f"{tokens[i // cols]}) column {i % cols}: got 0x{int(g[i]):08x}, reference 0x{int(r[i]):08x}")


def same_state(got, exp, what):
    if got.tobytes() == exp.tobytes():
        return
    out = []
    for f in STEP_STATE.names:
        if f != "key" and got[f] != exp[f]:
            out.append(f"{f}: got {int(got[f])}, expected {int(exp[f])}")
    for p in range(2):
        lanes = np.flatnonzero(got["key"][p] != exp["key"][p])
        if lanes.size:
            l = int(lanes[0])
            out.append(f"key[{p}]: {lanes.size} slots differ, first {l}: got 0x{int(got['key'][p][l]):016x}, expected "
                       f"0x{int(exp['key'][p][l]):016x}")
    raise AssertionError(f"{what}: state after the launch: " + "; ".join(out))


def run_embed(qtype, wd, table, st, what, n_ctx=sc.N_CTX):
    """One k_embed launch on the state `st`: x, the whole state, the history and the guards."""
    V = table.shape[0]
    hist0 = sc.init_hist(1, n_ctx)
    x, st1, h1, _, bad = call(STEP_EMBED, qtype, wd, table, n_ctx, states=[st], hist=hist0)
    est, eh, tok, pos = sc.entry_ref(st, hist0[0], V, n_ctx)
    same_x(x, bits(table[tok])[None, :], what, [tok])
    same_state(st1[0], est, what)
    assert np.array_equal(h1[0], eh), f"{what}: history {h1[0].tolist()}, expected {eh.tolist()}"
    assert bad == [0, 0, 0], f"{what}: guard words changed (x, hist, states): {bad}"


def run_bembed(qtype, wd, table, states, tseq, what, n_ctx=sc.N_CTX):
    """One k_bembed launch of len(tseq) slots over the sequences `states`: the x rows (a slot
    past nt keeps the sentinel), every state and history row (a sequence outside the batch
    unchanged), tpos and the guards."""
    V, cols = table.shape
    n_seq = len(states)
    hist0 = sc.init_hist(n_seq, n_ctx)
    tpos0 = np.arange(8, dtype=np.int32) - 1000
    x, st1, h1, tp, bad = call(STEP_BEMBED, qtype, wd, table, n_ctx, states=states, hist=hist0, tseq=tseq, tpos=tpos0)
    ex = np.full((8, cols), STEP_SENTINEL, dtype=np.uint32)
    est, eh, etp, toks = [np.array(s, dtype=STEP_STATE).reshape(()) for s in states], hist0.copy(), tpos0.copy(), ["-"] * 8
    for s, q in enumerate(tseq):
        est[q], eh[q], tok, pos = sc.entry_ref(states[q], hist0[q], V, n_ctx)
        ex[s], etp[s], toks[s] = bits(table[tok]), pos, tok
    same_x(x, ex, what, toks)
    for q in range(n_seq):
        same_state(st1[q], est[q], f"{what}, sequence {q}" + ("" if q in tseq else " (not in the batch)"))
    assert np.array_equal(h1, eh), f"{what}: history rows {np.flatnonzero((h1 != eh).any(axis=1)).tolist()} differ"
    assert tp.tolist() == etp.tolist(), f"{what}: tpos {tp.tolist()}, expected {etp.tolist()}"
    assert bad == [0, 0, 0], f"{what}: guard words changed (x, hist, states): {bad}"


def stale_state(token):
    """A state whose every field but `token` would mislead a kernel that read it."""
    st = np.zeros((), dtype=STEP_STATE)
    st["token_in"], st["token_in_pos"], st["pos_next"], st["pos"], st["token"], st["seq"] = 3, 9, 9, 8, token, 77
    st["key"][:] = sc.key(0xC0000000, 5)
    return st


def run_embed_row(qtype, wd, table, token, what):
    """k_embed_row reads the clamped st->token and writes nothing but x."""
    V = table.shape[0]
    st = stale_state(token)
    x, st1, _, _, bad = call(STEP_EMBED_ROW, qtype, wd, table, sc.N_CTX, states=[st])
    tok = token if 0 <= token < V else 0
    same_x(x, bits(table[tok])[None, :], what, [tok])
    same_state(st1[0], st, what)
    assert bad == [0, 0, 0], f"{what}: guard words changed (x, hist, states): {bad}"


def row_state(row, pos_next, feedback):
    """The state that makes a step entry fetch `row`: as the host token, or fed back through
    key slot row % 64."""
    st = np.zeros((), dtype=STEP_STATE)
    st["pos_next"], st["seq"], st["pos"], st["token"] = pos_next, 1, pos_next - 1, -3
    if feedback:
        st["token_in"], st["token_in_pos"] = -9, pos_next + 1
        st["key"][(pos_next + 1) & 1][row % 64] = sc.key(0xC0000000, row)
    else:
        st["token_in"], st["token_in_pos"] = row, pos_next
    return st


# ---- get_rows ---------------------------------------------------------------------------------
GR_CASES = [pytest.param(q, shape, num, id=f"{TNAME[q]}-{shape[0]}x{shape[1]}-{NUM_IDS[num]}")
            for q in QTYPES for shape in sc.SHAPES for num in (0, 1)]


def weights(qtype, shape):
    """[(set name, device-layout weight, reference table)] in the numerics in effect."""
    out = []
    for name, raw, table in sc.references(qtype, *shape):
        assert np.isfinite(table).all(), f"{name}: non-finite reference"
        out.append((name, repack(qtype, np.array(raw), *shape), table))
    return out


@pytest.mark.parametrize("qtype,shape,num", GR_CASES)
def test_get_rows_every_element(gpu, qtype, shape, num):
    """k_pf_embed over a permutation of the whole vocabulary with repeats: every element of
    the matrix through dequant_elem, and the history of the launch."""
    V = shape[0]
    rng = np.random.default_rng(qtype + V + shape[1] + num)
    with numerics(num):
        for name, wd, table in weights(qtype, shape):
            toks = np.concatenate([rng.permutation(V), rng.integers(0, V, 9)])
            n_ctx, pos0 = len(toks) + 5, 2
            hist0 = sc.init_hist(1, n_ctx)
            x, _, h1, _, bad = call(STEP_PF_EMBED, qtype, wd, table, n_ctx, hist=hist0, tokens=toks, pos0=pos0)
            ex, eh = sc.pf_ref(table, toks, hist0, pos0, n_ctx)
            same_x(x, bits(ex), name, toks)
            assert np.array_equal(h1, eh), f"{name}: history"
            assert bad == [0, 0, 0], f"{name}: guard words changed (x, hist, states): {bad}"


@pytest.mark.parametrize("qtype,shape,num", GR_CASES)
def test_get_rows_at_the_group_edges(gpu, qtype, shape, num):
    """k_embed, k_embed_row and k_bembed (eight slots) on rows 0, 1, RG - 1, RG, RG + 1, the last
    RG + 1 rows, V - 1 and a few random ones, the token given by the host and fed back in turn."""
    rng = np.random.default_rng(qtype + shape[0] + shape[1] + num)
    with numerics(num):
        for name, wd, table in weights(qtype, shape):
            rows = sc.row_list(*shape, rng)
            for j, r in enumerate(rows):
                run_embed(qtype, wd, table, row_state(r, j % sc.N_CTX, j & 1), f"{name}, k_embed, row {r}")
                run_embed_row(qtype, wd, table, r, f"{name}, k_embed_row, row {r}")
            for j in range(0, len(rows), 8):
                chunk = rows[j: j + 8]
                states = [row_state(0, 0, 0)] * 8
                for s, r in enumerate(chunk):
                    states[TSEQ[s]] = row_state(r, (j + 3 * s) % sc.N_CTX, (s + 1) & 1)
                run_bembed(qtype, wd, table, states, TSEQ[: len(chunk)], f"{name}, k_bembed, rows {chunk}")


# ---- token selection and state ----------------------------------------------------------------
STATE_SHAPES = [pytest.param(s, id=f"{s[0]}x{s[1]}") for s in (sc.SMALL, sc.WIDE)]


@functools.lru_cache(maxsize=None)
def state_weight(shape):
    """The Q4_K random set of the shape in generic numerics."""
    name, raw, table = sc.references(Q4_K, *shape)[0]
    assert np.isfinite(table).all()
    with numerics(0):
        return repack(Q4_K, np.array(raw), *shape), table


@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_token_selection_and_state_embed(gpu, shape):
    """Every state case through k_embed: 1 workgroup (256 columns) and 64 workgroups (16384
    columns) that each derive the token."""
    wd, table = state_weight(shape)
    with numerics(0):
        for name, st in sc.state_cases(shape[0]):
            run_embed(Q4_K, wd, table, st, name)


@pytest.mark.parametrize("nt", [1, 3, 8])
@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_token_selection_and_state_bembed(gpu, shape, nt):
    """Every state case through k_bembed, eight sequences at a time, the first nt slots in the
    batch through a non-identity tseq: a different case, mode and position per slot, and the
    sequences outside the batch untouched."""
    wd, table = state_weight(shape)
    cases = sc.state_cases(shape[0])
    with numerics(0):
        for j in range(0, len(cases), nt):
            # the nt cases of this launch at the batch's sequences, other cases at the rest
            states = [cases[(j + nt + q) % len(cases)][1] for q in range(8)]
            names = []
            for s in range(nt):
                name, states[TSEQ[s]] = cases[(j + s) % len(cases)]
                names.append(name)
            run_bembed(Q4_K, wd, table, states, TSEQ[:nt], f"slots {names}")


def test_prefill_tokens_and_history(gpu):
    """k_pf_embed: T in 1, 33, 600; ids outside the vocabulary read row 0 and the history
    records the clamped id; past n_ctx the history stops and every x row is still written."""
    wd, table = state_weight(sc.SMALL)
    with numerics(0):
        for name, toks, pos0, n_ctx in sc.pf_token_cases(sc.SMALL[0]):
            hist0 = sc.init_hist(1, n_ctx)
            x, _, h1, _, bad = call(STEP_PF_EMBED, Q4_K, wd, table, n_ctx, hist=hist0, tokens=toks, pos0=pos0)
            ex, eh = sc.pf_ref(table, toks, hist0, pos0, n_ctx)
            same_x(x, bits(ex), name, toks)
            assert np.array_equal(h1, eh), f"{name}: history differs at {np.flatnonzero(h1[0] != eh[0])[:8].tolist()}"
            assert bad == [0, 0, 0], f"{name}: guard words changed (x, hist, states): {bad}"


@pytest.mark.parametrize("shape", STATE_SHAPES)
def test_embed_row_reads_the_clamped_token(gpu, shape):
    wd, table = state_weight(shape)
    V = shape[0]
    with numerics(0):
        for token in (0, 1, V // 2, V - 1, -1, V, V + 7, sc.I32_MAX, sc.I32_MIN):
            run_embed_row(Q4_K, wd, table, token, f"st->token {token}")
