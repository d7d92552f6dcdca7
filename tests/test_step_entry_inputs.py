"""The inputs of the step-entry tests (tests/step_entry_cases.py) on the CPU: the two
statements of the get_rows reference agree bit for bit on every weight set, the NumPy model of
the device layout inverts itself, and every deliberately wrong variant -- of the layout read
and of the token / state contract -- is told from the right one by a named case."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import step_entry_cases as sc
from helpers import Q4_K, Q5_K, Q6_K, QTYPES, TNAME

IDS = [TNAME[q] for q in QTYPES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_shapes_reach_every_row_group():
    got = {shape: sc.layout_rgs(*shape) for shape in sc.SHAPES}
    assert set(got.values()) == {0, 1, 2, 3, 4}, got
    # two of them through the rows % R fallback: the width alone would give 16 rows per group
    assert got[(1001, 256)] == 0 and got[(1004, 512)] == 2
    assert sc.layout_rgs(1008, 256) == 4 and sc.layout_rgs(1008, 512) == 4
    # the table of the module's docstring
    assert [got[s] for s in sc.SHAPES] == [4, 0, 2, 3, 2, 2, 1, 1, 0]


@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_and_numpy_dequantize_agree(qtype, shape):
    """pyoracle.dequantize and the NumPy restatement of ggml's dequantize_row_*, bit for bit
    on every weight set of the matrix; and all of it finite."""
    for name, raw, table in sc.references(qtype, *shape):
        assert np.isfinite(table).all(), name
        mine = sc.dequant_np(qtype, raw, *shape)
        bad = np.flatnonzero(bits(mine).reshape(-1) != bits(table).reshape(-1))
        assert bad.size == 0, (f"{name}: {bad.size} differ, first at row {bad[0] // shape[1]} col {bad[0] % shape[1]}: numpy "
                               f"{mine.reshape(-1)[bad[0]]!r}, oracle {table.reshape(-1)[bad[0]]!r}")


@functools.lru_cache(maxsize=None)
def _layout_case(qtype, shape, x86):
    """The random weight set in the device layout, the row list, and the reference of those
    rows (dequant_np, held to the oracle above)."""
    name, raw = sc.weight_sets(qtype, *shape)[0]
    rows = sc.row_list(*shape, np.random.default_rng(shape[0]))
    ref = sc.dequant_np(qtype, raw.reshape(shape[0], -1)[rows].reshape(-1), len(rows), shape[1])
    return name, sc.repack_np(qtype, raw, *shape, x86), rows, ref


@pytest.mark.parametrize("x86", [0, 1], ids=["generic", "x86"])
@pytest.mark.parametrize("qtype", QTYPES, ids=IDS)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layout_model_inverts_the_repack(qtype, shape, x86):
    """k_repack_* followed by dequant_elem, both in NumPy, is ggml's dequantize: the model
    the mutants below are applied to is itself right."""
    _, P, rows, ref = _layout_case(qtype, shape, x86)
    got = sc.layout_get_rows(qtype, P, *shape, x86, rows)
    assert np.array_equal(bits(got), bits(ref))


def _layout_witnesses(mutant, types):
    seen = []
    for qtype in types:
        for shape in sc.SHAPES:
            for x86 in (0, 1):
                name, P, rows, ref = _layout_case(qtype, shape, x86)
                got = sc.layout_get_rows(qtype, P, *shape, x86, rows, mutant=mutant)
                wrong = np.flatnonzero((bits(got) != bits(ref)).any(axis=1))
                if wrong.size:
                    seen.append(f"{TNAME[qtype]}-{shape[0]}x{shape[1]}-{'x86' if x86 else 'generic'}-{name}-row{rows[wrong[0]]}")
    return seen


@pytest.mark.parametrize("mutant", sc.MUTANTS_LAYOUT)
def test_layout_mutants_are_seen(mutant):
    types = {"q6_no_xor": (Q6_K,), "q5_other_half": (Q5_K,)}.get(mutant, QTYPES)
    seen = _layout_witnesses(mutant, types)
    print(f"{mutant}: seen by {len(seen)} cases, first {seen[:3]}")
    assert seen, f"no case tells {mutant} from the right read"
    if mutant in ("order_swapped", "rgs_plus_one"):
        # every type sees them (Q8_0 has one byte order: only the K-quants see a swapped one)
        for q in (Q4_K, Q5_K, Q6_K) if mutant == "order_swapped" else QTYPES:
            assert any(s.startswith(TNAME[q] + "-") for s in seen), (mutant, TNAME[q])
    if mutant == "rgs_ignored":
        # seen at every shape whose rows are grouped, by every type
        for q in QTYPES:
            for shape in sc.SHAPES:
                if sc.layout_rgs(*shape):
                    assert any(s.startswith(f"{TNAME[q]}-{shape[0]}x{shape[1]}-") for s in seen), (TNAME[q], shape)


def test_row_lists_hold_the_group_edges():
    for shape in sc.SHAPES:
        V, RG = shape[0], 1 << sc.layout_rgs(*shape)
        rows = sc.row_list(*shape, np.random.default_rng(1))
        assert {0, 1, RG - 1, RG, RG + 1, V - 1} <= set(rows)
        assert set(range(V - RG - 1, V)) <= set(rows)
        assert {r % RG for r in rows} == set(range(RG))
        assert all(0 <= r < V for r in rows) and len(set(rows)) == len(rows)


# ---- token selection and state --------------------------------------------------------------
@pytest.mark.parametrize("vocab", [sc.SMALL[0], sc.WIDE[0]])
def test_state_cases_are_what_they_claim(vocab):
    cases = dict(sc.state_cases(vocab))
    hist = sc.init_hist(1, sc.N_CTX)[0]
    ref = {n: sc.entry_ref(st, hist, vocab, sc.N_CTX) for n, st in cases.items()}
    assert ref["host_token"][2] == 7 and ref["feedback"][2] == 9 and ref["feedback_odd"][2] == 13
    for k in range(64):
        assert ref[f"max_in_lane_{k}"][2] == (5 * k + 3) % vocab
    assert ref["top_bit"][2] == ref["top_bit_swapped"][2] == 3
    assert ref["hi_low_bit"][2] == ref["hi_low_bit_swapped"][2] == vocab - 1
    assert ref["equal_hi"][2] == ref["equal_hi_swapped"][2] == 5
    assert ref["id_zero"][2] == 0 and ref["id_last"][2] == vocab - 1
    assert ref["empty_keys"][2] == 0
    for n in cases:
        st, h, tok, pos = ref[n]
        assert 0 <= tok < vocab
        if n.startswith("clamp_"):
            assert tok == 0, n
        # the history changes at [pos] only, and only inside the context
        changed = np.flatnonzero(h != hist)
        assert list(changed) == ([pos] if 0 <= pos < sc.N_CTX else []), n
        assert not st["key"][pos & 1].any() and st["key"][(pos + 1) & 1].any() == (n != "empty_keys")
    assert int(ref["seq_wraps"][0]["seq"]) == 0 and int(ref["seq_zero"][0]["seq"]) == 1
    assert {int(st["pos_next"]) for st in cases.values()} >= {0, sc.N_CTX - 1, sc.N_CTX, sc.N_CTX + 5, -1}


@pytest.mark.parametrize("mutant", sc.MUTANTS_STATE)
def test_state_mutants_are_seen(mutant):
    for vocab in (sc.SMALL[0], sc.WIDE[0]):
        hist = sc.init_hist(1, sc.N_CTX)[0]
        seen = []
        for name, st in sc.state_cases(vocab):
            right, wrong = sc.entry_ref(st, hist, vocab, sc.N_CTX), sc.entry_ref(st, hist, vocab, sc.N_CTX, mutant=mutant)
            if right[2] != wrong[2] or right[0].tobytes() != wrong[0].tobytes() or not np.array_equal(right[1], wrong[1]):
                seen.append(name)
        print(f"{mutant}, vocabulary {vocab}: seen by {seen[:6]}")
        assert seen, f"no state case tells {mutant} from the contract"
        if mutant.startswith("skip_lane_"):
            assert f"max_in_lane_{mutant[10:]}" in seen


def test_prefill_token_cases():
    V = sc.SMALL[0]
    table = np.arange(V * 4, dtype=np.float32).reshape(V, 4)
    for name, tok, pos0, n_ctx in sc.pf_token_cases(V):
        hist = sc.init_hist(1, n_ctx)
        x, h = sc.pf_ref(table, tok, hist, pos0, n_ctx)
        T = len(tok)
        inside = ((tok >= 0) & (tok < V))
        assert np.array_equal(x[~inside], np.broadcast_to(table[0], (int((~inside).sum()), 4)))
        n = max(0, min(T, n_ctx - pos0))
        assert np.array_equal(h[0, pos0: pos0 + n], np.where(inside, tok, 0)[:n])
        assert np.array_equal(np.delete(h[0], np.arange(pos0, pos0 + n)), np.delete(hist[0], np.arange(pos0, pos0 + n)))
        if "crossing" in name and T > 1:
            assert 0 < n < T
        if T > 1:
            assert {-1, V, sc.I32_MAX, sc.I32_MIN} <= set(int(t) for t in tok)
    assert {len(t) for _, t, _, _ in sc.pf_token_cases(V)} == {1, 33, 600}
