"""The step-entry hook's C surface without a GPU: llmi_step_entry is exported and every bad
argument is refused before any device call (the device pointer is never dereferenced); and
llmi_device_layout_bytes / llmi_repack refuse a matrix whose quant plane reaches 4 GiB, the
range of the kernels' 32-bit piece offsets."""
from __future__ import annotations

import ctypes as C

import pytest

import llmi
from helpers import Q4_K, Q5_K, Q6_K, Q8_0
from llmi._lib import llmi_step_entry_args, llmi_step_state

DEV = 0x1000  # a non-null "device pointer": no valid call gets as far as using it


def make(kernel=0, **over):
    a = llmi_step_entry_args()
    a.kernel, a.type, a.w_dev, a.vocab, a.cols, a.n_ctx, a.pos0 = kernel, Q4_K, DEV, 64, 256, 32, 0
    a.nt = {0: 1, 1: 3, 2: 5, 3: 1}.get(kernel, 1)
    a.n_seq = 8 if kernel == 1 else 1
    keep = dict(tseq=(C.c_int32 * 8)(5, 2, 7, 0, 1, 3, 4, 6), tokens=(C.c_int32 * 8)(), states=(llmi_step_state * 8)(),
                hist=(C.c_int32 * (8 * 32))(), tpos=(C.c_int32 * 8)(), x_out=(C.c_uint32 * (8 * 256))(),
                guard_bad=(C.c_int32 * 3)())
    for k, v in keep.items():
        setattr(a, k, C.cast(v, type(getattr(a, k))) if k == "states" else v)
    for k, v in over.items():
        if k == "tseq_values":
            for i, t in enumerate(v):
                keep["tseq"][i] = t
        else:
            setattr(a, k, v)
    return a, keep


def refused(a):
    rc = llmi.lib().llmi_step_entry(C.byref(a[0]))
    return rc == -1 and "llmi_step_entry" in llmi.last_error()


def test_symbol_is_exported():
    assert hasattr(llmi.lib(), "llmi_step_entry")
    assert llmi.lib().llmi_step_entry(None) < 0


def test_state_record_matches_the_c_struct():
    assert llmi.STEP_STATE.itemsize == C.sizeof(llmi_step_state) == 6 * 4 + 2 * 64 * 8
    assert llmi.STEP_STATE.fields["key"][1] == llmi_step_state.key.offset


_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())  # noqa: E731
COMMON_BAD = [dict(type=2), dict(type=-1), dict(type=15), dict(type=0), dict(w_dev=None), dict(cols=0), dict(cols=300),
              dict(cols=-256), dict(cols=2 ** 31 + 256), dict(vocab=0), dict(vocab=-4), dict(vocab=2 ** 31), dict(n_ctx=0),
              dict(n_ctx=-1), dict(n_ctx=2 ** 20 + 1), dict(x_out=None), dict(guard_bad=None)]


@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("bad", COMMON_BAD, ids=_ids)
def test_rejects_bad_common_arguments(kernel, bad):
    assert refused(make(kernel, **bad)), bad


@pytest.mark.parametrize("kernel", [-1, 4, 100])
def test_rejects_unknown_kernels(kernel):
    assert refused(make(kernel))


@pytest.mark.parametrize("kernel,nt", [(0, 0), (0, 2), (3, 0), (3, 2), (1, 0), (1, 9), (1, -1), (2, 0), (2, -3), (2, 65536)])
def test_token_counts_per_kernel(kernel, nt):
    assert refused(make(kernel, nt=nt))


@pytest.mark.parametrize("kernel,n_seq", [(0, 0), (0, 2), (2, 2), (3, 8), (1, 2), (1, 0), (1, 65)])
def test_sequence_counts_per_kernel(kernel, n_seq):
    assert refused(make(kernel, n_seq=n_seq)), (kernel, n_seq)  # (kernel 1: nt = 3 slots need 3..64 states)


@pytest.mark.parametrize("tseq", [(5, 2, 5), (0, 0, 1), (5, 2, 8), (-1, 2, 3), (1, 2, 2 ** 31 - 1)], ids=str)
def test_rejects_duplicate_and_out_of_range_tseq(tseq):
    assert refused(make(1, tseq_values=tseq))


def test_rejects_null_pointers_per_kernel():
    for kernel, fields in ((0, ("states", "hist")), (1, ("states", "hist", "tseq", "tpos")), (2, ("tokens", "hist")),
                           (3, ("states",))):
        for f in fields:
            assert refused(make(kernel, **{f: None})), (kernel, f)


@pytest.mark.parametrize("pos0", [-1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 5])
def test_prefill_pos0_must_not_be_negative_or_overflow(pos0):
    assert refused(make(2, pos0=pos0))


# rows x cols whose A plane (128 B per K-quant block, 32 B per Q8_0 block) ends exactly at
# 4 GiB, and the largest row count below it
PLANE_EDGES = [(Q4_K, 2 ** 17, 65536), (Q5_K, 2 ** 21, 4096), (Q6_K, 2 ** 25, 256), (Q8_0, 2 ** 20, 4096),
               (Q8_0, 2 ** 16, 65536)]


@pytest.mark.parametrize("qtype,rows,cols", PLANE_EDGES)
def test_layout_hooks_refuse_a_quant_plane_of_4_gib(qtype, rows, cols):
    L = llmi.lib()
    per_row = cols // 256 * 128 if qtype != Q8_0 else cols
    assert rows * per_row == 2 ** 32
    for r in (rows, rows + 1, 4 * rows):
        assert L.llmi_device_layout_bytes(qtype, r, cols) == -1
        assert "4 GiB" in llmi.last_error() and "llmi_device_layout_bytes" in llmi.last_error()
        assert L.llmi_repack(qtype, DEV, DEV, r, cols) == -1  # refused on the host: DEV is never used
        assert "4 GiB" in llmi.last_error() and "llmi_repack" in llmi.last_error()
    # one row fewer fits: the bytes are the GGUF bytes plus plane alignment
    fit = L.llmi_device_layout_bytes(qtype, rows - 1, cols)
    gguf = (rows - 1) * (cols // {Q8_0: 32}.get(qtype, 256)) * {Q4_K: 144, Q5_K: 176, Q6_K: 210, Q8_0: 34}[qtype]
    assert gguf <= fit < gguf + 4 * 256
    a = make(2, type=qtype, vocab=rows, cols=cols)
    assert refused(a) and "4 GiB" in llmi.last_error()


def test_unquantized_layouts_have_no_plane_limit():
    assert llmi.lib().llmi_device_layout_bytes(0, 2 ** 20, 4096) == 2 ** 20 * 4096 * 4  # F32: no piece offsets
