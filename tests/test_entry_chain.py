"""tools/entry_chain.py on a hand-written listing (tests/golden/entry_chain.s): the scalar
waits ahead of the first vector load, the vmcnt waits among the loads, and the kernarg
preload length, per kernel (no GPU)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LISTING = os.path.join(ROOT, "tests", "golden", "entry_chain.s")


def _by_name():
    import entry_chain as ec

    return {name: ec.entry_chain(body) for name, body in ec.kernels(open(LISTING).read())}


def test_kernels_only():
    assert sorted(_by_name()) == ["_Z6k_plainPKfPfi", "_Z9k_preloadPKfPfi"]  # not the device function


def test_plain_kernel_counts():
    swaits, vmwaits, lead, loads, preload = _by_name()["_Z6k_plainPKfPfi"]
    # lgkmcnt waits with an s_load outstanding: the second of two back-to-back waits has none;
    # the combined vmcnt(0) lgkmcnt(0) line ahead of the first load counts
    assert swaits == 3
    # vmcnt(1) stands between loads; vmcnt(2) and vmcnt(0) follow the last one
    assert vmwaits == 1
    assert (lead, loads) == (2, 4)  # global and buffer loads, not the store
    assert preload == 0


def test_preloaded_kernel_counts():
    swaits, vmwaits, lead, loads, preload = _by_name()["_Z9k_preloadPKfPfi"]
    assert swaits == 0   # the preamble's loads and wait lie ahead of .p2align: not the wave's path
    assert vmwaits == 0  # the lgkmcnt wait among the loads is not a vector-memory wait
    assert (lead, loads) == (3, 3)
    assert preload == 5


def test_command_line_filters_by_name():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "entry_chain.py"), LISTING, "k_preload"],
                         check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(out) == 1 and "k_preload" in out[0]
    assert out[0].split()[-10:] == ["swaits", "0", "vmwaits", "0", "lead", "3", "loads", "3", "preload", "5"]
