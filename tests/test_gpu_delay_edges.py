"""The hand-scheduled DELAY loop (csrc/mcs_delay_asm.hip) on its structural edges: the workloads of
tests/delay_edges.py, each proven on the CPU to reach its edge and to be computed alike by the oracle, a
plain per-second reference and hand-worked cases (tests/test_delay_edges_cpu.py).  Bit-exact against the
oracle, and with the exact hand-over and escalation counts: the engine re-runs a cluster the loop stops, so
a runaway guard or an early bail-out shows in mcs_stats.handed_over alone.  Run on a real MI355X."""
import json
import os

import numpy as np
import pytest

import delay_edges as E
from kat_util import GOLDEN
from mcs_amd import Engine
from test_gpu_delay import assert_delay_parity, handed_expected, run

pytestmark = pytest.mark.gpu
DKATS = json.load(open(os.path.join(GOLDEN, "kats_delay.json")))["delay"]
ASM = "mcs::delay_asm_kernel"
CS_FIELDS = ("t_end", "placed", "waited", "peak_running", "flags")


def launch(cases, max_wait_s=10, escalations=0, asm=True):
    """One launch of the cases in a fresh engine, checked against the oracle; returns the outputs."""
    arrays, streams = E.pack(cases)
    with Engine(0, policy="DELAY", max_wait_s=max_wait_s) as eng:
        node, start, fin, st, cs, ds = run(eng, arrays, streams)
        kernel = eng.last_kernel
    od = assert_delay_parity(arrays, streams, node, start, fin, cs, ds, max_wait_s=max_wait_s)
    if asm:
        handed = handed_expected(od)
        assert st.handed_over == handed, f"{st.handed_over} clusters handed over, Level1 outgrows LDS in {handed}"
        assert kernel == (ASM if handed == 0 else
                          f"{ASM} + mcs::delay_kernel ({handed} of {len(cases)} clusters handed over)")
    else:
        assert kernel == "mcs::delay_kernel" and st.handed_over == 0
    assert st.escalations == escalations
    # a cluster that was re-run counts once
    assert st.placed + st.unplaced == streams.n_jobs
    assert st.placed == int(od["placed"].sum()) and st.waited == int(od["moved_l1"].sum())
    assert st.unplaced == streams.n_jobs - int(od["placed"].sum())
    assert st.deadlocked == int((od["flags"] & 1).sum())
    return node, start, fin, cs, ds, streams


def assert_same_outputs(a, b):
    for i in range(3):
        np.testing.assert_array_equal(a[i], b[i])
    for f in CS_FIELDS:
        np.testing.assert_array_equal(a[3][f], b[3][f], err_msg=f)
    for f in a[4].dtype.names:
        np.testing.assert_array_equal(a[4][f], b[4][f], err_msg=f)


@pytest.mark.parametrize("fam,diag", [("capacity", "0"), ("rows", "0"), ("rows", "1"), ("g", "0"), ("g", "1"),
                                      ("modes", "0"), ("wide", "0"), ("pool", "0"), ("mixed", "0")])
def test_gpu_delay_edge_family(fam, diag, monkeypatch):
    """Every family in the loop (MCS_FIFO_DIAG=1: its counting build) and, in a fresh engine with
    MCS_DELAY_ASM=0, in the compiled delay_kernel: the oracle's outputs from both.  The pool cluster
    (700 running jobs against 512 slots) escalates once; only capacity_K641 is handed over."""
    cases = E.FAMILIES[fam]()
    esc = 1 if fam in ("pool", "mixed") else 0
    monkeypatch.setenv("MCS_FIFO_DIAG", diag)
    got = launch(cases, escalations=esc)
    if diag == "1":
        assert (got[3]["release_scans"] > 0).any()
        return
    monkeypatch.setenv("MCS_DELAY_ASM", "0")
    assert_same_outputs(got, launch(cases, escalations=esc, asm=False))


@pytest.mark.parametrize("mw", [1, 1000])
def test_gpu_delay_edge_rows_max_wait(mw):
    launch(E.rows_family(mw), max_wait_s=mw)


def test_gpu_delay_edge_mixed_equals_single_launches():
    """A quiet cluster, one handed over, one that escalates, a deadlocked, an empty and a 1-node cluster in
    one launch give what each gives alone (the re-runs touch their own clusters only)."""
    cases = E.mixed_family()
    node, start, fin, cs, ds, streams = launch(cases, escalations=1)
    for k, c in enumerate(cases):
        if len(c.free_c) < 129:  # (alone it is no cluster of the loop's shape)
            continue
        one = launch([c], escalations=int(c.name == "pool"))
        js = streams.of(k)
        for x, y in zip((node[js], start[js], fin[js]), one[:3]):
            np.testing.assert_array_equal(x, y, err_msg=c.name)
        for f in CS_FIELDS:
            assert cs[f][k] == one[3][f][0], (c.name, f)
        for f in ds.dtype.names:
            assert ds[f][k] == one[4][f][0], (c.name, f)


@pytest.mark.parametrize("k", DKATS, ids=[k["name"] for k in DKATS])
def test_gpu_delay_edge_embedded_kats(k):
    """The hand-derived DKATs, padded to 256 nodes so that the hand-scheduled loop runs them: their
    golden expectations, node indices shifted by the padding ahead of the real nodes."""
    emb = E.embedded_kats([k])
    node, start, fin, cs, ds, streams = launch([e[0] for e in emb])
    for i, (c, en, es, ef) in enumerate(emb):
        js = streams.of(i)
        np.testing.assert_array_equal(node[js], en, err_msg=c.name)
        np.testing.assert_array_equal(start[js], es, err_msg=c.name)
        np.testing.assert_array_equal(fin[js], ef, err_msg=c.name)
        for key, v in k["stats"].items():
            got = ds[key][i] if key in ds.dtype.names else cs[key][i]
            assert got == v, (c.name, key)
