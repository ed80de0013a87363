"""Exact redos that fold the layer above a firing merged layer again (refold_parent, dd_kernels.hip).

When the width-1 pruning of a batch cut fires in a merged layer whose parent layer is narrow
and holds several alive nodes, the pruning needs that layer's values of the cut.  No summary
holds them, so the redo folds the few tree layers between the nearest width-1 summary and that
layer again, into LDS, and prunes from there.  Expected results are the CPU reference's
(tests/test_gpu_parity.py helpers), never the engine's.  That the path is taken is read from
the per-record refold counters (Engine.refold_stats, SGUFP_REFOLD_STATS=1: a side buffer, the
results are what they are without it).

The counts in the docstrings were seen on the GPU, summed over the records and the runs of a test.
"""
import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import frontier, instance, pools
from tests import golden_io
from tests import test_gpu_parity as P

pytestmark = pytest.mark.gpu


def _engine(monkeypatch, net, pool, slots, cb, screen):
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    monkeypatch.setenv("SGUFP_REFOLD_STATS", "1")
    monkeypatch.delenv("SGUFP_REDO_SWEEP", raising=False)
    e = E.Engine(net, 0, slots)
    e.add_cuts(pool)
    return e


def _frontier_case(oracle_bin, tmp, cfg, seed, nf, no):
    """`cfg` (seed), a BFS frontier of 64 records, an nf F + no O synthetic pool; the incumbents
    are the 40th and 80th percentile of the reference's DOUBLE_MIN bounds under the whole pool.
    The reference's results at DOUBLE_MIN and at both incumbents are computed once."""
    inst = instance.generate(instance.CONFIGS[cfg], seed, scenarios=1)
    net = str(tmp / "net.txt")
    inst.write(net)
    pool = pools.synthetic_pool(inst, nf, no, seed)
    e = E.Engine(net, 0, 64)
    recs = E.batch_to_records(frontier.bfs_frontier(e, 64))
    e.close()
    assert 0 < len(recs) <= 64
    nodes, cuts = str(tmp / "nodes.txt"), str(tmp / "cuts.txt")
    pools.write_nodes(nodes, recs)
    pools.write_pool(cuts, pool)
    want0 = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    fin = [g.ub for g in want0 if g.status in (0, 3)]
    incs = [float(np.percentile(fin, 40)), float(np.percentile(fin, 80))]
    want = [(pools.DOUBLE_MIN, want0)] + [(inc, P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, inc)) for inc in incs]
    return {"net": net, "pool": pool, "recs": recs, "want": want}


@pytest.fixture(scope="module")
def c2_case(oracle_bin, tmp_path_factory):
    """The workload of c2_case in tests/test_redo_values.py (C2 seed 1, 4 F + 12 O)."""
    return _frontier_case(oracle_bin, tmp_path_factory.mktemp("c2"), "C2", 1, 4, 12)


def _run(monkeypatch, case, cb, screen, finite_only=True):
    """The case's runs against the reference; the refold counters summed over the runs, [16]."""
    e = _engine(monkeypatch, case["net"], case["pool"], 64, cb, screen)
    total = np.zeros(16, dtype=np.int64)
    deepest = most = 0
    for inc, w in case["want"]:
        if finite_only and inc == pools.DOUBLE_MIN:
            continue
        bad = golden_io.compare_results(e.relax(case["recs"], inc), w)
        assert not bad, f"CB={cb} screen={screen} incumbent {inc!r}: " + "\n".join(bad[:10])
        r = e.refold_stats().astype(np.int64)
        total += r.sum(0)
        deepest, most = max(deepest, int(r[:, 2].max())), max(most, int(r[:, 3].max()))
    e.close()
    total[2], total[3] = deepest, most
    return total


def test_refold_is_taken_and_deep(monkeypatch, c2_case):
    """CB 4 and 8, screen 0, both incumbents, against the reference.  Every record refolds; each
    refold spans 3 to 7 tree layers there, and one redo refolds for up to 20 firing merged layers.
    Per CB value: 4013 refolds over 15073 layers in 335 redos."""
    for cb in ["4", "8"]:
        t = _run(monkeypatch, c2_case, cb, "0")
        print(f"refold[C2 CB={cb}] = {t.tolist()}")
        assert t[0] > 0 and t[1] >= t[0], t          # some record refolded at least one layer
        assert t[2] >= 2 and t[8:].sum() > 0, t      # a refold of two or more tree layers
        assert t[3] >= 2, t                          # several firing merged layers in one redo
        assert t[6:].sum() == t[0] and t[5] > 0, t


def test_no_stale_lds_after_the_screen(monkeypatch, c2_case):
    """The same workload at CB 4 with four screened cuts: the screen's sweeps use the LDS value
    buffers the refold writes, just before the loop.  1702 refolds in 150 redos."""
    t = _run(monkeypatch, c2_case, "4", "4")
    print(f"refold[C2 CB=4 screen=4] = {t.tolist()}")
    assert t[0] > 0 and t[2] >= 2, t


def test_feasibility_batch_redo_refolds(monkeypatch):
    """A redo inside a feasibility batch (layers from 1, threshold -0.01) that refolds: the
    fixture c3_s4_dfs, every run, CB 4 and 8, against the golden files.  Refolds in feasibility
    batches: 1 in each of the two runs (3 tree layers), at CB 4 and at CB 8."""
    name = "c3_s4_dfs"
    d = golden_io.case_dir(name)
    pool = pools.read_pool(golden_io.golden_file(d, "cuts.txt"))
    nodes = P.nodes_of(name)
    case = [c for c in golden_io.manifest() if c["name"] == name][0]
    feas = []
    for cb in ["4", "8"]:
        e = _engine(monkeypatch, f"{d}/net.txt", pool, 256, cb, "0")
        n = 0
        for r in case["runs"]:
            got = e.relax(nodes, float.fromhex(r["incumbent"]))
            want = golden_io.parse_results_text(golden_io.read_golden(name, r["file"]))
            bad = golden_io.compare_results(got, want)
            assert not bad, f"CB={cb} {r['file']}: " + "\n".join(bad[:10])
            n += int(e.refold_stats()[:, 4].sum())
        e.close()
        feas.append(n)
    print(f"feasibility refolds[CB 4, 8] = {feas}")
    assert feas[0] > 0, feas


def test_counters_need_the_switch(monkeypatch):
    """Without SGUFP_REFOLD_STATS the engine keeps no counters and says so."""
    monkeypatch.delenv("SGUFP_REFOLD_STATS", raising=False)
    name = "c2_s2_dfs"
    d = golden_io.case_dir(name)
    e = E.Engine(f"{d}/net.txt", 0, 256)
    e.add_cuts(pools.read_pool(golden_io.golden_file(d, "cuts.txt")))
    e.relax(P.nodes_of(name), 0.0)
    with pytest.raises(RuntimeError):
        e.refold_stats()
    e.close()
