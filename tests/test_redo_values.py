"""Exact redos that prune from the batch sweep's own values (redo_cut, dd_kernels.hip).

When the width-1 pruning of a batch cut fires and the DD has not been edited since the batch
sweep, the pruning reads that cut's state2 from what the sweep already computed (the width-1
summaries, the wide layers in s2b, the narrow layers kept in s2n) instead of sweeping the cut
again.  SGUFP_REDO_SWEEP=1 forces the sweep everywhere.  Expected results are the golden
files or the CPU reference / oracle, never the code under test; the two paths must also agree
in the `sweeps` and `redo` counters, and every class must actually take redos.

The redo counts in the docstrings below were seen on the GPU, summed over the records and
the runs of the test; the sweep path of the commit before this change gives the same.
"""
import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import frontier, instance, pools
from tests import golden_io
from tests import test_gpu_parity as P

pytestmark = pytest.mark.gpu

FIXTURES = ["c2_s2_dfs", "c2_s3_dfs_big", "c3_s1_dfs", "c1_s2_dfs", "c2_s4_opt_only", "c2_s5_feas_only"]


def _counters(e):
    """(sweeps, redo) per record of the engine's last batch."""
    return e.stats()[3].copy(), (e.debug()[1].astype(np.int64) & 0xFF)


def _engine(monkeypatch, net, pool, slots, cb, screen, sweep):
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    if sweep:
        monkeypatch.setenv("SGUFP_REDO_SWEEP", "1")
    else:
        monkeypatch.delenv("SGUFP_REDO_SWEEP", raising=False)
    e = E.Engine(net, 0, slots)
    e.add_cuts(pool)
    return e


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_match_golden_on_both_paths(monkeypatch, name):
    """A/B against the forced sweep path on the fixtures at their finite-incumbent runs (the
    feasibility-only fixture has none: its DOUBLE_MIN run), CB 4 / 8 / 16, screen 0 / 4: both
    paths give the golden results and the same sweeps / redo counters.
    Redos per fixture, summed over CB and screen values: c2_s2_dfs 36, c2_s3_dfs_big 78,
    c3_s1_dfs 69, c1_s2_dfs 57, c2_s4_opt_only 33, c2_s5_feas_only 6."""
    d = golden_io.case_dir(name)
    net = f"{d}/net.txt"
    pool = pools.read_pool(golden_io.golden_file(d, "cuts.txt"))
    nodes = P.nodes_of(name)
    case = [c for c in golden_io.manifest() if c["name"] == name][0]
    runs = [r for r in case["runs"] if float.fromhex(r["incumbent"]) != pools.DOUBLE_MIN] or case["runs"]
    want = {r["file"]: golden_io.parse_results_text(golden_io.read_golden(name, r["file"])) for r in runs}
    total = 0
    for cb in ["4", "8", "16"]:
        for screen in ["0", "4"]:
            ctr = {}
            for sweep in [False, True]:
                e = _engine(monkeypatch, net, pool, 256, cb, screen, sweep)
                for r in runs:
                    got = e.relax(nodes, float.fromhex(r["incumbent"]))
                    bad = golden_io.compare_results(got, want[r["file"]])
                    assert not bad, f"CB={cb} screen={screen} sweep={sweep} {r['file']}: " + "\n".join(bad[:10])
                    ctr[(sweep, r["file"])] = _counters(e)
                e.close()
            for r in runs:
                (sw_a, rd_a), (sw_b, rd_b) = ctr[(False, r["file"])], ctr[(True, r["file"])]
                assert np.array_equal(sw_a, sw_b) and np.array_equal(rd_a, rd_b), f"CB={cb} screen={screen} {r['file']}"
                total += int(rd_a.sum())
    print(f"redo[{name}] = {total}")
    assert total > 0


@pytest.fixture(scope="module")
def c2_case(oracle_bin, tmp_path_factory):
    """C2 (seed 1), 4 F + 12 O synthetic pool, a BFS frontier of 64 records; the incumbents are
    the 40th and 80th percentile of the reference's DOUBLE_MIN bounds under the whole pool."""
    tmp = tmp_path_factory.mktemp("c2")
    inst = instance.generate(instance.CONFIGS["C2"], 1, scenarios=1)
    net = str(tmp / "net.txt")
    inst.write(net)
    pool = pools.synthetic_pool(inst, 4, 12, 1)
    e = E.Engine(net, 0, 64)
    recs = E.batch_to_records(frontier.bfs_frontier(e, 64))
    e.close()
    assert 0 < len(recs) <= 64
    nodes = str(tmp / "nodes.txt")
    pools.write_nodes(nodes, recs)
    cuts = str(tmp / "cuts.txt")
    pools.write_pool(cuts, pool)
    want0 = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    fin = [g.ub for g in want0 if g.status in (0, 3)]
    incs = [float(np.percentile(fin, 40)), float(np.percentile(fin, 80))]
    return {"net": net, "pool": pool, "recs": recs, "nodes": nodes, "incs": incs, "oracle": oracle_bin}


def _applied_o(pool):
    """List positions of the optimality cuts in the order they are applied (newest first)."""
    return [i for i, c in enumerate(pool) if c.type == 0][::-1]


def _c2_run(monkeypatch, tmp_path, case, pool):
    """Both paths at CB 4 and 8 against the CPU reference at both incumbents; the redo sum."""
    cuts = str(tmp_path / "cuts.txt")
    pools.write_pool(cuts, pool)
    want = [(inc, P._cpu_relax(case["oracle"], tmp_path, case["net"], cuts, case["nodes"], inc)) for inc in case["incs"]]
    total = 0
    for cb in ["4", "8"]:
        ctr = {}
        for sweep in [False, True]:
            e = _engine(monkeypatch, case["net"], pool, 64, cb, "0", sweep)
            for inc, w in want:
                bad = golden_io.compare_results(e.relax(case["recs"], inc), w)
                assert not bad, f"CB={cb} sweep={sweep} incumbent {inc!r}: " + "\n".join(bad[:10])
                ctr[(sweep, inc)] = _counters(e)
            e.close()
        for inc, _ in want:
            (sw_a, rd_a), (sw_b, rd_b) = ctr[(False, inc)], ctr[(True, inc)]
            assert np.array_equal(sw_a, sw_b) and np.array_equal(rd_a, rd_b), f"CB={cb} incumbent {inc!r}"
            total += int(rd_a.sum())
    return total


def test_every_batch_position(monkeypatch, tmp_path, c2_case):
    """The first j = 0..3 applied optimality cuts dropped: every cut of the pool takes every
    position of a batch of four.  Redos for j = 0..3: 670 each (the first three applied cuts
    fire nowhere: the lengths 1..3 below take no redo)."""
    applied = _applied_o(c2_case["pool"])
    redos = []
    for j in range(4):
        drop = set(applied[:j])
        pool = [c for i, c in enumerate(c2_case["pool"]) if i not in drop]
        sub = tmp_path / f"j{j}"
        sub.mkdir()
        redos.append(_c2_run(monkeypatch, sub, c2_case, pool))
    print(f"redo[j=0..3] = {redos}")
    assert sum(1 for r in redos if r > 0) >= 2, redos


@pytest.mark.parametrize("lengths", [(1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12)])
def test_firing_cut_is_the_pools_last(monkeypatch, tmp_path, c2_case, lengths):
    """The optimality list cut off after each length 1..12, so that a firing cut is the last
    of the pool (no later batch rewrites what the redo left).  Redos per length 1..12: 0, 0, 0, 6,
    260, 452, 452, 610, 610, 622, 654, 670."""
    applied = _applied_o(c2_case["pool"])
    redos = []
    for n in lengths:
        drop = set(applied[n:])
        pool = [c for i, c in enumerate(c2_case["pool"]) if i not in drop]
        sub = tmp_path / f"n{n}"
        sub.mkdir()
        redos.append(_c2_run(monkeypatch, sub, c2_case, pool))
    print(f"redo[len={lengths}] = {redos}")
    assert sum(redos) > 0


def test_short_dds_parent_layer_in_hbm_and_lds(oracle_bin, tmp_path, monkeypatch):
    """The M1 seed-3 short DDs of test_short_dds_match_oracle (wide layers, a narrow parent
    under a wide leaf layer: the layer above a firing layer is in s2b or in s2n) at the 40th
    percentile, CB 4 and 8, against the oracle.  Redos: 144."""
    inst = instance.generate(instance.CONFIGS["M1"], 3, scenarios=1)
    net, cuts = str(tmp_path / "net.txt"), str(tmp_path / "cuts.txt")
    inst.write(net)
    pool = pools.synthetic_pool(inst, 4, 12, 3)
    pools.write_pool(cuts, pool)
    levels = [[pools.NodeRecord(0, pools.DOUBLE_MIN, pools.DOUBLE_MAX, [], [])]]
    while True:
        kids = [c for g in P._oracle_relax(oracle_bin, tmp_path, net, cuts, levels[-1], pools.DOUBLE_MIN) for c in g.children]
        if not kids:
            break
        levels.append(kids[::max(1, len(kids) // 64)][:64])
    recs = levels[-2][::2] + levels[-1][::2]
    assert 0 < len(recs) <= 64
    want0 = P._oracle_relax(oracle_bin, tmp_path, net, cuts, recs, pools.DOUBLE_MIN)
    pct40 = float(np.percentile([g.ub for g in want0 if g.status in (0, 3)], 40))
    want = P._oracle_relax(oracle_bin, tmp_path, net, cuts, recs, pct40)
    total = 0
    for cb in ["4", "8"]:
        ctr = []
        for sweep in [False, True]:
            e = _engine(monkeypatch, net, pool, 64, cb, "0", sweep)
            bad = golden_io.compare_results(e.relax(recs, pct40), want)
            assert not bad, f"CB={cb} sweep={sweep}: " + "\n".join(bad[:10])
            ctr.append(_counters(e))
            e.close()
        assert np.array_equal(ctr[0][0], ctr[1][0]) and np.array_equal(ctr[0][1], ctr[1][1]), f"CB={cb}"
        total += int(ctr[0][1].sum())
    print(f"redo[M1] = {total}")
    assert total > 0
