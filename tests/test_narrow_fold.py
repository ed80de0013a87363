"""The narrow sweep's folded tree runs (fold_run, dd_kernels.hip) without the rank select.

Tree layers take the coefficient of rank 0 (the decision -1) from the staged ring as -0.0, so a
level of a run is `in ? x + coef : DMIN` with no `reg ? x + coef : x` select: x + -0.0 is x bit
for bit, both zeros included.  Merged layers keep the table's +0.0 (their width-1 summary is
parent + 0.0, and a zero maximum re-runs the layer with the exact pick).  These tests pin that on
pools whose values are zeros of both signs, check that the records fold runs of every depth, and
run pools whose last batch is partial (the store branch of fold_run feeds the path walks).

Inputs and expected results come from the CPU reference alone (the frontier is a BFS over the
reference's cutset children; tests/test_gpu_parity.py helpers), never from the engine.
"""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import instance, pools
from tests import golden_io
from tests import test_gpu_parity as P

gpu = pytest.mark.gpu


def _kernel_constant(name):
    """A `constexpr` integer of dd_kernels.hip, read from the source the library is built from."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sgufp_solver_amd", "csrc", "dd_kernels.hip")
    with open(src) as fh:
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(\d+)\s*;", fh.read())
    assert m, name
    return int(m.group(1))


# the narrow sweep's staging constants
STAGE_ENTRIES, TOPO_ENTRIES, STAGE_LAYERS, MAX_RUN, NARROW_MAX = (
    _kernel_constant(n) for n in ("kStageEntries", "kTopoEntries", "kStageLayers", "kMaxRun", "kNarrowMax"))


def _cpu_frontier(oracle_bin, tmp, net, cuts, n):
    """The first n records of a BFS over cutset children from the root record, relaxed at
    DOUBLE_MIN under the pool by the CPU reference (frontier.bfs_frontier's order)."""
    level = [pools.NodeRecord(0, pools.DOUBLE_MIN, pools.DOUBLE_MAX, [], [])]
    done = []
    while level and len(done) < n:
        nodes = str(tmp / "level.txt")
        pools.write_nodes(nodes, level)
        level = [c for g in P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN) for c in g.children]
        done += level[:n - len(done)]
    return done


def _zero_cut(inst, rhs):
    """An optimality cut whose coefficients are all explicit zeros."""
    return pools.PoolCut(0, rhs, [(i, q, j, 0.0) for (i, q, j) in pools.vbar_keys(inst)])


@pytest.fixture(scope="module")
def c2_zero_case(oracle_bin, tmp_path_factory):
    """C2 seed 1 with 64 BFS records under a 4 F + 12 O synthetic pool that also holds an all-zero
    optimality cut with right-hand side 0.0 (oldest: applied last) and one with -0.0 (newest:
    applied first).  The synthetic optimality cuts' right-hand sides are lowered by the median of
    the reference's bounds under the plain pool, so that the records' bounds lie on both sides of
    zero and the zero cuts bind in some records only.  The reference's results at DOUBLE_MIN and
    at the 40th / 80th percentile of its DOUBLE_MIN bounds are computed once."""
    tmp = tmp_path_factory.mktemp("c2zero")
    inst = instance.generate(instance.CONFIGS["C2"], 1, scenarios=1)
    net, cuts, nodes = str(tmp / "net.txt"), str(tmp / "cuts.txt"), str(tmp / "nodes.txt")
    inst.write(net)
    base = pools.synthetic_pool(inst, 4, 12, 1)
    pools.write_pool(cuts, base)
    recs = _cpu_frontier(oracle_bin, tmp, net, cuts, 64)
    assert 0 < len(recs) <= 64
    pools.write_nodes(nodes, recs)
    plain = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    mid = float(np.median([g.ub for g in plain if g.status in (0, 3)]))
    pool = ([_zero_cut(inst, 0.0)] + [pools.PoolCut(c.type, c.rhs - mid if c.type == 0 else c.rhs, c.coeff) for c in base] +
            [_zero_cut(inst, -0.0)])
    pools.write_pool(cuts, pool)
    want0 = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    fin = [g.ub for g in want0 if g.status in (0, 3)]
    incs = [float(np.percentile(fin, 40)), float(np.percentile(fin, 80))]
    want = [(pools.DOUBLE_MIN, want0)] + [(inc, P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, inc)) for inc in incs]
    widths = subprocess.run([oracle_bin, "widths", net, nodes], check=True, capture_output=True, text=True).stdout
    return {"net": net, "pool": pool, "recs": recs, "want": want, "widths": [ln.split() for ln in widths.splitlines()]}


def _bound_bits(results):
    """lb, ub and the children's bounds of every record as hex strings (the sign of a zero shows)."""
    return [(g.lb.hex(), g.ub.hex(), tuple((c.lb.hex(), c.ub.hex()) for c in g.children)) for g in results]


@gpu
@pytest.mark.parametrize("screen", ["0", "4"])
@pytest.mark.parametrize("cb", ["4", "8"])
def test_zero_maxima(monkeypatch, c2_zero_case, cb, screen):
    """Every incumbent against the reference, bounds by bit pattern.  Under the all-zero cuts every
    candidate of a merged layer is a zero, so every merged layer re-runs with the exact pick.  (No
    zero of these results carries a sign bit: test_negative_zero_through_tree_runs is the one that
    tells -0.0 from +0.0.)"""
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    e = E.Engine(c2_zero_case["net"], 0, 64)
    e.add_cuts(c2_zero_case["pool"])
    zeros = 0
    for inc, want in c2_zero_case["want"]:
        got = e.relax(c2_zero_case["recs"], inc)
        bad = golden_io.compare_results(got, want)
        assert not bad, f"CB={cb} screen={screen} incumbent {inc!r}: " + "\n".join(bad[:10])
        assert _bound_bits(got) == _bound_bits(want)
        zeros += sum(1 for g in want if g.ub == 0.0)
    e.close()
    # the zero cuts do bind, and records finish: on the reference's results alone
    assert zeros >= 8
    assert sum(1 for g in c2_zero_case["want"][0][1] if g.status in (0, 3)) >= 32
    assert sum(1 for g in c2_zero_case["want"][1][1] if g.status in (0, 3)) >= 8


def _provable_run_depths(tokens, us, cb):
    """Depths of the tree runs the narrow sweep folds in a DD whose layers (root to the one before
    the last) have the node counts `tokens` (dd_oracle widths: 'm' marks a merged layer), counted on
    the host the way build_stream groups layers and sweep_narrow cuts runs.  The width list does
    not give a merged layer's in-arc count, only bounds (one to `us` arcs per parent node: a state
    set holds at most `us` decisions, -1 included); the count keeps to the runs whose ends those
    bounds settle and stops at the first one they do not, so every run it returns is one the
    kernel folds."""
    nn = [int(t.rstrip("m")) for t in tokens]
    merged = [t.endswith("m") for t in tokens]
    kg = next((k for k in range(len(nn)) if nn[k] > NARROW_MAX), len(nn))
    lo = [nn[k] + (max(2, nn[k - 1]) if merged[k] else 0) for k in range(len(nn))]
    hi = [nn[k] + (nn[k - 1] * us if merged[k] else 0) for k in range(len(nn))]
    depths = collections.Counter()
    # a single layer above one ring slot sends the DD down the single-cut path; a width-1 layer
    # without the mark may be a merged layer of one arc
    if any(hi[k] > TOPO_ENTRIES or (nn[k] == 1 and not merged[k]) for k in range(1, kg)):
        return depths
    maxl = min(STAGE_LAYERS, max(1, STAGE_ENTRIES // (cb * us)))

    def runs(j, k1, known_end):
        """Runs of the group that starts at j and holds the layers below k1 -- all of it
        (known_end), or at least those.  False: a run's end depends on what is not known."""
        while j < k1:
            if merged[j]:
                j += 1
                continue
            cap = j + MAX_RUN - 1
            last = min(cap, k1 - 1 if known_end else min(k1, kg - 1))
            stop = next((t for t in range(j, last + 1) if merged[t]), None)
            if stop is not None:
                kb = stop - 1
            elif cap <= k1 - 1:
                kb = cap
            elif known_end:
                kb = k1 - 1
            else:
                return False
            kb -= (kb - j) & 1
            depths[kb - j + 1] += 1
            j = kb + 1
        return True

    k = 1
    while k < kg:
        k1, wlo, whi = k + 1, lo[k], hi[k]
        while k1 < kg and k1 - k < maxl:
            if whi + hi[k1] <= TOPO_ENTRIES:
                wlo, whi, k1 = wlo + lo[k1], whi + hi[k1], k1 + 1
            elif wlo + lo[k1] > TOPO_ENTRIES:
                break
            else:
                runs(k, k1, False)
                return depths
        runs(k, k1, True)
        k = k1
    return depths


def test_run_depth_census_on_known_shapes():
    """The host-side count itself, on hand-made width lists (us = 3, CB = 4: 10 layers per group)."""
    # root, six tree layers, a merged layer, three tree layers: one group -> runs 5, 1, then 3
    assert _provable_run_depths("1 2 3 6 9 12 48 1m 4 13 52 200".split(), 3, 4) == {5: 1, 1: 1, 3: 1}
    # CB = 8: 5 layers per group -> 5 | 1, (merged), 3
    assert _provable_run_depths("1 2 3 6 9 12 48 1m 4 13 52 200".split(), 3, 8) == {5: 1, 1: 1, 3: 1}
    # an even stretch folds as 3 + 1; a wide layer ends the narrow part
    assert _provable_run_depths("1 2 4 8 16 1m 300".split(), 3, 4) == {3: 1, 1: 1}
    # a merged layer whose arc count may or may not fit the ring slot: nothing after it is counted
    assert _provable_run_depths("1 100 120 1m 4".split(), 3, 4) == {1: 2}


def _synthetic_bfs_case(oracle_bin, tmp, cfg, seed):
    """`cfg` (seed), the root record and 63 BFS records, a 4 F + 12 O synthetic pool; the reference's results at
    DOUBLE_MIN and the 40th percentile of its bounds, and the records' layer widths."""
    inst = instance.generate(instance.CONFIGS[cfg], seed, scenarios=1)
    net, cuts, nodes = str(tmp / "net.txt"), str(tmp / "cuts.txt"), str(tmp / "nodes.txt")
    inst.write(net)
    pool = pools.synthetic_pool(inst, 4, 12, seed)
    pools.write_pool(cuts, pool)
    recs = [pools.NodeRecord(0, pools.DOUBLE_MIN, pools.DOUBLE_MAX, [], [])] + _cpu_frontier(oracle_bin, tmp, net, cuts, 63)
    assert 1 < len(recs) <= 64
    pools.write_nodes(nodes, recs)
    want0 = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    inc = float(np.percentile([g.ub for g in want0 if g.status in (0, 3)], 40))
    want = [(pools.DOUBLE_MIN, want0), (inc, P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, inc))]
    widths = subprocess.run([oracle_bin, "widths", net, nodes], check=True, capture_output=True, text=True).stdout
    return {"net": net, "pool": pool, "recs": recs, "want": want, "widths": [ln.split() for ln in widths.splitlines()]}


@pytest.fixture(scope="module")
def p1_case(oracle_bin, tmp_path_factory):
    """P1 seed 3: state sets of three decisions (stride 3), so a staging group holds 10 layers at
    CB 4 and 5 at CB 8, and the DDs open with six tree layers, a merged one and five more tree
    layers: runs of depth 5, 3 and 1 at both batch sizes.  (The networks of the C2 / C3 fixtures
    have strides 4 and 5: at CB 8 their groups hold 4 and 3 layers and no run reaches depth 5,
    c3_s4_dfs included.)"""
    return _synthetic_bfs_case(oracle_bin, tmp_path_factory.mktemp("p1"), "P1", 3)


def _depths_and_parity(monkeypatch, case, cb):
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", "0")
    e = E.Engine(case["net"], 0, 64)
    e.add_cuts(case["pool"])
    us = int(e.info.max_states)
    depths = collections.Counter()
    for tokens in case["widths"]:
        depths += _provable_run_depths(tokens, us, int(cb))
    for inc, want in case["want"][:2]:
        bad = golden_io.compare_results(e.relax(case["recs"], inc), want)
        assert not bad, f"CB={cb} incumbent {inc!r}: " + "\n".join(bad[:10])
    e.close()
    return us, depths


@gpu
@pytest.mark.parametrize("cb", ["4", "8"])
def test_tree_runs_of_every_depth(monkeypatch, p1_case, cb):
    """CB 4 and 8: the records fold runs of depth 1, 3 and 5 (host-side count over the reference's
    layer widths with the engine's state-set stride), and their results are the reference's."""
    us, depths = _depths_and_parity(monkeypatch, p1_case, cb)
    print(f"tree runs[P1 CB={cb} us={us}] = {dict(depths)}")
    assert depths[1] > 0 and depths[3] > 0 and depths[5] > 0, depths


@gpu
def test_tree_runs_of_every_depth_c2(monkeypatch, c2_zero_case):
    """The same on the C2 records at CB 4 (stride 4: 8 layers per group)."""
    us, depths = _depths_and_parity(monkeypatch, c2_zero_case, "4")
    print(f"tree runs[C2 CB=4 us={us}] = {dict(depths)}")
    assert depths[1] > 0 and depths[3] > 0 and depths[5] > 0, depths


# ---------------------------------------------------------------- a -0.0 through the tree runs
@pytest.fixture(scope="module")
def neg_zero_case(oracle_bin, tmp_path_factory):
    """C2 seed 1, the records whose decisions so far are all -1, at every third global layer: their root
    fold adds nothing, so under an all-zero optimality cut of right-hand side -0.0 the root value is
    -0.0 and stays -0.0 along rank-0 steps (a step of any other rank adds the table's +0.0 and
    gives +0.0).  The feasibility cuts of the synthetic pool come first."""
    tmp = tmp_path_factory.mktemp("negzero")
    inst = instance.generate(instance.CONFIGS["C2"], 1, scenarios=1)
    net, cuts, nodes = str(tmp / "net.txt"), str(tmp / "cuts.txt"), str(tmp / "nodes.txt")
    inst.write(net)
    pool = [c for c in pools.synthetic_pool(inst, 4, 12, 1) if c.type == 1] + [_zero_cut(inst, -0.0)]
    pools.write_pool(cuts, pool)
    root = [pools.NodeRecord(0, pools.DOUBLE_MIN, pools.DOUBLE_MAX, [], [])]
    pools.write_nodes(nodes, root)
    layers = len(subprocess.run([oracle_bin, "widths", net, nodes], check=True, capture_output=True, text=True).stdout.split()) + 1
    recs = [pools.NodeRecord(g, pools.DOUBLE_MIN, pools.DOUBLE_MAX, [], [-1] * g) for g in range(0, layers, 3)]
    pools.write_nodes(nodes, recs)
    want = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
    return {"net": net, "pool": pool, "recs": recs, "want": want}


def _neg_zero(x):
    return x == 0.0 and float(x).hex().startswith("-")


@gpu
@pytest.mark.parametrize("screen", ["0", "4"])
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("exact_fast", ["0", "1"])
def test_negative_zero_through_tree_runs(monkeypatch, neg_zero_case, exact_fast, cb, screen):
    """On the reference's results alone: enough records finish, and some bounds are -0.0.  Then the
    engine against them, by bit pattern.  The records whose bound is -0.0 are exact DDs; with
    SGUFP_EXACT_FAST=0 their optimality phase stays in k_relax's batch sweeps (the narrow sweep and
    its tree runs) and does not go to the cut-parallel kernels."""
    monkeypatch.setenv("SGUFP_EXACT_FAST", exact_fast)
    want = neg_zero_case["want"]
    assert sum(1 for g in want if g.status in (0, 3)) >= 16
    assert sum(1 for g in want if _neg_zero(g.ub)) >= 3
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    e = E.Engine(neg_zero_case["net"], 0, 128)
    e.add_cuts(neg_zero_case["pool"])
    got = e.relax(neg_zero_case["recs"], pools.DOUBLE_MIN)
    e.close()
    bad = golden_io.compare_results(got, want)
    assert not bad, f"CB={cb} screen={screen}: " + "\n".join(bad[:10])
    assert _bound_bits(got) == _bound_bits(want)


# ---------------------------------------------------------------- partial last batches, path walks
@pytest.fixture(scope="module")
def last_batch_case(oracle_bin, tmp_path_factory):
    """The network and the 133 DFS records of the fixture c2_s3_dfs_big under the first 5 F and
    the first 13 O cuts of its pool: the last O batch has nb = 1 at CB 4 and 5 at CB 8, the last F
    batch 1 and 5.  Incumbents: DOUBLE_MIN and the 40th / 80th percentile of the reference's
    bounds.  `small`: the first 4 O cuts alone -- one batch at CB 4 and 8, so every batch of a
    record, a restart after a redo included, is its last."""
    tmp = tmp_path_factory.mktemp("lastbatch")
    d = golden_io.case_dir("c2_s3_dfs_big")
    net, nodes = f"{d}/net.txt", f"{d}/nodes.txt"
    full = pools.read_pool(golden_io.golden_file(d, "cuts.txt"))
    feas, opt = [c for c in full if c.type == 1], [c for c in full if c.type == 0]
    out = {"net": net, "recs": pools.read_nodes(nodes)}
    for key, pool in (("pool", feas[:5] + opt[:13]), ("small", opt[:4])):
        cuts = str(tmp / f"{key}.txt")
        pools.write_pool(cuts, pool)
        want0 = P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, pools.DOUBLE_MIN)
        fin = [g.ub for g in want0 if g.status in (0, 3)]
        incs = [float(np.percentile(fin, 40)), float(np.percentile(fin, 80))]
        out[key] = pool
        out[key + "_want"] = [(pools.DOUBLE_MIN, want0)] + [(i, P._cpu_relax(oracle_bin, tmp, net, cuts, nodes, i)) for i in incs]
    return out


@gpu
@pytest.mark.parametrize("screen", ["0", "4"])
@pytest.mark.parametrize("cb", ["4", "8"])
def test_partial_last_batch_walks(monkeypatch, last_batch_case, cb, screen):
    """5 F + 13 O: argmax paths and cutset children (the path walks' outputs) with the rest of the
    results against the reference.  The reference's own results hold at least 4 records that end
    non-exact with children and at least 4 that end exact with a path."""
    want0 = last_batch_case["pool_want"][0][1]
    assert sum(1 for g in want0 if not g.exact and g.children) >= 4
    assert sum(1 for g in want0 if g.exact and g.path) >= 4
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    e = E.Engine(last_batch_case["net"], 0, 256)
    e.add_cuts(last_batch_case["pool"])
    for inc, want in last_batch_case["pool_want"]:
        bad = golden_io.compare_results(e.relax(last_batch_case["recs"], inc), want)
        assert not bad, f"CB={cb} screen={screen} incumbent {inc!r}: " + "\n".join(bad[:10])
    e.close()


@gpu
@pytest.mark.parametrize("cb", ["4", "8"])
def test_redo_in_the_last_batch(monkeypatch, last_batch_case, cb):
    """0 F + 4 O: the pool is one batch, so a record that took a redo (the engine's per-record
    redo count) took it in its last batch and restarted into another last batch; results against
    the reference at every incumbent."""
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", "0")
    e = E.Engine(last_batch_case["net"], 0, 256)
    e.add_cuts(last_batch_case["small"])
    redos = 0
    for inc, want in last_batch_case["small_want"]:
        got = e.relax(last_batch_case["recs"], inc)
        bad = golden_io.compare_results(got, want)
        assert not bad, f"CB={cb} incumbent {inc!r}: " + "\n".join(bad[:10])
        redo = e.debug()[1].astype(np.int64) & 0xFF
        redos += int(sum(1 for r, g in zip(redo, want) if r > 0 and g.status in (0, 3)))
    e.close()
    print(f"finishing records with a redo in the last batch[CB={cb}] = {redos}")
    assert redos > 0


@gpu
@pytest.mark.parametrize("screen", ["0", "4"])
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("name", ["c2_s4_opt_only", "c2_s5_feas_only"])
def test_single_phase_pools(monkeypatch, name, cb, screen):
    """A pool without F cuts and one whose last batch is a feasibility batch (12 F: nb = 4 at CB 8),
    every run of the fixture against the golden files."""
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", screen)
    d = golden_io.case_dir(name)
    e = E.Engine(f"{d}/net.txt", 0, 256)
    e.add_cuts(pools.read_pool(golden_io.golden_file(d, "cuts.txt")))
    case = [c for c in golden_io.manifest() if c["name"] == name][0]
    for run in case["runs"]:
        got = e.relax(P.nodes_of(name), float.fromhex(run["incumbent"]))
        want = golden_io.parse_results_text(golden_io.read_golden(name, run["file"]))
        bad = golden_io.compare_results(got, want)
        assert not bad, f"{name} CB={cb} screen={screen} {run['file']}: " + "\n".join(bad[:10])
    e.close()
