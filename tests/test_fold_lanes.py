"""The narrow sweep's folded tree runs with nodes on lanes (fold_run, dd_kernels.hip).

A lane of a folded run holds one node of the run's last layer and the CB cut values of that node
in registers: one ancestor walk per node, wide LDS reads of the parent values and wide writes of
the results.  What that mapping can get wrong is lanes against widths -- the 64-lane pass boundary
and the clamp at the layer's last node, the NaN sentinel slot 127 next to a 127-wide layer,
partial batches (cuts >= nb must leave no summary), and the summary / walk-value stores when
several lanes share an ancestor.  The census below asserts, on the CPU reference's layer widths
alone, that the records fold runs of every width class and depth; the parity tests compare status,
bounds (bit for bit), children and argmax paths with the CPU reference.

Inputs and expected results come from the CPU reference (tests/test_gpu_parity.py and
tests/test_narrow_fold.py helpers), never from the engine.
"""
import collections

import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import pools
from tests import golden_io
from tests import test_narrow_fold as N
from tests import test_redo_refold as R
from tests.test_narrow_fold import last_batch_case  # noqa: F401  (fixture: c2_s3_dfs_big, 5 F + 13 O and 0 F + 4 O)

gpu = pytest.mark.gpu


def _provable_runs(tokens, us, cb):
    """(depth, width of the last layer) of the tree runs the narrow sweep folds in a DD whose layers
    have the node counts `tokens`: tests.test_narrow_fold._provable_run_depths' grouping rules (the
    way build_stream groups layers and sweep_narrow cuts runs, keeping to the runs whose ends the
    bounds on the merged layers' arc counts settle), with the last layer's width kept."""
    nn = [int(t.rstrip("m")) for t in tokens]
    merged = [t.endswith("m") for t in tokens]
    kg = next((k for k in range(len(nn)) if nn[k] > N.NARROW_MAX), len(nn))
    lo = [nn[k] + (max(2, nn[k - 1]) if merged[k] else 0) for k in range(len(nn))]
    hi = [nn[k] + (nn[k - 1] * us if merged[k] else 0) for k in range(len(nn))]
    found = collections.Counter()
    if any(hi[k] > N.TOPO_ENTRIES or (nn[k] == 1 and not merged[k]) for k in range(1, kg)):
        return found
    maxl = min(N.STAGE_LAYERS, max(1, N.STAGE_ENTRIES // (cb * us)))

    def runs(j, k1, known_end):
        while j < k1:
            if merged[j]:
                j += 1
                continue
            cap = j + N.MAX_RUN - 1
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
            found[(kb - j + 1, nn[kb])] += 1
            j = kb + 1
        return True

    k = 1
    while k < kg:
        k1, wlo, whi = k + 1, lo[k], hi[k]
        while k1 < kg and k1 - k < maxl:
            if whi + hi[k1] <= N.TOPO_ENTRIES:
                wlo, whi, k1 = wlo + lo[k1], whi + hi[k1], k1 + 1
            elif wlo + lo[k1] > N.TOPO_ENTRIES:
                break
            else:
                runs(k, k1, False)
                return found
        runs(k, k1, True)
        k = k1
    return found


def _width_class(n):
    return 0 if n <= 16 else 1 if n <= 64 else 2


def test_run_census_on_known_shapes():
    """The host-side census itself, on hand-made width lists (us = 3)."""
    shape = "1 2 3 6 9 12 48 1m 4 13 52 200".split()
    assert _provable_runs(shape, 3, 4) == {(5, 12): 1, (1, 48): 1, (3, 52): 1}
    # the depths agree with the census of tests/test_narrow_fold.py
    for cb in (4, 8):
        depths = collections.Counter()
        for (d, _), n in _provable_runs(shape, 3, cb).items():
            depths[d] += n
        assert depths == N._provable_run_depths(shape, 3, cb)
    # an even stretch folds as 3 + 1; a wide layer ends the narrow part
    assert _provable_runs("1 2 4 8 16 1m 300".split(), 3, 4) == {(3, 8): 1, (1, 16): 1}
    # widths on both sides of the 64-lane pass boundary and the widest narrow layer (stride 1: the
    # merged layers' arc counts are known); at stride 3 the arc count of the merged layer behind the
    # 127 nodes may or may not fit the ring slot, so the 127-wide run is not counted
    assert _provable_runs("1 64 1m 65 1m 127 1m 128".split(), 1, 4) == {(1, 64): 1, (1, 65): 1, (1, 127): 1}
    assert _provable_runs("1 64 1m 65 1m 127 1m 128".split(), 3, 4) == {(1, 64): 1, (1, 65): 1}


# configuration, seed: the root and 63 BFS records each, a 4 F + 12 O synthetic pool.  By the census:
# C3 seed 4 folds depth-5 runs that end on 64 nodes (CB 4) and depth-1 / depth-3 runs on 64 (CB 8),
# P1 seed 9 depth-1 runs on 65 and depth-5 runs on 126 nodes, P1 seed 3 depth-5 runs on 63 nodes at
# CB 4 and 8, C2 seed 1 the depth-3 runs of the 65-127 class.
CASES = {"c3": ("C3", 4), "p1": ("P1", 3), "p1w": ("P1", 9), "c2": ("C2", 1)}


@pytest.fixture(scope="module")
def bfs_cases(oracle_bin, tmp_path_factory):
    """The reference's results at DOUBLE_MIN and the 40th percentile of its bounds, and the records'
    layer widths, computed once per configuration."""
    return {key: N._synthetic_bfs_case(oracle_bin, tmp_path_factory.mktemp(key), cfg, seed) for key, (cfg, seed) in CASES.items()}


def _stride(case):
    e = E.Engine(case["net"], 0, 64)
    us = int(e.info.max_states)
    e.close()
    return us


@gpu
def test_width_census(bfs_cases):
    """On the reference's layer widths alone (the engine only tells the state-set stride of each
    network), at CB 4 and at CB 8: the records fold runs that end on <= 16, 17-64 and 65-127 nodes;
    runs of depth 1 and of depth 3 in each of the two upper classes; depth-5 runs (in every class
    at CB 4, in the upper two at CB 8, where only the P1 networks reach depth 5); a run that ends on
    exactly 64 and one on exactly 65 nodes."""
    strides = {key: _stride(case) for key, case in bfs_cases.items()}
    for cb in (4, 8):
        runs = collections.Counter()
        for key, case in bfs_cases.items():
            for tokens in case["widths"]:
                runs += _provable_runs(tokens, strides[key], cb)
        classes = collections.Counter()
        for (d, n), cnt in runs.items():
            classes[(d, _width_class(n))] += cnt
        print(f"runs[CB={cb}] (depth, class) = {dict(sorted(classes.items()))}")
        print(f"  depth 5 ends on {sorted(n for (d, n) in runs if d == 5)}")
        assert all(any(classes[(d, wc)] for d in (1, 3, 5)) for wc in (0, 1, 2)), classes
        assert all(classes[(d, wc)] > 0 for d in (1, 3) for wc in (1, 2)), classes
        assert all(classes[(5, wc)] > 0 for wc in ((0, 1, 2) if cb == 4 else (1, 2))), classes
        widths = {n for (_, n) in runs}
        assert 64 in widths and 65 in widths, sorted(widths)


@gpu
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("key", sorted(CASES))
def test_parity_over_the_width_classes(monkeypatch, bfs_cases, key, cb):
    """Status, bounds bit for bit, children and argmax paths at DOUBLE_MIN and the 40th percentile
    of the reference's bounds."""
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", "0")
    case = bfs_cases[key]
    e = E.Engine(case["net"], 0, 64)
    e.add_cuts(case["pool"])
    for inc, want in case["want"]:
        got = e.relax(case["recs"], inc)
        bad = golden_io.compare_results(got, want)
        assert not bad, f"{key} CB={cb} incumbent {inc!r}: " + "\n".join(bad[:10])
        assert N._bound_bits(got) == N._bound_bits(want)
    e.close()


@gpu
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("which", ["pool", "small"])
def test_partial_batches(monkeypatch, last_batch_case, which, cb):  # noqa: F811
    """The 133 DFS records of c2_s3_dfs_big under 5 F + 13 O (last batch nb = 1 at CB 4, 5 at CB 8)
    and under 0 F + 4 O, at DOUBLE_MIN and the 40th percentile of the reference's bounds.  The
    reference's results hold records that end non-exact with children and exact with a path, so
    the walk values and the width-1 summaries of the partial batch are read back."""
    want0 = last_batch_case[which + "_want"][0][1]
    assert sum(1 for g in want0 if not g.exact and g.children) >= 4
    assert sum(1 for g in want0 if g.exact and g.path) >= 4
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", "0")
    e = E.Engine(last_batch_case["net"], 0, 256)
    e.add_cuts(last_batch_case[which])
    for inc, want in last_batch_case[which + "_want"][:2]:
        got = e.relax(last_batch_case["recs"], inc)
        bad = golden_io.compare_results(got, want)
        assert not bad, f"{which} CB={cb} incumbent {inc!r}: " + "\n".join(bad[:10])
        assert N._bound_bits(got) == N._bound_bits(want)
    e.close()


@pytest.fixture(scope="module")
def redo_case(oracle_bin, tmp_path_factory):
    """The workload of tests/test_redo_refold.py's c2_case (C2 seed 1, 4 F + 12 O)."""
    return R._frontier_case(oracle_bin, tmp_path_factory.mktemp("redo"), "C2", 1, 4, 12)


@gpu
@pytest.mark.parametrize("cb", ["4", "8"])
def test_single_cut_sweeps(monkeypatch, redo_case, cb):
    """SGUFP_REDO_SWEEP=1: every exact redo sweeps its cut alone -- the narrow sweep with nb = 1
    and a write mask -- at every incumbent of the fixture; the engine's redo counts show that
    redos were taken."""
    monkeypatch.setenv("SGUFP_CUT_BATCH", cb)
    monkeypatch.setenv("SGUFP_SCREEN", "0")
    monkeypatch.setenv("SGUFP_REDO_SWEEP", "1")
    e = E.Engine(redo_case["net"], 0, 64)
    e.add_cuts(redo_case["pool"])
    redos = 0
    for inc, want in redo_case["want"]:
        got = e.relax(redo_case["recs"], inc)
        bad = golden_io.compare_results(got, want)
        assert not bad, f"CB={cb} incumbent {inc!r}: " + "\n".join(bad[:10])
        assert N._bound_bits(got) == N._bound_bits(want)
        redos += int((e.debug()[1].astype("int64") & 0xFF).sum())
    e.close()
    print(f"single-cut redo sweeps[CB={cb}] = {redos}")
    assert redos > 0
