"""The split relaxation (launch_relax, k_relax<CB, head / chunk>, dd_kernels.hip): a batch runs as a
head launch (build, feasibility batches, screen) and chunk launches of Q pool positions on two
in-order chains, each record suspended between two batches with its loop state in the slot's
scratch and resumed by the next launch.

Every operation of a record and their order are those of the single launch, so an engine with the
split forced (SGUFP_RELAX_CHUNK=<Q>) must give, bit for bit, what an engine with SGUFP_RELAX_CHUNK=0
gives on the same upload: status, exact, lb, ub, child counts, sweeps, redo counts, DD sizes, the
children arrays, the argmax paths and the routes.  Where the CPU reference's results exist they are
compared too (tests/test_narrow_fold.py and tests/test_redo_refold.py helpers).

What can go wrong is state that does not survive the launch boundary -- the layer table after an
edit, the counters, the hand-off flag, the root solution's slots, the staging groups -- and
boundaries that fall where a batch restarted after a redo (the position then moves by less than
CB), so the shapes are: one batch per launch (Q = CB), two (Q = 8), partial last batches, an odd
record count (halves of 66 and 67), one record, no optimality cut, fewer than the screen takes.
"""
import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import pools
from tests import golden_io
from tests import test_narrow_fold as N
from tests import test_redo_refold as R
from tests.test_narrow_fold import last_batch_case  # noqa: F401  (fixture: c2_s3_dfs_big, 5 F + 13 O and 0 F + 4 O)

pytestmark = pytest.mark.gpu

FIELDS = ("status", "exact", "lb", "ub", "n_children", "dd_nodes", "dd_arcs", "dd_layers", "sweeps", "redo",
          "child_off", "child_gl", "child_lb", "child_ub", "child_states_off", "child_states", "child_sol_off",
          "child_sol", "path_off", "paths", "routes")


def _snapshot(e):
    """Every per-record output of the last relaxation, as raw arrays."""
    ch = e.children_arrays()
    ns, nsol = int(ch[4][-1]), int(ch[6][-1])
    ch = ch[:5] + (ch[5][:ns], ch[6], ch[7][:nsol])
    off, buf = e.paths()
    vals = e.results_arrays() + e.stats() + (e.debug()[1],) + ch + (off, buf[:int(off[-1])], e.routes())
    return dict(zip(FIELDS, vals))


def _differences(a, b):
    return [f for f in FIELDS if a[f].dtype != b[f].dtype or a[f].tobytes() != b[f].tobytes()]


def _engine(monkeypatch, net, pool, slots, chunk, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if chunk is None:
        monkeypatch.delenv("SGUFP_RELAX_CHUNK", raising=False)
    else:
        monkeypatch.setenv("SGUFP_RELAX_CHUNK", str(chunk))
    e = E.Engine(net, 0, slots)
    e.add_cuts(pool)
    return e


def _launches(n_opt, q, parts):
    return parts * (1 + (n_opt + q - 1) // q)


def _compare(monkeypatch, net, pool, recs, runs, q, env, slots=256, parts=2):
    """Split (Q = q) against unsplit on the same records at every incumbent of `runs` [(incumbent,
    reference results or None)]; returns the unsplit snapshots."""
    base = _engine(monkeypatch, net, pool, slots, 0, env)
    split = _engine(monkeypatch, net, pool, slots, q, dict(env, SGUFP_RELAX_STREAMS=str(parts)))
    n_opt = sum(1 for c in pool if c.type == 0)
    snaps = []
    try:
        for inc, want in runs:
            want_b = base.relax(recs, inc)
            assert base.relax_launches() == 1
            a = _snapshot(base)
            got = split.relax(recs, inc)
            assert split.relax_launches() == _launches(n_opt, q, min(parts, len(recs)))
            b = _snapshot(split)
            assert not (b["status"] == 8).any(), "a suspended record left the relaxation"
            assert _differences(a, b) == [], f"Q={q} incumbent {inc!r}"
            if want is not None:
                for res in (want_b, got):
                    bad = golden_io.compare_results(res, want)
                    assert not bad, f"Q={q} incumbent {inc!r}: " + "\n".join(bad[:10])
                assert N._bound_bits(got) == N._bound_bits(want)
            snaps.append(a)
    finally:
        base.close()
        split.close()
    return snaps


def _kinds(snaps, n_feas, screened):
    """Records of the unsplit runs pruned by a feasibility cut, by the screen (the loop never ran an
    in-order optimality batch: sweeps = F cuts + screened cuts) and by a later, in-order cut."""
    f = s = late = 0
    for a in snaps:
        f += int((a["status"] == E.PRUNED_F).sum())
        o = a["status"] == E.PRUNED_O
        s += int((o & (a["sweeps"] == n_feas + screened)).sum())
        late += int((o & (a["sweeps"] > n_feas + screened)).sum())
    return f, s, late


@pytest.mark.parametrize("q", [0, 8])   # 0: Q = CB, one batch per launch
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("which", ["pool", "small"])
def test_split_partial_batches(monkeypatch, last_batch_case, which, cb, q):  # noqa: F811
    """The 133 DFS records of c2_s3_dfs_big (an odd count: chains of 66 and 67) under 5 F + 13 O and
    under 0 F + 4 O -- at CB 8 fewer optimality cuts than the screen takes -- at DOUBLE_MIN and the
    40th / 80th percentile of the reference's bounds.  The unsplit run holds non-exact survivors with
    children, exact records with a path, and records pruned by feasibility cuts and by the screen
    (which takes every optimality prune here: test_split_redos_cross_launches has the in-order ones)."""
    pool = last_batch_case[which]
    snaps = _compare(monkeypatch, last_batch_case["net"], pool, last_batch_case["recs"], last_batch_case[which + "_want"],
                     q or int(cb), {"SGUFP_CUT_BATCH": cb})
    a = snaps[0]
    assert int(((a["exact"] == 0) & (a["n_children"] > 0)).sum()) >= 4
    assert int(((a["exact"] == 1) & (np.diff(a["path_off"]) > 0)).sum()) >= 4
    n_feas, n_opt = sum(1 for c in pool if c.type == 1), sum(1 for c in pool if c.type == 0)
    f, s, late = _kinds(snaps, n_feas, min(int(cb), n_opt))
    print(f"pruned[{which} CB={cb}] feasibility {f} screen {s} later cut {late}")
    if which == "pool":
        assert f > 0 and s > 0, (f, s, late)


@pytest.mark.parametrize("exact_fast", ["0", "1"])
def test_split_exact_hand_off(monkeypatch, last_batch_case, exact_fast):  # noqa: F811
    """Exact DDs leave the head launch for the cut-parallel kernels (routes say so), or, with the
    hand-off disabled, run their optimality batches in the chunk launches."""
    snaps = _compare(monkeypatch, last_batch_case["net"], last_batch_case["pool"], last_batch_case["recs"],
                     last_batch_case["pool_want"], 4, {"SGUFP_CUT_BATCH": "4", "SGUFP_EXACT_FAST": exact_fast})
    assert int(snaps[0]["exact"].sum()) >= 4
    handed = sum(int((a["routes"] == E.ROUTE_EXACT_PHASE).sum()) for a in snaps)
    assert (handed > 0) == (exact_fast == "1"), handed


@pytest.mark.parametrize("parts", [1, 2, 3])
def test_split_one_record_and_chains(monkeypatch, last_batch_case, parts):  # noqa: F811
    """One record (a single chain whatever was asked for) and the whole batch on 1, 2 and 3 chains."""
    net, pool, recs = last_batch_case["net"], last_batch_case["pool"], last_batch_case["recs"]
    env = {"SGUFP_CUT_BATCH": "4"}
    runs = last_batch_case["pool_want"]
    for k in (0, len(recs) - 1):
        _compare(monkeypatch, net, pool, recs[k:k + 1], [(inc, w[k:k + 1]) for inc, w in runs[:2]], 4, env, parts=parts)
    _compare(monkeypatch, net, pool, recs, runs[1:2], 8, env, parts=parts)


def test_split_without_optimality_cuts(monkeypatch, last_batch_case):  # noqa: F811
    """5 F + 0 O: the head launches finish every record (no chunk launch follows, see _launches);
    the fixture c3_s4_dfs prunes by feasibility and restarts feasibility batches after redos."""
    feas = [c for c in last_batch_case["pool"] if c.type == 1]
    _compare(monkeypatch, last_batch_case["net"], feas, last_batch_case["recs"], [(pools.DOUBLE_MIN, None), (0.0, None)], 4,
             {"SGUFP_CUT_BATCH": "4"})
    name = "c3_s4_dfs"
    d = golden_io.case_dir(name)
    pool = pools.read_pool(golden_io.golden_file(d, "cuts.txt"))
    case = [c for c in golden_io.manifest() if c["name"] == name][0]
    runs = [(float.fromhex(r["incumbent"]), golden_io.parse_results_text(golden_io.read_golden(name, r["file"])))
            for r in case["runs"]]
    nodes = pools.read_nodes(f"{d}/nodes.txt")
    for cb in ("4", "8"):
        snaps = _compare(monkeypatch, f"{d}/net.txt", pool, nodes, runs, int(cb), {"SGUFP_CUT_BATCH": cb, "SGUFP_SCREEN": "0"})
        f, _, _ = _kinds(snaps, 0, 0)
        print(f"c3_s4_dfs CB={cb}: pruned by feasibility {f}")
        assert f > 0


@pytest.fixture(scope="module")
def redo_case(oracle_bin, tmp_path_factory):
    """The workload of tests/test_redo_refold.py's c2_case (C2 seed 1, 64 BFS records, 4 F + 12 O)."""
    return R._frontier_case(oracle_bin, tmp_path_factory.mktemp("redo"), "C2", 1, 4, 12)


@pytest.mark.parametrize("cb", ["4", "8"])
def test_split_redos_cross_launches(monkeypatch, redo_case, cb):
    """335 redos over the two finite incumbents (screen 0): with one batch per launch a batch
    restarted after a redo starts its own launch, with the counters carried over.  With no screen
    every optimality prune is an in-order cut's, in a chunk launch; some fall in a launch after the
    first (more than 4 F + CB cuts applied)."""
    snaps = _compare(monkeypatch, redo_case["net"], redo_case["pool"], redo_case["recs"], redo_case["want"], int(cb),
                     {"SGUFP_CUT_BATCH": cb, "SGUFP_SCREEN": "0"}, slots=64)
    redos = sum(int((a["redo"].astype(np.int64) & 0xFF).sum()) for a in snaps)
    _, first, late = _kinds(snaps, 4, int(cb))
    late += sum(int(((a["status"] == E.PRUNED_O) & (a["sweeps"] < 4 + int(cb))).sum()) for a in snaps)
    later = sum(int(((a["status"] == E.PRUNED_O) & (a["sweeps"] > 4 + int(cb))).sum()) for a in snaps)
    print(f"redos[CB={cb}] = {redos}; pruned by an in-order cut {first + late}, in a launch after the first {later}")
    assert redos > 0
    assert first + late > 0 and later > 0


@pytest.mark.parametrize("skip", ["0", "6"])
def test_split_nx_hand_off(monkeypatch, last_batch_case, redo_case, skip):  # noqa: F811
    """SGUFP_NX_MIN=1: non-exact survivors leave for the cut-parallel phase at the first loop position
    at or past SGUFP_NX_SKIP optimality cuts -- in the first chunk launch (0) or in a later one (6,
    between the launches of Q = 4) -- and the records the phase hands back are run again whole."""
    env = {"SGUFP_CUT_BATCH": "4", "SGUFP_NX": "1", "SGUFP_NX_MIN": "1", "SGUFP_NX_SKIP": skip}
    taken = 0
    for net, pool, recs, runs, slots in (
            (last_batch_case["net"], last_batch_case["pool"], last_batch_case["recs"], last_batch_case["pool_want"], 256),
            (redo_case["net"], redo_case["pool"], redo_case["recs"], redo_case["want"], 64)):
        base = _engine(monkeypatch, net, pool, slots, 0, env)
        split = _engine(monkeypatch, net, pool, slots, 4, env)
        try:
            for inc, want in runs:
                for e in (base, split):
                    bad = golden_io.compare_results(e.relax(recs, inc), want)
                    assert not bad, f"skip={skip} incumbent {inc!r}: " + "\n".join(bad[:10])
                a, b = _snapshot(base), _snapshot(split)
                assert _differences(a, b) == [], f"skip={skip} incumbent {inc!r}"
                taken += int((a["routes"] >= E.ROUTE_NX_PHASE).sum())
        finally:
            base.close()
            split.close()
    print(f"records through the cut-parallel phase[skip={skip}] = {taken}")
    assert taken > 0


def test_small_batches_keep_the_single_launch(monkeypatch, redo_case):
    """Default settings: a 64-record batch is far below the device's resident k_relax waves, so it
    runs as one k_relax launch."""
    for cb in (None, "4"):
        env = {} if cb is None else {"SGUFP_CUT_BATCH": cb}
        if cb is None:
            monkeypatch.delenv("SGUFP_CUT_BATCH", raising=False)
        e = _engine(monkeypatch, redo_case["net"], redo_case["pool"], 64, None, env)
        try:
            inc, want = redo_case["want"][1]
            bad = golden_io.compare_results(e.relax(redo_case["recs"], inc), want)
            assert not bad, "\n".join(bad[:10])
            assert e.relax_launches() == 1
        finally:
            e.close()
