"""DD templates (Templates in dd_device.hpp; k_tpl_key / k_tpl_assign / k_tpl_build and dd_instantiate
in dd_kernels.hip): what dd_build and build_stream leave depends on a record's global layer and root
state set only, so a relaxation builds each (layer, state set) that two or more of its eligible
records -- valid, not bound-pruned, sol_len == gl -- share once, and those records copy it.

After the copy a record's slot holds what its own build leaves, so an engine under
SGUFP_RELAX_TEMPLATES=1 must give, byte for byte, what one under SGUFP_RELAX_TEMPLATES=0 gives on the
same upload (FIELDS / _snapshot of tests/test_relax_chunks.py), unsplit and split on two chains
(SGUFP_RELAX_CHUNK=8), at CB 4 and 8; where the CPU reference's results exist they are compared too.
Engine.relax_templates() is checked against a host census of (gl, sorted states, sol_len == gl).

What can go wrong: a copy that misses part of a range (peeled heads and tails, byte arrays whose
template and record slots disagree in alignment), edits of a record reaching the shared template
(redos, cascades: two members of a class pruned differently), a class past the pool's slots, records
that must not count (invalid, bound-pruned, singletons), templates at a batch size that keeps the
single launch.
"""
import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import pools
from tests import golden_io
from tests import test_bnb as B
from tests import test_narrow_fold as N
from tests import test_redo_refold as R
from tests.test_narrow_fold import last_batch_case  # noqa: F401  (fixture: c2_s3_dfs_big, 5 F + 13 O and 0 F + 4 O)
from tests.test_relax_chunks import _differences, _snapshot

pytestmark = pytest.mark.gpu

CHUNKS = [0, 8]   # unsplit, split on two chains


def _census(recs, skip=()):
    """Class sizes of the eligible records, keyed (gl, sorted states); `skip`: excluded positions."""
    classes = {}
    for k, r in enumerate(recs):
        if k in skip or len(r.sol) != r.gl:
            continue
        key = (r.gl, tuple(r.states))
        classes[key] = classes.get(key, 0) + 1
    return sorted(classes.values(), reverse=True)


def _expected(sizes):
    """(templates, instantiations) of a pool that holds every class of two records or more."""
    shared = [s for s in sizes if s >= 2]
    return len(shared), sum(shared)


def _engine(monkeypatch, net, pool, slots, templates, chunk, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SGUFP_RELAX_TEMPLATES", templates)
    monkeypatch.setenv("SGUFP_RELAX_CHUNK", str(chunk))
    monkeypatch.setenv("SGUFP_RELAX_STREAMS", "2")
    e = E.Engine(net, 0, slots)
    e.add_cuts(pool)
    return e


def _compare(monkeypatch, net, pool, recs, runs, chunk, env, slots=256, want_counts=None):
    """Templates on against off on the same records at every incumbent of `runs` [(incumbent,
    reference results or None)]; returns the snapshots of the engine without templates."""
    base = _engine(monkeypatch, net, pool, slots, "0", chunk, env)
    tpl = _engine(monkeypatch, net, pool, slots, "1", chunk, env)
    if want_counts is None:
        want_counts = _expected(_census(recs))
    snaps = []
    try:
        for inc, want in runs:
            want_b = base.relax(recs, inc)
            assert base.relax_templates() == (0, 0)
            a = _snapshot(base)
            got = tpl.relax(recs, inc)
            counts = tpl.relax_templates()
            assert base.relax_launches() == tpl.relax_launches()
            b = _snapshot(tpl)
            assert _differences(a, b) == [], f"chunk={chunk} incumbent {inc!r}"
            if callable(want_counts):
                want_counts(counts)
            else:
                assert counts == want_counts, f"chunk={chunk} incumbent {inc!r}"
            if want is not None:
                for res in (want_b, got):
                    bad = golden_io.compare_results(res, want)
                    assert not bad, f"chunk={chunk} incumbent {inc!r}: " + "\n".join(bad[:10])
                assert N._bound_bits(got) == N._bound_bits(want)
            snaps.append(a)
    finally:
        base.close()
        tpl.close()
    return snaps


def _golden(name):
    d = golden_io.case_dir(name)
    pool = pools.read_pool(golden_io.golden_file(d, "cuts.txt"))
    case = [c for c in golden_io.manifest() if c["name"] == name][0]
    runs = [(float.fromhex(r["incumbent"]), golden_io.parse_results_text(golden_io.read_golden(name, r["file"])))
            for r in case["runs"]]
    return f"{d}/net.txt", pool, pools.read_nodes(f"{d}/nodes.txt"), runs


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("name,sizes,counts", [("c2_s1_bfs", [80, 1], (1, 80)), ("c1_s1_bfs", [30, 30, 1], (2, 60)),
                                               ("w1_s1_wide", [117, 1, 1, 1, 1], (1, 117))])
def test_big_class_beside_a_singleton(monkeypatch, name, sizes, counts, cb, chunk):
    """BFS frontiers: one or two big classes and a singleton, which builds itself; w1_s1_wide: the
    wide-layer shape, 117 records in one class.  By (gl, states) alone the big classes of the two BFS
    fixtures hold 92 and 36 + 36 records; 12 of each fixture's records carry a solution shorter than
    their layer, are not eligible and build themselves."""
    net, pool, recs, runs = _golden(name)
    census = _census(recs)
    assert census == sizes and _expected(census) == counts
    _compare(monkeypatch, net, pool, recs, runs, chunk, {"SGUFP_CUT_BATCH": cb}, want_counts=counts)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("which", ["pool", "small"])
def test_many_classes(monkeypatch, last_batch_case, which, cb, chunk):  # noqa: F811
    """c2_s3_dfs_big: 133 records, chains of 66 and 67, under 5 F + 13 O and 0 F + 4 O.  By (gl, states)
    they fall into 18 classes: 104, triples and singletons; the triples' solutions are shorter than
    their layer, so among the eligible records one class of 104 stands beside 17 singletons."""
    recs = last_batch_case["recs"]
    census = _census(recs)
    assert len({(r.gl, tuple(r.states)) for r in recs}) == 18
    assert len(census) == 18 and census[0] == 104 and census.count(1) == 17
    _compare(monkeypatch, last_batch_case["net"], last_batch_case[which], recs, last_batch_case[which + "_want"], chunk,
             {"SGUFP_CUT_BATCH": cb})


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cb", ["4", "8"])
@pytest.mark.parametrize("name,slots", [("c3_s1_dfs", 2), ("c1_s1_bfs", 1)])
def test_a_small_pool(monkeypatch, name, slots, cb, chunk):
    """SGUFP_RELAX_TEMPLATE_SLOTS: c3_s1_dfs (50 classes by (gl, states); its eligible records are one
    class of 72 and singletons) under 2 slots, and c1_s1_bfs, two classes of 30, under 1: the class
    past the pool builds itself.  Which classes take the slots is not fixed, so the instantiations lie
    between the `slots` smallest and the `slots` largest classes of two or more."""
    net, pool, recs, runs = _golden(name)
    shared = [s for s in _census(recs) if s >= 2]
    if name == "c3_s1_dfs":
        assert len({(r.gl, tuple(r.states)) for r in recs}) == 50
    else:
        assert len(shared) > slots
    k = min(slots, len(shared))

    def check(counts):
        assert counts[0] == k
        assert sum(shared[-k:]) <= counts[1] <= sum(shared[:k])
    _compare(monkeypatch, net, pool, recs, runs, chunk, {"SGUFP_CUT_BATCH": cb, "SGUFP_RELAX_TEMPLATE_SLOTS": str(slots)},
             want_counts=check)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cb", ["4", "8"])
def test_one_record_and_64_copies(monkeypatch, last_batch_case, cb, chunk):  # noqa: F811
    """A single record makes no template; the same record 64 times is one class whose members agree
    in everything (first and last record of the fixture: different layers)."""
    net, pool, recs = last_batch_case["net"], last_batch_case["pool"], last_batch_case["recs"]
    env = {"SGUFP_CUT_BATCH": cb}
    full = [k for k, r in enumerate(recs) if len(r.sol) == r.gl]
    assert recs[full[0]].gl != recs[full[-1]].gl
    for k in (full[0], full[-1]):
        runs = [(inc, w[k:k + 1]) for inc, w in last_batch_case["pool_want"][:2]]
        _compare(monkeypatch, net, pool, recs[k:k + 1], runs, chunk, env, want_counts=(0, 0))
        many = [(inc, w * 64) for inc, w in runs]
        _compare(monkeypatch, net, pool, [recs[k]] * 64, many, chunk, env, want_counts=(1, 64))


@pytest.mark.parametrize("chunk", CHUNKS)
def test_invalid_records_count_for_nothing(monkeypatch, chunk):
    """Records the upload marks invalid (a decision id past the arcs) inside the big class of
    c2_s1_bfs: they stay out of the census and come back as before."""
    net, pool, recs, runs = _golden("c2_s1_bfs")
    big = [k for k, r in enumerate(recs) if len(r.sol) >= 1 and len(r.sol) == r.gl]
    bad = set(big[1:40:4])
    recs = [pools.NodeRecord(r.gl, r.lb, r.ub, r.states, [32000] + list(r.sol[1:])) if k in bad else r
            for k, r in enumerate(recs)]
    counts = _expected(_census(recs, skip=bad))
    assert counts == (1, 80 - len(bad))
    snaps = _compare(monkeypatch, net, pool, recs, [(inc, None) for inc, _ in runs], chunk, {"SGUFP_CUT_BATCH": "4"},
                     want_counts=counts)
    assert all(int((a["status"] == 16).sum()) == len(bad) for a in snaps)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_bound_pruned_records_count_for_nothing(monkeypatch, chunk):
    """A B&B round (tests/test_bnb.py): every third record of the frontier has ub <= the incumbent and
    is skipped unprocessed; the round's counters and the children it pushes are those of an engine
    without templates, and the pruned records are in no class."""
    inst, path = B._inst("C2", 1, 1)
    pool = pools.synthetic_pool(inst, 4, 12, 1)
    z = 100.0
    out = []
    for templates in ("0", "1"):
        eng = _engine(monkeypatch, path, pool, 256, templates, chunk, {"SGUFP_CUT_BATCH": "4"})
        try:
            recs = B._records(eng, 30)
            ub = recs.ub.copy()
            ub[::3] = 50.0
            recs = E.batch_from_arrays(recs.gl, recs.lb, ub, recs.states_off, recs.states, recs.sol_off, recs.sol)
            eng.frontier_clear()
            eng.frontier_push(recs)
            z2, st = eng.bnb_step(z)
            counts = eng.relax_templates()
            kids = eng.frontier_take(eng.frontier_size(), from_bottom=True)
            st = {k: v for k, v in st.as_dict().items() if k != "ms_relax"}
            out.append((z2, st, kids, counts, E.batch_to_records(recs)))
        finally:
            eng.close()
    (za, sa, ka, ca, _), (zb, sb, kb, cb_, recs) = out
    assert sa["pruned_bound"] == 10 and sa["relaxed"] == 20
    assert za == zb and sa == sb
    B._same(ka, kb)
    assert ca == (0, 0)
    assert cb_ == _expected(_census(recs, skip=set(range(0, 30, 3)))) and cb_[1] >= 2


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("exact_fast", ["0", "1"])
def test_exact_dds(monkeypatch, last_batch_case, exact_fast, chunk):  # noqa: F811
    """The exact DDs of the C2 fixture leave for the cut-parallel kernels (routes say so) or, with the
    hand-off disabled, run their optimality batches in k_relax -- from a copied DD."""
    snaps = _compare(monkeypatch, last_batch_case["net"], last_batch_case["pool"], last_batch_case["recs"],
                     last_batch_case["pool_want"], chunk, {"SGUFP_CUT_BATCH": "4", "SGUFP_EXACT_FAST": exact_fast})
    assert int(snaps[0]["exact"].sum()) >= 4
    handed = sum(int((a["routes"] == E.ROUTE_EXACT_PHASE).sum()) for a in snaps)
    assert (handed > 0) == (exact_fast == "1"), handed


@pytest.fixture(scope="module")
def redo_case(oracle_bin, tmp_path_factory):
    """The workload of tests/test_redo_refold.py's c2_case (C2 seed 1, 64 BFS records, 4 F + 12 O)."""
    return R._frontier_case(oracle_bin, tmp_path_factory.mktemp("redo_tpl"), "C2", 1, 4, 12)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("cb", ["4", "8"])
def test_redos_edit_a_private_copy(monkeypatch, redo_case, cb, chunk):
    """335 redos over the two finite incumbents (screen 0): the edits after the instantiation -- arc
    pruning, cascades, refolds -- must hit the record's copy.  Some class holds two members that end
    differently (pruned against not, or at different sweeps)."""
    recs = redo_case["recs"]
    snaps = _compare(monkeypatch, redo_case["net"], redo_case["pool"], recs, redo_case["want"], chunk,
                     {"SGUFP_CUT_BATCH": cb, "SGUFP_SCREEN": "0"}, slots=64)
    redos = sum(int((a["redo"].astype(np.int64) & 0xFF).sum()) for a in snaps)
    assert redos > 0
    differ = 0
    for a in snaps:
        ends = {}
        for k, r in enumerate(recs):
            if len(r.sol) == r.gl:
                ends.setdefault((r.gl, tuple(r.states)), set()).add((int(a["status"][k]), int(a["sweeps"][k])))
        differ += sum(1 for v in ends.values() if len(v) >= 2)
    print(f"redos[CB={cb}] = {redos}; classes whose members end differently {differ}")
    assert differ > 0


def test_default_settings_keep_small_batches_as_they_were(monkeypatch, redo_case):
    """Default settings: a 64-record batch is far below the device's resident k_relax waves: one
    k_relax launch and no template."""
    for var in ("SGUFP_RELAX_TEMPLATES", "SGUFP_RELAX_CHUNK", "SGUFP_RELAX_STREAMS", "SGUFP_RELAX_TEMPLATE_SLOTS",
                "SGUFP_CUT_BATCH"):
        monkeypatch.delenv(var, raising=False)
    e = E.Engine(redo_case["net"], 0, 64)
    try:
        e.add_cuts(redo_case["pool"])
        inc, want = redo_case["want"][1]
        bad = golden_io.compare_results(e.relax(redo_case["recs"], inc), want)
        assert not bad, "\n".join(bad[:10])
        assert e.relax_launches() == 1
        assert e.relax_templates() == (0, 0)
    finally:
        e.close()
