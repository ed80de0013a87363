"""The incumbent's routing and the bound over the device frontier (sgufp_bnb_incumbent,
sgufp_incumbent_set / _sync, sgufp_frontier_bound; bnb.cpp, shard.cpp, k_frontier_bound).

The reference keeps and prints the incumbent's value only (DDSolver.cpp:848-867), so these are
checked against what they must mean: the bound against numpy over the peeked stack and against
the extensive-form optimum (oracle/extensive_form.py) after every round, the routing by solving
its scenario subproblem again -- on the device and with the oracle's LP -- which must give the
incumbent's value.  Tolerances are the suite's: 1e-9 relative for subproblem values
(tests/test_subproblem.py), 1e-5 for the optimum (tests/test_bnb.py), integers exact.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

from oracle import extensive_form as ef
from oracle import subproblem_oracle as so
from sgufp_solver_amd import engine as E
from sgufp_solver_amd import instance
from sgufp_solver_amd.pools import DOUBLE_MAX, DOUBLE_MIN, NodeRecord
from sgufp_solver_amd.solver import DDSolver
from tests import golden_io
from tests.test_bnb import E2E
from tests.test_native_shards import run_threads

pytestmark = pytest.mark.gpu
os.environ.setdefault("SGUFP_LOOPBACK_TIMEOUT", "60")

TOL_SUB = 1e-9
TOL_OPT = 1e-5
ROOT = NodeRecord(0, DOUBLE_MIN, DOUBLE_MAX, [], [])


@functools.lru_cache(maxsize=None)
def _case(cfg, seed, S):
    """(instance, network file, extensive-form optimum), made once per instance."""
    inst = instance.generate(instance.CONFIGS[cfg], seed, scenarios=S)
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_sol_"), "net.txt")
    inst.write(path)
    return inst, path, ef.solve(inst)


# ---- sgufp_frontier_bound against numpy over the peeked stack -----------------------------------
Z = 12.5


def _stack(n, with_max):
    """n synthetic root-like records: ub around the incumbent Z, equal to it (every 7th, the
    first one included: must not count as open), below it, negative, and DOUBLE_MAX once."""
    rng = np.random.default_rng(1000 + n)
    ub = np.round(rng.uniform(-50.0, 50.0, size=n), 3)
    ub[::7] = Z
    if with_max and n:
        ub[n // 2] = DOUBLE_MAX
    z0 = np.zeros(n + 1, dtype=np.int64)
    return E.batch_from_arrays(np.zeros(n, np.uint16), np.full(n, DOUBLE_MIN), ub, z0, np.zeros(1, np.int16), z0,
                               np.zeros(1, np.int16))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100003])
def test_frontier_bound_matches_numpy(native_lib, n):
    eng = E.Engine(os.path.join(golden_io.case_dir("c2_s2_dfs"), "net.txt"), 0, 64)
    try:
        for with_max in (False, True):
            eng.frontier_clear()
            b = _stack(n, with_max)
            if n:
                eng.frontier_push(b)
            assert eng.frontier_size() == n
            ub = eng.frontier_peek(0, n).ub if n else np.zeros(0)
            assert ub.tobytes() == b.ub.tobytes()
            for z in (Z, DOUBLE_MIN, -10.0, 50.0):
                is_open = ub > z
                want = (float(ub[is_open].max()) if is_open.any() else DOUBLE_MIN, int(is_open.sum()))
                assert eng.frontier_bound(z) == want, (n, with_max, z)
            if n and not with_max:   # the records equal to the incumbent are there, and not open
                assert (ub == Z).any() and eng.frontier_bound(Z)[1] == n - int((ub <= Z).sum())
            assert eng.frontier_size() == n
    finally:
        eng.close()


# ---- the bound brackets the optimum after every round ------------------------------------------
BRACKET = [("T2", 3, 3), ("T4", 2, 3), ("T4", 3, 3)]


@functools.lru_cache(maxsize=None)
def _bracket_run(cfg, seed, S, seeding):
    """bnb_step(z, 3) driven by hand; returns (rounds, final open count, failures)."""
    _, path, opt = _case(cfg, seed, S)
    tol = TOL_OPT * max(1.0, abs(opt))
    z = opt - 10.0 if seeding == "opt-10" else DOUBLE_MIN
    eng = E.Engine(path, 0, 256)
    bad, rounds, op = [], 0, -1
    try:
        eng.frontier_clear()
        eng.frontier_push([ROOT])
        while eng.frontier_size() > 0 and rounds < 20000:
            z, _ = eng.bnb_step(z, 3)
            rounds += 1
            mx, op = eng.frontier_bound(z)
            n = eng.frontier_size()
            ub = eng.frontier_peek(0, n).ub if n else np.zeros(0)
            print(f"{cfg}-{seed}-{S} {seeding} round {rounds}: z={z!r} max_ub={mx!r} open={op} stack={n} opt={opt!r}")
            if op != int((ub > z).sum()):
                bad.append((rounds, "open", op, int((ub > z).sum())))
            if (ub > z).any() and mx != float(ub[ub > z].max()):
                bad.append((rounds, "max_ub", mx))
            if not z <= opt + tol:
                bad.append((rounds, "z above the optimum", z, opt))
            if not opt <= max(z, mx) + tol:
                bad.append((rounds, "bound below the optimum", z, mx, opt))
        if eng.frontier_size() != 0:
            bad.append((rounds, "no termination"))
        if abs(z - opt) > tol:
            bad.append((rounds, "final value", z, opt))
    finally:
        eng.close()
    return rounds, op, bad


@pytest.mark.parametrize("cfg,seed,S", BRACKET, ids=[f"{c}-{s}-{S}" for c, s, S in BRACKET])
@pytest.mark.parametrize("seeding", ["none", "opt-10"])
def test_bound_brackets_the_optimum_every_round(native_lib, cfg, seed, S, seeding):
    rounds, final_open, bad = _bracket_run(cfg, seed, S, seeding)
    assert not bad, bad
    assert rounds >= 1 and final_open == 0


def test_bracket_cases_are_not_root_only(native_lib):
    assert max(_bracket_run(c, s, S, seeding)[0] for c, s, S in BRACKET for seeding in ("none", "opt-10")) >= 3


# ---- the incumbent's routing ---------------------------------------------------------------------
def _check_routing(solver, inst, path_file, opt, z):
    eng = solver.eng
    r = solver.result()
    assert r.value == z and abs(z - opt) <= TOL_OPT * max(1.0, abs(opt)), (z, opt)
    assert r.complete and r.bound == z and r.gap == 0 and r.open_nodes == 0
    path = r.path
    assert path is not None and len(path) <= eng.info.total_layers
    la = eng.processing_order()[0]
    chosen = set()
    for a, d in enumerate(path):
        if d == -1:
            continue
        q = int(inst.heads[la[a]])
        assert 0 <= d < inst.m and int(inst.tails[d]) == q, (a, d)     # an out-arc of the layer's V-bar node
        assert d not in chosen, (a, d)
        chosen.add(d)
    typ, _, _, obj_mean = eng.subproblem([path])
    assert typ[0] == 0
    print(f"z={z!r} device obj_mean={obj_mean[0]!r} opt={opt!r}")
    assert abs(obj_mean[0] - z) <= TOL_SUB * max(1.0, abs(z)), (obj_mean[0], z)
    net = so.from_instance(inst, la)
    want = so.evaluate(net, path)
    assert all(s == "optimal" for s, _ in want), want
    mean = sum(o for _, o in want) / net.S
    assert abs(mean - z) <= TOL_SUB * max(1.0, abs(z)), (mean, z)
    assert r.matching == so.ybar_of_path(net, path)
    assert eng.bnb_incumbent() == (z, path)
    # its recourse flows: every scenario optimal, the scenario mean of the objectives is z
    st, obj, frew, _, _ = solver.flows()
    assert (st == 0).all() and (frew == obj).all()
    assert abs(float(obj.sum()) / net.S - z) <= TOL_SUB * max(1.0, abs(z))


@pytest.mark.parametrize("cfg,seed,S", E2E, ids=[f"{c}-{s}-{S}" for c, s, S in E2E])
@pytest.mark.parametrize("seeding", ["none", "opt-10"])
def test_incumbent_path_gives_the_incumbent_value(native_lib, cfg, seed, S, seeding):
    inst, path, opt = _case(cfg, seed, S)
    solver = DDSolver(path, max_batch=1024, max_rounds=20000, verbose=False)
    try:
        z = solver.start_solver(opt - 10.0 if seeding == "opt-10" else DOUBLE_MIN)
        _check_routing(solver, inst, path, opt, z)
    finally:
        solver.eng.close()


VARIANTS = [("T2", 3, 3), ("T4", 2, 3), ("T4", 3, 3)]


@pytest.mark.parametrize("cfg,seed,S", VARIANTS, ids=[f"{c}-{s}-{S}" for c, s, S in VARIANTS])
@pytest.mark.parametrize("variant", ["deferred", "restricted"])
def test_incumbent_path_of_resumed_and_seeded_searches(native_lib, cfg, seed, S, variant):
    """round_iters=1 with batch_nodes=3: the leaf closes in a round that resumed its loop;
    restricted_width=8: the seed's routing counts until a leaf beats it."""
    inst, path, opt = _case(cfg, seed, S)
    kw = dict(round_iters=1, batch_nodes=3) if variant == "deferred" else dict(restricted_width=8)
    solver = DDSolver(path, max_batch=256, max_rounds=50000, verbose=False, **kw)
    try:
        z = solver.start_solver(DOUBLE_MIN)
        if variant == "deferred":
            print("resumed loops:", solver.counters["resumed"])
        _check_routing(solver, inst, path, opt, z)
    finally:
        solver.eng.close()


def test_seed_above_the_optimum_leaves_no_path(native_lib):
    _, path, opt = _case("T4", 3, 3)
    solver = DDSolver(path, max_batch=256, max_rounds=20000, verbose=False)
    try:
        seed = opt + 1.0
        assert solver.start_solver(seed) == seed
        r = solver.result()
        assert r.complete and r.value == seed and r.path is None and r.matching is None
        assert r.gap == 0 and r.bound == seed and r.open_nodes == 0
        assert solver.eng.bnb_incumbent() == (DOUBLE_MIN, None)
    finally:
        solver.eng.close()


def test_incumbent_set_round_trips(native_lib):
    _, path, _ = _case("T2", 3, 3)
    eng = E.Engine(path, 0, 16)
    try:
        assert eng.bnb_incumbent() == (DOUBLE_MIN, None)
        L = eng.info.total_layers
        p = [(-1 if k % 3 == 0 else k) for k in range(L)]
        eng.incumbent_set(41.25, p)
        assert eng.bnb_incumbent() == (41.25, p)
        eng.incumbent_set(-3.0, p[:1])
        assert eng.bnb_incumbent() == (-3.0, p[:1])
        eng.incumbent_sync(7.0)                       # one shard: a stored value != z is dropped
        assert eng.bnb_incumbent() == (DOUBLE_MIN, None)
        eng.incumbent_set(7.0, p)
        eng.incumbent_sync(7.0)
        assert eng.bnb_incumbent() == (7.0, p)
        with pytest.raises(RuntimeError):
            eng.incumbent_set(1.0, [0] * (L + 1))     # len <= total_layers
        eng.frontier_clear()
        assert eng.bnb_incumbent() == (DOUBLE_MIN, None)
    finally:
        eng.close()


# ---- loopback shards: one routing on every rank ----------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_loopback_shards_agree_on_the_routing(native_lib, world):
    inst, path, opt = _case("T4", 3, 3)
    single = DDSolver(path, max_batch=256, batch_nodes=16, max_rounds=20000, verbose=False)
    try:
        z1 = single.start_solver(DOUBLE_MIN)
    finally:
        single.eng.close()
    grp = E.LoopbackGroup(world)
    engs = [E.Engine(path, 0, 256) for _ in range(world)]
    for r, e in enumerate(engs):
        e.comm_init_loopback(grp, r)
    solvers = [DDSolver(engine=engs[r], batch_nodes=16, verbose=False, native_world=world, max_rounds=20000)
               for r in range(world)]
    try:
        zs = run_threads([lambda s=s: s.start_solver(DOUBLE_MIN) for s in solvers])
        print(f"world {world}: single-rank value {z1!r}, shard values {zs!r}")
        assert zs == [zs[0]] * world and abs(zs[0] - z1) <= TOL_OPT * max(1.0, abs(z1)), (zs, z1)
        z1 = zs[0]
        res = [s.result() for s in solvers]
        assert all(r.complete and r.value == z1 and r.bound == z1 and r.gap == 0 and r.open_nodes == 0 for r in res)
        assert res[0].path is not None and all(r.path == res[0].path for r in res)
        assert all(e.bnb_incumbent() == (z1, res[0].path) for e in engs)
        typ, _, _, obj_mean = engs[0].subproblem([res[0].path])
        assert typ[0] == 0 and abs(obj_mean[0] - z1) <= TOL_SUB * max(1.0, abs(z1))
        # a value no shard holds: every shard ends with none
        run_threads([lambda e=e: e.incumbent_sync(z1 + 1.0) for e in engs])
        assert all(e.bnb_incumbent() == (DOUBLE_MIN, None) for e in engs)
        # the lowest rank holding z owns the routing
        for r, e in enumerate(engs):
            if r >= 1:
                e.incumbent_set(5.0, [r, -1, r])
        run_threads([lambda e=e: e.incumbent_sync(5.0) for e in engs])
        assert all(e.bnb_incumbent() == (5.0, [1, -1, 1]) for e in engs)
    finally:
        for e in engs:
            e.close()
        grp.close()
