"""Best-bound node selection on the device frontier and the gap limit (sgufp_frontier_select,
select_kernels.hip; DDSolver node_selection / gap_limit; Inavap::DDSolver::nodeSelection / gapLimit).

The rule has one host statement, frontier.select_order; the toy engine of the CPU part and the
GPU checks both use it.  CPU: select_order against a brute-force sort, the driver's rounds on a
toy engine, the exported symbols.  GPU: the device call against select_order on synthetic stacks
of real records (bit for bit through frontier_peek), inside hand-driven searches, and through
the Python and C++ drivers.  Tolerances are the suite's: 1e-5 for the optimum (tests/test_bnb.py),
1e-9 relative for subproblem values (tests/test_subproblem.py); everything else is exact.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from sgufp_solver_amd import engine as E
from sgufp_solver_amd import frontier
from sgufp_solver_amd.pools import DOUBLE_MAX, DOUBLE_MIN, NodeRecord
from sgufp_solver_amd.solution import gap_of
from sgufp_solver_amd.solver import DDSolver
from tests import golden_io
from tests.test_solver_protocol import ToyEngine, brute

os.environ.setdefault("SGUFP_LOOPBACK_TIMEOUT", "60")

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT_DIR, "sgufp_solver_amd", "lib")
TOL_SUB = 1e-9
TOL_OPT = 1e-5
ROOT = NodeRecord(0, DOUBLE_MIN, DOUBLE_MAX, [], [])


# ---- the rule: select_order against a brute-force sort -------------------------------------------
def _brute_order(ub, k):
    """The rule spelled out with Python's sort on (ub, index) pairs."""
    n = len(ub)
    k = min(max(k, 0), n)
    ranked = sorted(range(n), key=lambda i: (-(float(ub[i]) + 0.0), -i))
    sel = set(ranked[:k])
    return [i for i in range(n) if i not in sel] + [i for i in range(n) if i in sel]


def _ks(n):
    return sorted({0, 1, 3, n - 1, n, n + 5} - {-1})


ADVERSARIAL = {
    "all_equal": np.full(9, 4.5),
    "all_max": np.full(7, DOUBLE_MAX),
    "zeros_mixed": np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0, -0.0]),
    "extremes": np.array([DOUBLE_MIN, DOUBLE_MAX, 0.0, DOUBLE_MAX, DOUBLE_MIN, 3.0, -3.0]),
    "duplicates_at_threshold": np.array([5.0, 2.0, 5.0, 7.0, 5.0, 5.0, 1.0, 5.0, 9.0, 5.0]),
    "single": np.array([1.0]),
    "empty": np.zeros(0),
}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_select_order_adversarial(name):
    ub = ADVERSARIAL[name]
    for k in _ks(len(ub)):
        perm = frontier.select_order(ub, k)
        assert perm.tolist() == _brute_order(ub, k), (name, k)
    if name in ("all_equal", "all_max"):   # best-bound degrades to LIFO: nothing moves
        for k in range(len(ub) + 2):
            assert frontier.select_order(ub, k).tolist() == list(range(len(ub)))


def test_select_order_random():
    rng = np.random.default_rng(11)
    for n in (2, 5, 64, 65, 300):
        for _ in range(4):
            ub = np.round(rng.uniform(-5.0, 5.0, size=n), 1)      # many duplicates
            for k in _ks(n) + [n // 2]:
                perm = frontier.select_order(ub, k)
                assert perm.tolist() == _brute_order(ub, k), (n, k)
                kk = min(max(k, 0), n)
                # the k largest end on top, both groups in their old order
                assert sorted(ub[perm[n - kk:]].tolist()) == sorted(ub.tolist())[n - kk:]
                assert (np.diff(perm[:n - kk]) > 0).all() and (np.diff(perm[n - kk:]) > 0).all()


def test_duplicates_straddling_the_threshold_take_the_topmost():
    ub = ADVERSARIAL["duplicates_at_threshold"]      # 9, 7, then six 5s at 0 2 4 5 7 9
    perm = frontier.select_order(ub, 4)
    assert perm[-4:].tolist() == [3, 7, 8, 9]          # the 5s nearest the top: indices 9 and 7


# ---- the driver's rounds on a toy engine ----------------------------------------------------------
class SelectToy(ToyEngine):
    """ToyEngine with frontier_select (on select_order) and frontier_bound; it logs its rounds."""

    def __init__(self):
        super().__init__()
        self.log = []

    def frontier_select(self, k=0, policy=E.SELECT_BEST_BOUND):
        k = k or 4
        self.log.append(("select", k))
        perm = frontier.select_order([r.ub for r in self.stack], k)
        self.stack = [self.stack[i] for i in perm]
        top = self.stack[len(self.stack) - min(k, len(self.stack)):]
        return len(top), min((r.ub for r in top), default=DOUBLE_MIN)

    def frontier_bound(self, z):
        ub = [r.ub for r in self.stack if r.ub > z]
        return (max(ub) if ub else DOUBLE_MIN), len(ub)

    def bnb_step(self, z, max_nodes=0):
        z, st = super().bnb_step(z, max_nodes)
        self.log.append(("step", st["exact"]))
        return z, st


def test_best_bound_on_the_toy_selects_once_per_round_after_the_dive():
    eng = SelectToy()
    solver = DDSolver(engine=eng, batch_nodes=3, dive_batch=2, verbose=False, node_selection="best_bound",
                      max_rounds=100000)
    assert solver.start_solver(-1.0) == brute() and solver.complete
    steps = [i for i, e in enumerate(eng.log) if e[0] == "step"]
    first_exact = next(i for i in steps if eng.log[i][1] > 0)
    assert first_exact > 0 and first_exact < steps[-1]
    assert all(e[0] == "step" for e in eng.log[:first_exact + 1])         # the dive: no select
    after = eng.log[first_exact + 1:]
    assert [e[0] for e in after] == ["select", "step"] * (len(after) // 2) and len(after) % 2 == 0
    assert all(e == ("select", 3) for e in after[::2])
    assert solver.rounds == len(steps)


def test_default_policy_never_selects_on_the_toy():
    eng = SelectToy()
    solver = DDSolver(engine=eng, batch_nodes=3, verbose=False)
    assert solver.node_selection == "lifo" and solver.gap_limit == 0.0
    assert solver.start_solver(-1.0) == brute()
    assert all(e[0] == "step" for e in eng.log)


def test_gap_limit_stops_the_toy_early():
    eng = SelectToy()
    solver = DDSolver(engine=eng, batch_nodes=3, dive_batch=2, verbose=False, node_selection="best_bound",
                      gap_limit=0.5, max_rounds=100000)
    z = solver.start_solver(-1.0)
    print(f"toy: z={z} bound={solver.best_bound} gap={solver.gap} rounds={solver.rounds} optimum={brute()}")
    assert not solver.complete and eng.frontier_size() > 0
    assert solver.gap is not None and 0.0 <= solver.gap <= 0.5
    assert z <= brute() <= solver.best_bound
    assert solver.best_bound == max(z, eng.frontier_bound(z)[0])           # _finish reports the same bound


def test_best_bound_needs_an_engine_with_frontier_select():
    with pytest.raises(ValueError):
        DDSolver(engine=ToyEngine(), verbose=False, node_selection="best_bound")
    with pytest.raises(ValueError):
        DDSolver(engine=SelectToy(), verbose=False, node_selection="depth")
    DDSolver(engine=ToyEngine(), verbose=False)                             # the default keeps working


def test_libraries_export_the_selection_api(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, "libsgufp_hip.so")], capture_output=True,
                         text=True, check=True).stdout
    assert " sgufp_frontier_select\n" in out
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIB, "libsgufp_host.so")], capture_output=True,
                         text=True, check=True).stdout
    assert "Inavap::DDSolver::nodeSelection(" in out
    assert os.access(os.path.join(LIB, "select_test"), os.X_OK)


# ---- the device call on synthetic stacks ----------------------------------------------------------
MAX_BATCH = 4200          # k = n - 1 is not clamped up to n = 4097
SIZES = [0, 1, 2, 63, 64, 65, 257, 4097, 100003]
FIELDS = ("gl", "lb", "ub", "states_off", "states", "sol_off", "sol")


def _same(a, b):
    return a.n == b.n and all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIELDS)


def _take(b, idx):
    """E.batch_slice(b, idx) without a Python loop over the records (stacks of 1e5 records)."""
    idx = np.asarray(idx, dtype=np.int64)

    def ragged(off, data):
        lens = off[idx + 1] - off[idx]
        new = np.zeros(len(idx) + 1, dtype=np.int64)
        np.cumsum(lens, out=new[1:])
        src = np.repeat(off[idx] - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)
        return new, data[src]
    st_off, st = ragged(b.states_off, b.states)
    so_off, so = ragged(b.sol_off, b.sol)
    return E.batch_from_arrays(b.gl[idx], b.lb[idx], b.ub[idx], st_off, st, so_off, so)


def _arena(eng):
    n, s = ctypes.c_int64(0), ctypes.c_int64(0)
    eng._check(eng.lib.sgufp_frontier_size(eng.ctx, ctypes.byref(n), ctypes.byref(s)))
    return n.value, s.value


@pytest.fixture(scope="module")
def select_engine(native_lib):
    """One engine on c2_s2_dfs and its base records: the root, its cutset children and their
    children (different masks and solution lengths, the root's empty)."""
    eng = E.Engine(os.path.join(golden_io.case_dir("c2_s2_dfs"), "net.txt"), 0, MAX_BATCH)
    base = E.batch_concat([E.BatchArrays([ROOT]), frontier.bfs_frontier(eng, 300)])
    lens = np.diff(base.sol_off)
    assert base.n > 64 and len(set(lens.tolist())) > 1 and (lens == 0).any()
    assert len(set(np.diff(base.states_off).tolist())) > 1
    yield eng, base
    eng.close()


def _stack(base, n, equal=False):
    """n records, the base ones repeated cyclically, under a synthetic ub pattern: rounded uniform
    values (duplicates), every 7th equal, one DOUBLE_MAX, -0.0 / 0.0 pairs and negatives."""
    b = _take(base, np.arange(n) % base.n)
    rng = np.random.default_rng(2000 + n)
    ub = np.round(rng.uniform(-50.0, 50.0, size=n), 1)
    ub[::7] = 12.5
    if n > 4:
        ub[n // 2] = DOUBLE_MAX
        ub[1], ub[n - 2] = -0.0, 0.0
    if n > 40:
        ub[11], ub[30] = 0.0, -0.0
    if equal:
        ub[:] = DOUBLE_MAX
    b.ub = np.ascontiguousarray(ub)
    b.lb = np.ascontiguousarray(rng.uniform(-1.0, 1.0, size=n))
    return b


def _load(eng, b):
    eng.frontier_clear()
    if b.n:
        eng.frontier_push(b)
    assert eng.frontier_size() == b.n


def _expect(ub, k):
    kk = MAX_BATCH if k <= 0 else min(k, MAX_BATCH)
    n = len(ub)
    perm = frontier.select_order(ub, kk) if kk < n else np.arange(n)
    m = min(kk, n)
    thr = float(np.min(ub[perm[n - m:]])) if m else DOUBLE_MIN
    return perm, m, thr


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_select_matches_select_order_on_synthetic_stacks(select_engine, n):
    eng, base = select_engine
    b = _stack(base, n)
    for k in [k for k in sorted({0, 1, 3, 64, n - 1, n, n + 1}) if k >= 0]:   # 0: max_batch
        _load(eng, b)
        before = eng.frontier_peek(0, n) if n else b
        assert _same(before, b)
        perm, m, thr = _expect(b.ub, k)
        sel, got_thr = eng.frontier_select(k)
        print(f"n={n} k={k}: selected {sel} threshold {got_thr!r} moved {int((perm != np.arange(n)).sum())}")
        assert (sel, got_thr) == (m, thr), (n, k)
        after = eng.frontier_peek(0, n) if n else b
        assert _same(after, _take(before, perm)), (n, k)
        size, arena = _arena(eng)
        total = int(np.diff(b.sol_off).sum())
        assert size == n and arena >= total
        if (perm != np.arange(n)).any():
            assert arena == total          # compacted to the records' lengths
        # a second identical select finds the selected records on top: nothing changes
        assert eng.frontier_select(k) == (m, thr)
        assert _same(eng.frontier_peek(0, n) if n else b, after) and _arena(eng) == (size, arena)
        assert eng.frontier_select(k, E.SELECT_LIFO)[0] == m


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 65, 4097])
def test_all_equal_bounds_leave_the_stack_as_it_was(select_engine, n):
    eng, base = select_engine
    b = _stack(base, n, equal=True)
    _load(eng, b)
    arena = _arena(eng)
    for k in (1, 3, 64, n - 1):
        assert eng.frontier_select(k) == (min(k, n), DOUBLE_MAX)
        assert _same(eng.frontier_peek(0, n), b) and _arena(eng) == arena


@pytest.mark.gpu
def test_unknown_policy_is_an_argument_error(select_engine):
    eng, base = select_engine
    _load(eng, _stack(base, 65))
    with pytest.raises(RuntimeError):
        eng.frontier_select(3, 7)
    assert _same(eng.frontier_peek(0, 65), _stack(base, 65))


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,m", [(65, 3, 5), (257, 64, 70), (4097, 64, 300)])
def test_take_and_push_after_a_select_round_trip(select_engine, n, k, m):
    """The arena invariant through the paths the shards use: take from the bottom and from the
    top of a selected stack, push both back."""
    eng, base = select_engine
    b = _stack(base, n)
    _load(eng, b)
    eng.frontier_select(k)
    after = eng.frontier_peek(0, n)
    assert _same(after, _take(b, frontier.select_order(b.ub, k)))
    low = eng.frontier_take(m, True)
    high = eng.frontier_take(m, False)
    assert _same(low, _take(after, np.arange(m))) and _same(high, _take(after, np.arange(n - m, n)))
    assert _same(eng.frontier_peek(0, n - 2 * m), _take(after, np.arange(m, n - m)))
    eng.frontier_push(low)
    eng.frontier_push(high)
    want = _take(after, np.concatenate([np.arange(m, n - m), np.arange(m), np.arange(n - m, n)]))
    assert _same(eng.frontier_peek(0, n), want)
    assert _arena(eng) == (n, int(np.diff(b.sol_off).sum()))
    # and a select over the pushed-back stack still follows the rule
    eng.frontier_select(k)
    assert _same(eng.frontier_peek(0, n), _take(want, frontier.select_order(want.ub, k)))


# ---- inside hand-driven searches --------------------------------------------------------------------
def _case(cfg, seed, S):
    from tests.test_solution_gpu import _case as case
    return case(cfg, seed, S)


BRACKET = [("T2", 3, 3), ("T4", 2, 3), ("T4", 3, 3)]


@functools.lru_cache(maxsize=None)
def _hand_run(cfg, seed, S, policy, round_iters=0):
    """bnb_step(z, 3) driven by hand, under best-bound with select(3) before every step and every
    select checked against select_order.  Returns a dict of what the run saw."""
    _, path, opt = _case(cfg, seed, S)
    tol = TOL_OPT * max(1.0, abs(opt))
    eng = E.Engine(path, 0, 256)
    z, rounds, bad = DOUBLE_MIN, 0, []
    first_finite, away, resumed, deferred, gaps = None, 0, 0, 0, []
    last_deferred = 0
    try:
        eng.bnb_set_trace(True)
        if round_iters:
            eng.bnb_set_limits(round_iters, 0.0)
        eng.frontier_clear()
        eng.frontier_push([ROOT])
        while eng.frontier_size() > 0 and rounds < 30000:
            n = eng.frontier_size()
            want_ub = None
            if policy == "best_bound":
                before = eng.frontier_peek(0, n)
                perm, m, thr = _expect(before.ub, 3)
                if (eng.frontier_select(3)) != (m, thr):
                    bad.append((rounds, "selected / threshold"))
                after = eng.frontier_peek(0, n)
                if not _same(after, _take(before, perm)):
                    bad.append((rounds, "permutation"))
                want_ub = before.ub[perm[n - m:]]
                # the records a round deferred lie on top: did the select leave some of them below?
                if last_deferred and (perm[n - m:] < n - last_deferred).any():
                    away += 1
            z, st = eng.bnb_step(z, 3)
            rounds += 1
            resumed += int(st.resumed)
            deferred += int(st.deferred)
            last_deferred = int(st.deferred)
            if want_ub is not None:
                popped = np.array([t[3] for t in eng.bnb_trace(0)])
                if popped.tobytes() != np.ascontiguousarray(want_ub).tobytes():
                    bad.append((rounds, "popped ub", popped.tolist(), want_ub.tolist()))
            mx, _ = eng.frontier_bound(z)
            bound = max(z, mx)
            if first_finite is None and bound < DOUBLE_MAX:
                first_finite = rounds
            gaps.append(gap_of(z, bound, False))
            if not z <= opt + tol:
                bad.append((rounds, "z above the optimum", z, opt))
            if not opt <= bound + tol:
                bad.append((rounds, "bound below the optimum", z, mx, opt))
        if eng.frontier_size() != 0:
            bad.append((rounds, "no termination"))
        if abs(z - opt) > tol:
            bad.append((rounds, "final value", z, opt))
    finally:
        eng.close()
    return dict(rounds=rounds, bad=bad, first_finite=first_finite, away=away, resumed=resumed, deferred=deferred,
                gaps=gaps, z=z, opt=opt)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S", BRACKET, ids=[f"{c}-{s}-{S}" for c, s, S in BRACKET])
def test_select_inside_a_search(native_lib, cfg, seed, S):
    r = _hand_run(cfg, seed, S, "best_bound")
    finite = [g for g in r["gaps"] if g != float("inf") and g < 1e300]
    print(f"{cfg}-{seed}-{S} best-bound: {r['rounds']} rounds, bound finite from round {r['first_finite']}, "
          f"finite gaps from {finite[:1]} to {finite[-1:]}")
    assert not r["bad"], r["bad"][:5]
    assert r["rounds"] >= 1


@pytest.mark.gpu
def test_best_bound_makes_the_bound_finite_no_later_than_lifo(native_lib):
    bb = _hand_run("T4", 3, 3, "best_bound")
    lifo = _hand_run("T4", 3, 3, "lifo")
    print(f"T4-3-3: bound first finite at round {bb['first_finite']} of {bb['rounds']} under best-bound, "
          f"{lifo['first_finite']} of {lifo['rounds']} under LIFO")
    assert not lifo["bad"], lifo["bad"][:5]
    assert bb["first_finite"] is not None and lifo["first_finite"] is not None
    assert bb["first_finite"] <= lifo["first_finite"]


@pytest.mark.gpu
def test_deferred_records_selected_away_resume_later(native_lib):
    """round_iters = 1: loops are cut after one iteration and their records go back on top with
    the bound reached; best-bound may pop others next.  Popped later, they resume (the seen
    lists are kept by record content) and the search still ends at the optimum."""
    r = _hand_run("T4", 3, 3, "best_bound", 1)
    print(f"T4-3-3 round_iters=1: {r['rounds']} rounds, deferred {r['deferred']}, resumed {r['resumed']}, "
          f"rounds whose select left a just-deferred record below: {r['away']}")
    assert not r["bad"], r["bad"][:5]
    assert r["deferred"] > 0 and r["resumed"] > 0 and r["away"] > 0


# ---- the drivers ---------------------------------------------------------------------------------------
def _check(solver, opt, z):
    r = solver.result()
    assert r.value == z and abs(z - opt) <= TOL_OPT * max(1.0, abs(opt)), (z, opt)
    assert r.complete and r.gap == 0 and r.bound == z and r.open_nodes == 0
    assert r.path is not None
    typ, _, _, obj_mean = solver.eng.subproblem([r.path])
    assert typ[0] == 0 and abs(obj_mean[0] - z) <= TOL_SUB * max(1.0, abs(z)), (obj_mean[0], z)


def _e2e():
    from tests.test_bnb import E2E
    return E2E


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S", _e2e(), ids=[f"{c}-{s}-{S}" for c, s, S in _e2e()])
@pytest.mark.parametrize("seeding", ["none", "opt-10"])
def test_best_bound_driver_reaches_the_optimum(native_lib, cfg, seed, S, seeding):
    _, path, opt = _case(cfg, seed, S)
    solver = DDSolver(path, max_batch=1024, max_rounds=20000, verbose=False, node_selection="best_bound")
    try:
        z = solver.start_solver(opt - 10.0 if seeding == "opt-10" else DOUBLE_MIN)
        print(f"{cfg}-{seed}-{S} {seeding}: z={z!r} rounds={solver.rounds}")
        _check(solver, opt, z)
    finally:
        solver.eng.close()


@pytest.mark.gpu
def test_best_bound_driver_with_deferred_loops(native_lib):
    _, path, opt = _case("T4", 3, 3)
    solver = DDSolver(path, max_batch=256, max_rounds=50000, verbose=False, node_selection="best_bound",
                      round_iters=1, batch_nodes=3)
    try:
        z = solver.start_solver(DOUBLE_MIN)
        print(f"deferred {solver.counters['deferred']} resumed {solver.counters['resumed']} rounds {solver.rounds}")
        assert solver.counters["deferred"] > 0 and solver.counters["resumed"] > 0
        _check(solver, opt, z)
    finally:
        solver.eng.close()


@pytest.mark.gpu
def test_gap_limit_stops_the_driver_early(native_lib):
    """T4-3-3 at 3 records a round under best-bound with round_iters = 1.  The root's children
    carry DOUBLE_MAX and best-bound pops them first; the records their rounds deferred wait below
    with the finite bound their loops reached, so once the last child is gone the gap is finite
    and positive for some rounds.  The limit is the largest such gap of the hand-driven run of the
    same rounds: the driver must stop there, not at the empty frontier."""
    _, path, opt = _case("T4", 3, 3)
    tol = TOL_OPT * max(1.0, abs(opt))
    hand = _hand_run("T4", 3, 3, "best_bound", 1)
    finite = [g for g in hand["gaps"] if 0.0 < g < 1e300]
    print(f"hand-driven: {hand['rounds']} rounds, {len(finite)} with a finite positive gap: {finite[:3]} ... {finite[-3:]}")
    assert finite, "no round of the hand-driven run has a finite positive gap"
    limit = max(finite)
    solver = DDSolver(path, max_batch=256, max_rounds=50000, verbose=False, node_selection="best_bound",
                      batch_nodes=3, dive_batch=0, round_iters=1, gap_limit=limit)
    try:
        z = solver.start_solver(DOUBLE_MIN)
        r = solver.result()
        print(f"gap_limit {limit!r}: z={z!r} bound={r.bound!r} gap={r.gap!r} open={r.open_nodes} "
              f"rounds={solver.rounds} of {hand['rounds']} opt={opt!r}")
        assert not r.complete and solver.eng.frontier_size() > 0 and solver.rounds < hand["rounds"]
        assert 0.0 <= r.gap <= limit
        assert r.bound >= opt - tol and z <= opt + tol
    finally:
        solver.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_loopback_shards_reach_the_optimum_under_best_bound(native_lib, world):
    from tests.test_native_shards import run_threads
    _, path, opt = _case("T4", 3, 3)
    grp = E.LoopbackGroup(world)
    engs = [E.Engine(path, 0, 256) for _ in range(world)]
    for r, e in enumerate(engs):
        e.comm_init_loopback(grp, r)
    solvers = [DDSolver(engine=engs[r], batch_nodes=16, verbose=False, native_world=world, max_rounds=20000,
                        node_selection="best_bound") for r in range(world)]
    try:
        zs = run_threads([lambda s=s: s.start_solver(DOUBLE_MIN) for s in solvers])
        print(f"world {world}: values {zs!r} optimum {opt!r} rounds {[s.rounds for s in solvers]}")
        assert zs == [zs[0]] * world and abs(zs[0] - opt) <= TOL_OPT * max(1.0, abs(opt))
        res = [s.result() for s in solvers]
        assert all(r.complete and r.gap == 0 and r.bound == zs[0] and r.open_nodes == 0 for r in res)
    finally:
        for e in engs:
            e.close()
        grp.close()


@pytest.mark.gpu
def test_cpp_driver_makes_the_python_driver_s_rounds_under_best_bound(native_lib):
    _, path, opt = _case("T4", 3, 3)
    r = subprocess.run([os.path.join(LIB, "select_test"), path, "none", "best_bound"], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    value, complete, rounds = float.fromhex(lines["solution"][0]), int(lines["solution"][3]), int(lines["rounds"][0])
    solver = DDSolver(path, verbose=False, max_rounds=20000, node_selection="best_bound")
    try:
        z = solver.start_solver(DOUBLE_MIN)
        print(f"C++ value {value!r} in {rounds} rounds; Python value {z!r} in {solver.rounds} rounds")
        assert value.hex() == z.hex() and complete == 1 and rounds == solver.rounds
        assert abs(z - opt) <= TOL_OPT * max(1.0, abs(opt))
    finally:
        solver.eng.close()
    bad = subprocess.run([os.path.join(LIB, "select_test"), path, "none", "7"], capture_output=True, text=True,
                         timeout=240)
    assert bad.returncode == 1 and "unknown policy" in bad.stderr


# ---- the default path is the parent's ------------------------------------------------------------------
class _Recording(E.Engine):
    def __init__(self, *a):
        super().__init__(*a)
        self.per_round = []
        self.selects = 0

    def bnb_step(self, incumbent, max_nodes=0):
        z, st = super().bnb_step(incumbent, max_nodes)
        d = st.as_dict()
        d.pop("ms_relax", None)
        self.per_round.append((z, max_nodes, d))
        return z, st

    def frontier_select(self, k=0, policy=E.SELECT_BEST_BOUND):
        self.selects += 1
        return super().frontier_select(k, policy)


@pytest.mark.gpu
def test_default_policy_rounds_are_unchanged(native_lib):
    _, path, opt = _case("T4", 3, 3)
    runs = []
    for kw in ({}, {"node_selection": "lifo"}):
        eng = _Recording(path, 0, 256)
        try:
            solver = DDSolver(engine=eng, batch_nodes=16, verbose=False, max_rounds=20000, **kw)
            z = solver.start_solver(DOUBLE_MIN)
            assert eng.selects == 0
            runs.append((z, eng.per_round, eng.cuts_count(0), eng.cuts_count(1), dict(solver.counters)))
        finally:
            eng.close()
    assert runs[0] == runs[1]
    assert abs(runs[0][0] - opt) <= TOL_OPT * max(1.0, abs(opt))
