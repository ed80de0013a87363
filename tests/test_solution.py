"""What a search leaves besides its value (sgufp_solver_amd/solver.py, solution.py): the routing
of the incumbent, the bound over the open frontier and the gap -- on the CPU, with the toy
knapsack engine of tests/test_solver_protocol.py.

The reference prints the value only (DDSolver.cpp:848-867), so there is nothing of it to compare
with: the toy's optimum comes from brute force, its routing is checked against the knapsack
itself, and matching_of_path against the oracle's y-bar (oracle/subproblem_oracle.py).
"""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import subproblem_oracle as so
from sgufp_solver_amd.pools import DOUBLE_MIN
from sgufp_solver_amd.solution import gap_of, matching_of_path
from sgufp_solver_amd.solver import DDSolver
from tests.test_solver_protocol import A, CAP, D, W, ToyEngine, _free_port, brute
from tests.test_subproblem import _full_matching, _net, _path_of


class ToySolutionEngine(ToyEngine):
    """ToyEngine with the Engine's bnb_incumbent / frontier_bound."""

    def __init__(self):
        super().__init__()
        self.inc = (DOUBLE_MIN, None)

    def frontier_clear(self):
        super().frontier_clear()
        self.inc = (DOUBLE_MIN, None)

    def bnb_step(self, z, max_nodes=0):
        n0 = len(self.closed)
        best, st = super().bnb_step(z, max_nodes)
        if best > z:   # the first leaf of the round, in batch order, that reaches the maximum
            for sol in self.closed[n0:]:
                if float(np.dot(W, sol)) == best:
                    self.inc = (best, list(sol))
                    break
        return best, st

    def bnb_incumbent(self):
        return self.inc

    def open_ubs(self, z):
        return [r.ub for r in self.stack if r.ub > z]

    def frontier_bound(self, z):
        ubs = self.open_ubs(z)
        return (max(ubs) if ubs else DOUBLE_MIN), len(ubs)


def _summary(solver, eng):
    r = solver.result()
    return dict(value=r.value, path=r.path, bound=r.bound, gap=r.gap, open_nodes=r.open_nodes, complete=r.complete,
                local_open=len(eng.open_ubs(r.value)), matching=r.matching)


def _check_complete(res, opt):
    for r in res:
        assert r["complete"]
        assert r["value"] == opt
        x = np.asarray(r["path"], dtype=float)
        assert x.shape == (D,) and set(x.tolist()) <= {0.0, 1.0}
        assert float(np.dot(W, x)) == r["value"] and float(np.dot(A, x)) <= CAP
        assert r["path"] == res[0]["path"]
        assert r["bound"] == r["value"] and r["gap"] == 0 and r["open_nodes"] == 0


def _check_stopped(res, opt):
    for r in res:
        assert not r["complete"]
        assert r["value"] <= opt <= r["bound"]
        assert r["open_nodes"] == sum(x["local_open"] for x in res) > 0
        assert r["bound"] == res[0]["bound"] and r["path"] == res[0]["path"]
        assert r["gap"] == (r["bound"] - r["value"]) / max(1.0, abs(r["value"]))


def test_matching_of_path_equals_the_oracle():
    inst, _, net = _net("C2", 1, 1)
    rng = np.random.default_rng(11)
    for _ in range(5):
        path = _path_of(inst, net, _full_matching(net, rng, 0.7))
        assert any(d >= 0 for d in path)
        assert matching_of_path(net.layer_arcs, inst.tails, inst.heads, path) == so.ybar_of_path(net, path)


def test_gap_values():
    assert gap_of(5.0, 7.5, False) == 0.5 and gap_of(-0.5, 0.5, False) == 1.0
    assert gap_of(5.0, 7.5, True) == 0.0
    assert gap_of(DOUBLE_MIN, 7.5, False) == float("inf")
    assert gap_of(5.0, None, False) is None


def test_single_rank_toy_solution():
    eng = ToySolutionEngine()
    solver = DDSolver(engine=eng, batch_nodes=5, verbose=False)
    assert solver.start_solver(-1.0) == brute()
    _check_complete([_summary(solver, eng)], brute())
    assert solver.best_value == brute() and solver.best_bound == brute() and solver.gap == 0


def test_single_rank_toy_stopped_early():
    eng = ToySolutionEngine()
    solver = DDSolver(engine=eng, batch_nodes=3, verbose=False, stop_rounds=3)
    solver.start_solver(-1.0)
    assert solver.rounds == 3
    _check_stopped([_summary(solver, eng)], brute())


def test_seed_nobody_beats_leaves_no_path():
    eng = ToySolutionEngine()
    seed = brute() + 1.0
    solver = DDSolver(engine=eng, batch_nodes=5, verbose=False)
    assert solver.start_solver(seed) == seed
    r = solver.result()
    assert r.complete and r.value == seed and r.path is None and r.bound == seed and r.gap == 0 and r.open_nodes == 0


def test_plain_toy_engine_still_solves():
    """An engine without bnb_incumbent / frontier_bound: the value as before, no routing, no bound."""
    solver = DDSolver(engine=ToyEngine(), batch_nodes=5, verbose=False)
    assert solver.start_solver(-1.0) == brute()
    r = solver.result()
    assert r.value == brute() and r.complete
    assert r.path is None and r.matching is None and r.bound is None and r.open_nodes is None


def _worker(rank, world, port, stop_rounds, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = ToySolutionEngine()
    solver = DDSolver(engine=eng, batch_nodes=3, verbose=False, stop_rounds=stop_rounds)
    solver.start_solver(-1.0)
    q.put((rank, _summary(solver, eng)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,stop_rounds", [(2, 0), (3, 0), (2, 3)])
def test_multi_rank_toy_solution(world, stop_rounds):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, stop_rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res = [s for _, s in sorted(res, key=lambda t: t[0])]
    (_check_stopped if stop_rounds else _check_complete)(res, brute())


@pytest.mark.parametrize("stop_rounds", [0, 3])
def test_in_process_shards_toy_solution(stop_rounds):
    from sgufp_solver_amd.shards import LocalComm, LocalGroup, run_local_shards
    world = 2
    group = LocalGroup(world)
    engines = [ToySolutionEngine() for _ in range(world)]
    solvers = [DDSolver(engine=engines[r], batch_nodes=3, verbose=False, comm=LocalComm(group, r),
                        stop_rounds=stop_rounds) for r in range(world)]
    run_local_shards(solvers, lambda s: s.start_solver(-1.0))
    res = [_summary(s, e) for s, e in zip(solvers, engines)]
    (_check_stopped if stop_rounds else _check_complete)(res, brute())
