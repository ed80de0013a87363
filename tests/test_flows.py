"""The recourse flows of a routing (sgufp_subproblem_flows, k_flow_summary).

The reference's subproblem keeps the cut only (grb.cpp:139-360), so the exported flows are
checked against what an optimal flow must satisfy in the scenario's network -- conservation,
the scenario's bounds, the matching's coupling of in- and out-arcs at the V-bar nodes -- and
against the objective: sum_a reward_a x_a must equal the device objective exactly, and that
objective the oracle's LP (oracle/subproblem_oracle.py) within 1e-9 relative
(tests/test_subproblem.py's tolerance) on the networks it solves in seconds (m <= 200).
"""
import numpy as np
import pytest

from oracle import subproblem_oracle as so
from tests.test_subproblem import _full_matching, _net, _path_of

pytestmark = pytest.mark.gpu

TOL = 1e-9
# (cfg, seed, S, zero_lb, trials) and the oracle's (optimal, infeasible) scenario counts over the
# trials' paths, from a CPU run of this recipe (None: network too large for the oracle here)
CASES = [("T2", 3, 3, False, 6, (16, 2)), ("P1", 1, 4, False, 6, (15, 9)), ("C2", 2, 3, True, 6, (18, 0)),
         ("C3", 1, 4, True, 3, None), ("C5", 1, 2, True, 2, None)]


def _check_flow(inst, net, y, s, x):
    """x [m]: an optimal scenario's flow under matching y."""
    T, H = np.asarray(inst.tails), np.asarray(inst.heads)
    assert (x >= inst.lb[:, s]).all() and (x <= inst.ub[:, s]).all()
    fin = np.bincount(H, weights=x, minlength=inst.n)
    fout = np.bincount(T, weights=x, minlength=inst.n)
    inner = (np.bincount(H, minlength=inst.n) > 0) & (np.bincount(T, minlength=inst.n) > 0)
    assert (fin[inner] == fout[inner]).all()
    arc = {(int(T[a]), int(H[a])): a for a in range(inst.m)}
    used_in, used_out = set(), set()
    for (i, q, j) in y:
        a, b = arc[(i, q)], arc[(q, j)]
        assert x[a] == x[b], (i, q, j)
        used_in.add(a)
        used_out.add(b)
    for q in net.vbar:
        q = int(q)
        for a in range(inst.m):
            if (int(H[a]) == q and a not in used_in) or (int(T[a]) == q and a not in used_out):
                assert x[a] == 0, (q, a)


@pytest.mark.parametrize("cfg,seed,S,zl,trials,counts", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_flows_are_optimal_flows_of_the_routing(native_lib, cfg, seed, S, zl, trials, counts):
    from sgufp_solver_amd import engine as E
    inst, path, net = _net(cfg, seed, S, zl)
    eng = E.Engine(path, 0, 64)
    try:
        rng = np.random.default_rng(100 + seed)
        ys = [_full_matching(net, rng, 1.0 if t % 2 == 0 else 0.85) for t in range(trials)]
        paths = [_path_of(inst, net, y) for y in ys]
        n_cuts = (eng.cuts_count(1), eng.cuts_count(0))
        before = eng.subproblem(paths)
        st, obj, frew, x, mean = eng.subproblem_flows(paths)
        after = eng.subproblem(paths)
        # state isolation: pools untouched, the plain subproblem unchanged, warm starts still there
        assert (eng.cuts_count(1), eng.cuts_count(0)) == n_cuts
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        warm = eng.subproblem(paths, warm_src=[-1] * trials, warm_dst=list(range(trials)))
        assert (warm[0] == before[0]).all()
        assert x.shape == (trials, S, inst.m) and x.dtype == np.int16 and mean.shape == (trials, inst.m)
        reward = np.asarray(inst.reward)[:, 0].astype(np.int64)
        oracle = inst.m <= 200
        n_opt = n_inf = 0
        for k, y in enumerate(ys):
            want = [so.dual_lp(net, y, s)[:2] for s in range(S)] if oracle else None
            if oracle:
                n_opt += sum(w == "optimal" for w, _ in want)
                n_inf += sum(w == "infeasible" for w, _ in want)
                first_inf = next((s for s, (w, _) in enumerate(want) if w == "infeasible"), S)
                assert (st[k, :first_inf] == 0).all(), (k, st[k], want)
                if first_inf < S:
                    assert st[k, first_inf] == 1, (k, st[k], want)
            # the first-infeasible stop: a scenario is left unsolved only behind an infeasible one
            assert set(st[k].tolist()) <= {0, 1, 3}, st[k]
            for s in range(S):
                if st[k, s] == 3:
                    assert (st[k, :s] == 1).any(), st[k]
                if st[k, s] != 0:
                    assert not x[k, s].any(), (k, s)
                    continue
                _check_flow(inst, net, y, s, x[k, s].astype(np.int64))
                assert frew[k, s] == obj[k, s] == float((reward * x[k, s].astype(np.int64)).sum()), (k, s)
                if oracle:
                    wo = want[s][1]
                    assert abs(obj[k, s] - wo) <= TOL * max(1.0, abs(wo)), (k, s, obj[k, s], wo)
            if (st[k] == 0).all():
                assert mean[k].tobytes() == (x[k].sum(axis=0, dtype=np.int64) / S).tobytes()
            else:
                assert not mean[k].any()
        print(f"{cfg}-{seed}-{S}: device optimal {int((st == 0).sum())} infeasible {int((st == 1).sum())} "
              f"unsolved {int((st == 3).sum())}; oracle optimal {n_opt} infeasible {n_inf}")
        if counts is not None:
            assert (n_opt, n_inf) == counts
        assert (st == 0).any()
    finally:
        eng.close()


def test_flows_of_no_paths_and_bad_paths(native_lib):
    from sgufp_solver_amd import engine as E
    inst, path, net = _net("T2", 3, 3)
    eng = E.Engine(path, 0, 16)
    try:
        st, obj, frew, x, mean = eng.subproblem_flows([])
        assert st.shape == (0, 3) and x.shape == (0, 3, inst.m) and mean.shape == (0, inst.m)
        with pytest.raises(RuntimeError):
            eng.subproblem_flows([[-1] * (eng.info.total_layers + 1)])
    finally:
        eng.close()
