"""Scenario subproblem (GuroSolver::solveSubProblem, /root/reference/grb.cpp:139-360).

CPU tests pin the oracle (oracle/subproblem_oracle.py: the reference's dual LP restated,
solved by HiGHS) against the primal it is the dual of.  GPU tests compare the HIP
kernels (k_sub_scenario / k_sub_reduce through sgufp_subproblem) with the oracle:
per-scenario status and objective (1e-9 relative; the data are integral), tightness of
the returned cut at y-bar and validity at other matchings.  Parity at the Gurobi boundary
is unpinned (no reference fixture; duals are not unique), see DESIGN.md.
"""
import os
import tempfile

import numpy as np
import pytest

from oracle import subproblem_oracle as so
from sgufp_solver_amd import instance

TOL = 1e-9


def _net(cfg, seed, S, zero_lb=False):
    """Seeded instance (S None: the config's scenario count); zero_lb drops the sink-arc
    lower bounds so that most matchings are feasible (optimality cuts), otherwise many
    scenarios are infeasible (feasibility cuts)."""
    from sgufp_solver_amd import engine as E
    inst = instance.generate(instance.CONFIGS[cfg], seed, scenarios=S)
    if zero_lb:
        inst.lb[:] = 0
    d = tempfile.mkdtemp(prefix="sgufp_sub_")
    path = os.path.join(d, "net.txt")
    inst.write(path)
    L, la, vb = E.probe_network(path)
    return inst, path, so.from_instance(inst, la)


def _path_of(inst, net, y):
    """DD decisions per layer for a matching y (the inverse of ybar_of_path)."""
    outs = {}
    for b in range(inst.m):
        outs.setdefault(int(inst.tails[b]), []).append(b)
    path = []
    for a in net.layer_arcs:
        q, i = int(inst.heads[a]), int(inst.tails[a])
        d = -1
        for b in outs.get(q, []):
            if y.get((i, q, int(inst.heads[b])), 0):
                d = b
        path.append(d)
    return path


def _full_matching(net, rng, p_match=1.0):
    """Random matching that matches as many in-arcs as possible (feasible more often)."""
    T, H = net.tails, net.heads
    y = {}
    for q in net.vbar:
        q = int(q)
        ins = [a for a in range(net.m) if int(H[a]) == q]
        outs = [int(H[b]) for b in range(net.m) if int(T[b]) == q]
        rng.shuffle(ins)
        free = list(outs)
        rng.shuffle(free)
        for ai in ins:
            if free and rng.random() < p_match:
                y[(int(T[ai]), q, free.pop())] = 1
    return y


@pytest.mark.parametrize("cfg,seed,S,zl", [("C1", 1, 1, False), ("C1", 2, 1, True), ("C2", 1, 2, False),
                                           ("C2", 3, 2, True)])
def test_oracle_dual_equals_primal(cfg, seed, S, zl):
    inst, _, net = _net(cfg, seed, S, zl)
    rng = np.random.default_rng(seed)
    n_opt = 0
    for trial in range(6):
        y = _full_matching(net, rng, p_match=1.0 if trial % 2 == 0 else 0.8)
        for s in range(net.S):
            st, obj, _ = so.dual_lp(net, y, s)
            pst, pobj = so.primal_lp(net, y, s)
            assert st == pst
            if st == "optimal":
                n_opt += 1
                assert abs(obj - pobj) <= TOL * max(1.0, abs(obj))
    assert n_opt > 0 or not zl


@pytest.mark.parametrize("lb_last", [0, 2])
def test_oracle_dual_equals_primal_with_a_source_to_sink_arc(lb_last):
    """An arc source -> sink (the generator makes none): the reference empties that arc set
    (A4, Network.cpp:80; the 7j rows are commented out, grb.cpp:126-133), so the dual has no row
    for the arc and the primal leaves it out; its beta stays in the dual objective, so a positive
    lower bound on it (here: in the last scenario) makes that scenario infeasible in both."""
    from sgufp_solver_amd import engine as E
    from tests.helpers import sub_families as fam
    inst = fam.direct_arc(2, lb_last)
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_sub_"), "net.txt")
    inst.write(path)
    net = so.from_instance(inst, E.probe_network(path)[1])
    base = so.from_instance(fam.make("T2", 2, 2, "plain"), net.layer_arcs)
    rng = np.random.default_rng(7)
    for trial in range(4):
        y = _full_matching(net, rng, p_match=1.0 if trial % 2 == 0 else 0.8)
        for s in range(net.S):
            st, obj, _ = so.dual_lp(net, y, s)
            pst, pobj = so.primal_lp(net, y, s)
            assert st == pst == ("infeasible" if lb_last and s == net.S - 1 else "optimal")
            if st == "optimal":
                assert abs(obj - pobj) <= TOL * max(1.0, abs(obj))
                assert abs(obj - so.dual_lp(base, y, s)[1]) <= TOL * max(1.0, abs(obj))   # the arc earns nothing


def test_path_roundtrip():
    inst, _, net = _net("C2", 1, 1)
    rng = np.random.default_rng(5)
    for _ in range(5):
        y = _full_matching(net, rng, 0.7)
        assert so.ybar_of_path(net, _path_of(inst, net, y)) == y


# ----------------------------------------------------------------------------------- GPU
def _keys(eng):
    ks = eng.slot_keys()
    out = []
    for k in ks:
        k = int(k)
        out.append((k >> 16 & 0xFFFF, k & 0xFFFF, k >> 32 & 0xFFFF))   # (i, q, j)
    return out


def _cut_at(rhs, row, keys, y):
    v = rhs
    for s, k in enumerate(keys):
        if y.get(k, 0):
            v += row[s]
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S,zl,trials", [("C1", 1, 1, False, 6), ("C1", 2, 1, True, 6),
                                                   ("C2", 1, 2, False, 6), ("C2", 2, 3, True, 6),
                                                   ("C3", 1, 4, True, 3), ("C3", 2, 3, False, 3),
                                                   ("C5", 1, 2, True, 2), ("C5", 2, 2, False, 2)])
def test_subproblem_matches_highs(cfg, seed, S, zl, trials):
    from sgufp_solver_amd import engine as E
    inst, path, net = _net(cfg, seed, S, zl)
    eng = E.Engine(path, 0, 64)
    keys = _keys(eng)
    rng = np.random.default_rng(100 + seed)
    ys = [_full_matching(net, rng, 1.0 if t % 2 == 0 else 0.85) for t in range(trials)]
    paths = [_path_of(inst, net, y) for y in ys]
    typ, rhs, rows, obj_mean = eng.subproblem(paths)
    st, obj, dual = eng.subproblem_detail(len(paths))
    seen = set()
    for k, y in enumerate(ys):
        want = [so.dual_lp(net, y, s)[:2] for s in range(net.S)]
        first_inf = next((s for s, (w, _) in enumerate(want) if w == "infeasible"), None)
        for s, (ws, wo) in enumerate(want):
            if first_inf is not None and s > first_inf:
                continue                      # the reference stops at the first infeasible one
            assert st[k, s] == (0 if ws == "optimal" else 1), (k, s, st[k, s], ws)
            if ws == "optimal":
                assert abs(obj[k, s] - wo) <= TOL * max(1.0, abs(wo)), (k, s, obj[k, s], wo)
                assert dual[k, s] == obj[k, s]
        if first_inf is None:
            seen.add("opt")
            assert typ[k] == 0
            mean = sum(o for _, o in want) / net.S
            assert abs(obj_mean[k] - mean) <= TOL * max(1.0, abs(mean))
            # tight at y-bar
            v = _cut_at(rhs[k], rows[k], keys, y)
            assert abs(v - mean) <= 1e-9 * max(1.0, abs(mean)), (v, mean)
            # valid at other matchings: RHS + coef.y >= mean_s Q_s(y)
            for _ in range(2):
                y2 = _full_matching(net, rng, 0.9)
                q2 = [so.dual_lp(net, y2, s)[:2] for s in range(net.S)]
                if all(w == "optimal" for w, _ in q2):
                    m2 = sum(o for _, o in q2) / net.S
                    # (validity against HiGHS's objective at another matching: its LP tolerances, 1e-7)
                    assert _cut_at(rhs[k], rows[k], keys, y2) >= m2 - 1e-7 * max(1.0, abs(m2))
        else:
            seen.add("feas")
            assert typ[k] == 1
            # the ray cuts y-bar off
            assert _cut_at(rhs[k], rows[k], keys, y) < 0
            # and keeps matchings that are feasible for that scenario
            for _ in range(3):
                y2 = _full_matching(net, rng, 1.0)
                if so.dual_lp(net, y2, first_inf)[0] == "optimal":
                    assert _cut_at(rhs[k], rows[k], keys, y2) >= -1e-9
    eng.close()
    if zl:
        assert "opt" in seen            # optimality cuts exercised
    else:
        assert "feas" in seen           # feasibility rays exercised


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,zl,n_paths,sample", [("C4", 1, True, 3, 16), ("C4", 2, False, 3, 16),
                                                        ("C5", 1, True, 2, 6), ("C5", 2, False, 2, 6)])
def test_subproblem_at_benchmark_scenario_counts(cfg, seed, zl, n_paths, sample):
    """BASELINE configs[3] / [4] scenario counts (S = 256 on C4, 512 on C5).  Every scenario
    runs on the device and the reduce runs over all S (grb.cpp:174-351: 1/S-weighted sum, or
    the first infeasible scenario's ray); HiGHS checks a sampled subset of the scenarios plus
    the first infeasible one.  The cut's value at y-bar equals the mean of all S device
    objectives (tightness, so the 1/S reduction over every scenario is exact), and on C4 the
    first optimality cut is valid at another matching (all 256 scenario LPs of HiGHS)."""
    from sgufp_solver_amd import engine as E
    inst, path, net = _net(cfg, seed, None, zl)
    S = net.S
    assert S == instance.CONFIGS[cfg].scenarios
    eng = E.Engine(path, 0, 64)
    keys = _keys(eng)
    rng = np.random.default_rng(300 + seed)
    ys = [_full_matching(net, rng, 1.0) for _ in range(n_paths)]
    paths = [_path_of(inst, net, y) for y in ys]
    typ, rhs, rows, obj_mean = eng.subproblem(paths)
    st, obj, dual = eng.subproblem_detail(len(paths))
    eng.close()
    kinds = set()
    for k, y in enumerate(ys):
        assert (st[k] != 2).all(), f"path {k}: device error in scenarios {np.nonzero(st[k] == 2)[0][:8]}"
        inf = np.nonzero(st[k] == 1)[0]
        first_inf = int(inf[0]) if inf.size else None
        check = set(int(x) for x in rng.choice(S if first_inf is None else first_inf + 1,
                                               size=min(sample, S if first_inf is None else first_inf + 1),
                                               replace=False))
        if first_inf is not None:
            check.add(first_inf)
        for s in sorted(check):
            ws, wo = so.dual_lp(net, y, s)[:2]
            assert st[k, s] == (0 if ws == "optimal" else 1), (k, s, st[k, s], ws)
            if ws == "optimal":
                assert abs(obj[k, s] - wo) <= TOL * max(1.0, abs(wo)), (k, s, obj[k, s], wo)
                assert dual[k, s] == obj[k, s]
        if first_inf is None:
            kinds.add("opt")
            assert typ[k] == 0
            mean = float(np.sum(obj[k])) / S
            assert abs(obj_mean[k] - mean) <= TOL * max(1.0, abs(mean))
            v = _cut_at(rhs[k], rows[k], keys, y)
            assert abs(v - mean) <= 1e-9 * max(1.0, abs(mean)), (v, mean)
            if cfg == "C4" and "valid" not in kinds:     # one path: 256 HiGHS LPs (~25 s)
                kinds.add("valid")
                y2 = _full_matching(net, rng, 0.9)
                q2 = [so.dual_lp(net, y2, s)[:2] for s in range(S)]
                if all(w == "optimal" for w, _ in q2):
                    m2 = sum(o for _, o in q2) / S
                    assert _cut_at(rhs[k], rows[k], keys, y2) >= m2 - 1e-7 * max(1.0, abs(m2))
        else:
            kinds.add("feas")
            assert typ[k] == 1
            assert _cut_at(rhs[k], rows[k], keys, y) < 0
    assert ("opt" in kinds) if zl else ("feas" in kinds)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S,n_paths", [("C3", 1, 8, 8), ("C3", 2, 8, 8), ("C5", 1, 2, 4)])
def test_warm_bellman_ford_matches_cold(cfg, seed, S, n_paths, tmp_path):
    """The warm-started Bellman-Ford after each augmentation (invalidate_subtrees) must
    reach the labels a cold Bellman-Ford reaches.  The verify build (lib_verify,
    -DSGUFP_SUB_VERIFY) re-runs every warm Bellman-Ford cold and turns any difference into
    kSubError; its results must be identical to the production library's."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    helper = os.path.join(here, "tests", "helpers", "sub_run.py")
    vlib = os.path.join(here, "sgufp_solver_amd", "lib_verify", "libsgufp_hip.so")
    assert os.path.exists(vlib), "verify build missing: run __graft_entry__.build()"
    res = {}
    for name, lib in (("prod", None), ("verify", vlib)):
        env = dict(os.environ)
        env.pop("SGUFP_LIB_PATH", None)
        if lib:
            env["SGUFP_LIB_PATH"] = lib
        out = str(tmp_path / f"{name}.npz")
        subprocess.run([sys.executable, helper, cfg, str(seed), str(S), str(n_paths), out], env=env,
                       check=True, timeout=240)
        res[name] = np.load(out)
    assert str(res["verify"]["lib"]).endswith("lib_verify/libsgufp_hip.so")
    a, b = res["prod"], res["verify"]
    assert (b["st"] != 2).all(), "a warm Bellman-Ford disagreed with the cold one (or another error)"
    assert (a["st"] == 0).any()
    for k in ("typ", "st"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("rhs", "rows", "obj_mean", "obj", "dual"):
        np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S,n_paths", [("C3", 3, 16, 8), ("C5", 3, 2, 4)])
def test_kernel_variants_agree(cfg, seed, S, n_paths, tmp_path):
    """Launches without lower bounds run the 32-bit-key kernel with 12-byte chain records and
    predecessors from the register groups (launch_subproblem).  The same algorithm with 64-bit
    keys and 16-byte records (SGUFP_SUB_KEY64=1) and with the predecessors from the LDS chain
    records (SGUFP_SUB_PREDS_LDS=1) must give bit-identical results: same augmenting paths
    (the smallest tight arc code wins in every width), same duals, same cut rows."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    helper = os.path.join(here, "tests", "helpers", "sub_run.py")
    res = {}
    for name, extra in (("default", {}), ("key64", {"SGUFP_SUB_KEY64": "1"}),
                        ("preds_lds", {"SGUFP_SUB_PREDS_LDS": "1"})):
        env = dict(os.environ)
        env.pop("SGUFP_LIB_PATH", None)
        env.update(extra)
        out = str(tmp_path / f"{name}.npz")
        subprocess.run([sys.executable, helper, cfg, str(seed), str(S), str(n_paths), out], env=env,
                       check=True, timeout=240)
        res[name] = np.load(out)
    a = res["default"]
    assert (a["st"] == 0).all()
    for name in ("key64", "preds_lds"):
        b = res[name]
        for k in ("typ", "st"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=name)
        for k in ("rhs", "rows", "obj_mean", "obj", "dual"):
            np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64), err_msg=f"{name}: {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S,n_paths", [("C3", 4, 8, 12), ("C4", 1, 256, 4), ("C5", 4, 2, 4)])
@pytest.mark.parametrize("lib", ["prod", "verify"])
def test_warm_start_matches_cold(cfg, seed, S, n_paths, lib, tmp_path):
    """Warm-started subproblems (sgufp_subproblem_warm; the B&B's refinement loops use them):
    neighbours of solved paths -- the decisions of their last DD layers redrawn, as the exact
    leaves the B&B solves one after another differ -- start from the stored optimal flow and
    potentials and repair the imbalance.  Every scenario's status and objective must equal
    the cold solve's exactly (integral data), the dual objective must equal the primal (the
    kernel's certificate), the cut must be tight at its path, and the repair must take fewer
    augmenting paths than the cold solve.  The verify build re-solves every repaired scenario
    cold inside the kernel and flags any objective difference as an error."""
    import subprocess
    import sys
    from sgufp_solver_amd import engine as E
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    helper = os.path.join(here, "tests", "helpers", "sub_run.py")
    env = dict(os.environ)
    env.pop("SGUFP_LIB_PATH", None)
    if lib == "verify":
        env["SGUFP_LIB_PATH"] = os.path.join(here, "sgufp_solver_amd", "lib_verify", "libsgufp_hip.so")
    out = str(tmp_path / "warm.npz")
    subprocess.run([sys.executable, helper, cfg, str(seed), str(S), str(n_paths), out, "warm"], env=env, check=True,
                   timeout=240)
    r = np.load(out)
    assert (r["seed_st"] == 0).all()
    assert (r["st"] == 0).all(), f"warm statuses {np.unique(r['st'])} (2 = error / verify mismatch)"
    assert (r["cold_st"] == 0).all()
    np.testing.assert_array_equal(r["obj"], r["cold_obj"])
    np.testing.assert_array_equal(r["dual"], r["obj"])
    assert (r["typ"] == 0).all()
    np.testing.assert_array_equal(r["obj_mean"].view(np.uint64), r["cold_obj_mean"].view(np.uint64))
    aug, cold = r["warm_aug"], r["cold_aug"]
    if lib == "prod":
        assert (aug[:-1] >= 0).all(), "a warm start fell back to the cold solve"
        assert aug[:-1].mean() < 0.5 * cold[:-1].mean(), (aug.mean(), cold.mean())
    # the warm cut is tight at its path (RHS + coef . y-bar == mean objective)
    inst, path, net = _net(cfg, seed, S, True)
    eng = E.Engine(path, 0, 8)
    keys = _keys(eng)
    eng.close()
    for k in range(n_paths):
        y = so.ybar_of_path(net, [int(x) for x in r["paths"][k]])
        v = _cut_at(r["rhs"][k], r["rows"][k], keys, y)
        assert abs(v - r["obj_mean"][k]) <= 1e-9 * max(1.0, abs(r["obj_mean"][k])), (k, v, r["obj_mean"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,seed,S,n_paths", [("C3", 4, 16, 12), ("C4", 1, 256, 4), ("C5", 4, 16, 4)])
@pytest.mark.parametrize("lib", ["prod", "verify"])
def test_warm_start_with_lower_bounds(cfg, seed, S, n_paths, lib, tmp_path):
    """Warm starts on the generator's instances with their sink-arc lower bounds kept (64-bit
    Bellman-Ford keys, big-M costs in the cold solve; round-5 VERDICT item 2).  The repair keeps
    every flow within [max l, min u]; a scenario the new path makes infeasible cannot be
    repaired and falls back to the cold SSP, whose big-M potentials give the ray.  So per
    scenario the status equals the cold solve's, the objective of every feasible scenario equals
    the cold one exactly, dual == primal, a feasibility cut (the first infeasible scenario's
    ray, found by the same cold SSP) equals the cold cut bit for bit, and no feasible scenario
    whose source state was stored falls back."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    helper = os.path.join(here, "tests", "helpers", "sub_run.py")
    env = dict(os.environ)
    env.pop("SGUFP_LIB_PATH", None)
    if lib == "verify":
        env["SGUFP_LIB_PATH"] = os.path.join(here, "sgufp_solver_amd", "lib_verify", "libsgufp_hip.so")
    out = str(tmp_path / "warmgen.npz")
    subprocess.run([sys.executable, helper, cfg, str(seed), str(S), str(n_paths), out, "warmgen"], env=env,
                   check=True, timeout=240)
    r = np.load(out)
    st, cst = r["st"].reshape(n_paths, S), r["cold_st"].reshape(n_paths, S)
    assert (st != 2).all() and (cst != 2).all(), "error / verify mismatch"
    # per path up to its first infeasible scenario (the later ones may stop unsolved: status 3,
    # the reference returns at the first infeasible one, grb.cpp:284-351)
    for k in range(n_paths):
        inf = np.nonzero(cst[k] == 1)[0]
        upto = int(inf[0]) + 1 if inf.size else S
        np.testing.assert_array_equal(st[k, :upto], cst[k, :upto])
        assert (cst[k, :upto] != 3).all() and (st[k, :upto] != 3).all()
    st, cst = st.reshape(-1), cst.reshape(-1)
    feas = (cst == 0) & (st == 0)
    assert feas.any()
    if cfg != "C5":   # (C5's random matchings are mostly feasible: its 8-wave kernel is the point there)
        assert (~feas).any(), "the case should hold feasible and infeasible scenarios"
    obj, cobj, dual = r["obj"].reshape(-1), r["cold_obj"].reshape(-1), r["dual"].reshape(-1)
    np.testing.assert_array_equal(obj[feas], cobj[feas])
    np.testing.assert_array_equal(dual[feas], obj[feas])
    np.testing.assert_array_equal(r["typ"], r["cold_typ"])
    for k in range(n_paths):
        if r["typ"][k] == 0:
            assert r["obj_mean"][k] == r["cold_obj_mean"][k]
        else:
            assert r["rhs"][k] == r["cold_rhs"][k]
            np.testing.assert_array_equal(r["rows"][k].view(np.uint64), r["cold_rows"][k].view(np.uint64))
    if lib == "prod":
        aug = r["warm_aug"].reshape(n_paths, S)
        ok = r["seed_st"].reshape(n_paths, S) == 0     # the source slot stored a state
        sel = feas.reshape(n_paths, S) & ok
        sel[-1] = False                                # the unrelated path (far donor) may start cold
        assert sel.any()
        assert (aug[sel] >= 0).all(), "a feasible scenario with a stored source state fell back"
        cold = r["cold_aug"].reshape(n_paths, S)
        assert aug[sel].mean() < 0.5 * cold[sel].mean(), (aug[sel].mean(), cold[sel].mean())
