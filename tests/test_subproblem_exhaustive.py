"""Scenario subproblem kernels (k_sub_paths, k_sub_scenario, k_sub_reduce) against an exact
integer reference, exhaustively.

Every matching of a tiny network is enumerated, turned into its DD path and solved in one
sgufp_subproblem call; tests/helpers/exact_flow.py gives Q[y, s] for all of them (Python ints).
Then, with no tolerance: statuses and objectives equal the reference's, dual == primal, an
optimality cut is tight at its own matching and lies on or above the mean of Q at EVERY
matching whose scenarios are all feasible, a feasibility cut is negative at its own matching
and non-negative at EVERY matching feasible in its scenario.  That is what the kernel's own
certificate (dual objective == primal objective) does not prove: a dual with the right
objective that is not feasible gives a cut tight at y-bar and invalid elsewhere.

Scenario counts are 1, 2 and 4, so that the 1/S of an optimality cut is exact in binary64
and every comparison is one of exactly representable numbers; the one S = 3 case uses the
derived bound (total_layers + 2) * 2^-52 * (|rhs| + sum |row|).

Each case records the reference's (optimality paths, feasibility paths, histogram of the first
infeasible scenario, kinds of that scenario's infeasibility) from a CPU run; the counts are
asserted, so a change of the data cannot silently empty a class.  Kinds, by construction from
the chains: (i) a chain fixed at 0 (or a source -> sink arc) with l > 0 or u < 0, (ii) a
complete chain with max l > min u and no chain of kind (i), (iii) neither: a lower bound that
conservation cannot meet (the unmet big-M bound after the successive shortest paths).

Conventions.  Every node without in-arcs is a free supply and every node without out-arcs a
free demand, whatever its id (the reference's dual pins alpha[0] and alpha[n-1] only, but the
A1 / A2 rows of grb.cpp hold no alpha of such a node at all); node 0 is a source and n - 1 a
sink in every network here.  An arc source -> sink carries nothing (the reference's emptied
A4).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import subproblem_oracle as so
from tests.helpers import exact_flow as xf
from tests.helpers import sub_families as fam
from tests.helpers.matchings import all_matchings
from tests.test_subproblem import _keys, _path_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_CAPACITY = -4


# ------------------------------------------------------------------------------ reference
def _write(inst):
    from sgufp_solver_amd import engine as E
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_subx_"), "net.txt")
    inst.write(path)
    _, la, _ = E.probe_network(path)
    return path, so.from_instance(inst, la)


def _kind(net, C, s):
    lb, ub = net.lb[:, s], net.ub[:, s]
    if any(lb[a] > 0 or ub[a] < 0 for a in C.a4):
        return 0
    crossed = False
    for t, h, arcs in C.chains:
        L, U = max(int(lb[a]) for a in arcs), min(int(ub[a]) for a in arcs)
        if (t < 0 or h < 0) and (L > 0 or U < 0):
            return 0
        crossed |= t >= 0 and h >= 0 and L > U
    return 1 if crossed else 2


def _reference(net, ys):
    """Q[y][s] (None: infeasible) and the counts (opt paths, feas paths, histogram, kinds)."""
    Q = xf.q_table(net, ys)
    S = net.S
    hist, kinds, n_opt = [0] * S, [0, 0, 0], 0
    for y, row in zip(ys, Q):
        fi = next((s for s, q in enumerate(row) if q is None), None)
        if fi is None:
            n_opt += 1
        else:
            hist[fi] += 1
            kinds[_kind(net, xf.Contraction(net, y), fi)] += 1
    return Q, (n_opt, len(ys) - n_opt, hist, kinds)


class Result:
    def __init__(self, typ, rhs, rows, obj_mean, st, obj, dual):
        self.typ, self.rhs, self.rows, self.obj_mean, self.st, self.obj, self.dual = typ, rhs, rows, obj_mean, st, obj, dual


def _run(path, paths):
    from sgufp_solver_amd import engine as E
    eng = E.Engine(path, 0, max(len(paths), 32))
    try:
        keys = _keys(eng)
        layers = eng.info.total_layers
        out = eng.subproblem(paths)
        return Result(*out, *eng.subproblem_detail(len(paths))), keys, layers
    finally:
        eng.close()


def _check(net, ys, Q, res, keys, layers, sel=None):
    """The assertions of the module docstring for the paths of matchings ys[sel] (all of them by
    default; res holds one entry per selected matching), cut validity over every matching of ys."""
    S = net.S
    sel = list(range(len(ys))) if sel is None else list(sel)
    n_slots = len(keys)
    slot = {k: i for i, k in enumerate(keys)}
    Y = np.zeros((len(ys), n_slots))
    for j, y in enumerate(ys):
        for t in y:
            Y[j, slot[t]] = 1.0
    all_ok = np.array([all(q is not None for q in row) for row in Q])
    qsum = np.array([float(sum(row)) if ok else 0.0 for row, ok in zip(Q, all_ok)])   # ints below 2^53
    exact = S in (1, 2, 4)
    assert (res.typ != -1).all(), f"paths with type -1: {np.nonzero(res.typ == -1)[0][:8]}"
    assert res.rows.shape[1] == n_slots + 1 and not res.rows[:, -1].any()
    cut = res.rhs[:, None] + res.rows[:, :n_slots] @ Y.T          # [path, matching]
    tol = (layers + 2) * 2.0 ** -52 * (np.abs(res.rhs) + np.abs(res.rows).sum(axis=1))
    for k, j in enumerate(sel):
        row = Q[j]
        fi = next((s for s, q in enumerate(row) if q is None), None)
        for s in range(S):
            want = 0 if row[s] is not None else 1
            if fi is not None and s > fi:
                assert res.st[k, s] in (3, want), (j, s, res.st[k, s])
                continue
            assert res.st[k, s] == want, (j, s, res.st[k], row)
            if want == 0:
                assert res.obj[k, s] == float(row[s]), (j, s, res.obj[k, s], row[s])
                assert res.dual[k, s] == res.obj[k, s], (j, s)
        if fi is None:
            assert res.typ[k] == 0, (j, res.typ[k])
            if exact:
                assert res.obj_mean[k] == qsum[j] / S, (j, res.obj_mean[k], qsum[j])
                assert cut[k, j] == res.obj_mean[k], (j, cut[k, j], res.obj_mean[k])
                bad = np.nonzero(all_ok & (cut[k] < qsum / S))[0]
            else:
                assert abs(res.obj_mean[k] - qsum[j] / S) <= (S + 2) * 2.0 ** -52 * sum(abs(q) for q in row) / S
                assert abs(cut[k, j] - res.obj_mean[k]) <= tol[k], (j, cut[k, j], res.obj_mean[k])
                bad = np.nonzero(all_ok & (cut[k] < qsum / S - tol[k]))[0]
            assert bad.size == 0, f"optimality cut of matching {j} invalid at matchings {bad[:8]}"
        else:
            assert res.typ[k] == 1, (j, res.typ[k])
            assert cut[k, j] < 0, (j, cut[k, j])
            feas = np.array([r[fi] is not None for r in Q])
            bad = np.nonzero(feas & (cut[k] < 0))[0]
            assert bad.size == 0, f"feasibility cut of matching {j} (scenario {fi}) cuts off matchings {bad[:8]}"


def _case(inst, counts, ys=None):
    path, net = _write(inst)
    ys = all_matchings(inst) if ys is None else ys
    Q, got = _reference(net, ys)
    print("reference counts:", got)
    assert got == counts, got
    res, keys, layers = _run(path, [_path_of(inst, net, y) for y in ys])
    _check(net, ys, Q, res, keys, layers)
    return path, net, ys, Q, res


# --------------------------------------------------------------------- exhaustive families
# (config, seed, S, family): (optimality paths, feasibility paths, first-infeasible histogram,
# [kind (i), kind (ii), kind (iii)]) of the exact reference, from a CPU run
FAMILY_CASES = {
    ("T0", 2, 2, "gen_lb"): (81, 0, [0, 0], [0, 0, 0]),
    ("T2", 2, 4, "plain"): (864, 0, [0, 0, 0, 0], [0, 0, 0]),
    ("T2", 2, 4, "gen_lb"): (61, 803, [720, 52, 31, 0], [491, 0, 312]),
    ("T2", 2, 3, "gen_lb"): (92, 772, [576, 144, 52], [180, 0, 592]),
    ("T2", 2, 2, "zero_cap"): (864, 0, [0, 0], [0, 0, 0]),
    ("T2", 2, 2, "inner_lb"): (18, 846, [738, 108], [684, 0, 162]),
    ("T2", 2, 2, "fixed"): (28, 836, [738, 98], [18, 0, 818]),
    ("T2", 2, 2, "crossed"): (0, 864, [0, 864], [0, 864, 0]),
    ("T2", 2, 2, "crossed_split"): (0, 864, [0, 864], [648, 216, 0]),
    ("T2", 2, 2, "broken_lb"): (126, 738, [0, 738], [576, 0, 162]),
    ("T2", 2, 2, "neg_rewards"): (92, 772, [772, 0], [540, 0, 232]),
    ("T2", 2, 1, "zero_rewards"): (366, 498, [498], [378, 0, 120]),
    ("T2", 2, 4, "ties"): (864, 0, [0, 0, 0, 0], [0, 0, 0]),
    ("T1", 1, 2, "crossed"): (0, 648, [0, 648], [576, 72, 0]),
    ("T1", 1, 2, "crossed_split"): (0, 648, [0, 648], [576, 72, 0]),
    ("T1", 1, 2, "broken_lb"): (72, 576, [0, 576], [576, 0, 0]),
}


@pytest.mark.parametrize("cfg,seed,S,family", list(FAMILY_CASES), ids=["-".join(map(str, c)) for c in FAMILY_CASES])
def test_every_matching_against_the_exact_reference(native_lib, cfg, seed, S, family):
    _case(fam.make(cfg, seed, S, family), FAMILY_CASES[(cfg, seed, S, family)])


def test_coverage_of_the_families_that_keep_lower_bounds():
    """Together: >= 50 optimality-cut paths, >= 50 feasibility-cut paths, >= 10 feasibility paths
    whose first infeasible scenario is not scenario 0, every kind of ray."""
    keep = [c for k, c in FAMILY_CASES.items() if k[3] not in ("plain", "zero_cap", "ties")]
    assert sum(c[0] for c in keep) >= 50 and sum(c[1] for c in keep) >= 50
    assert sum(sum(c[2][1:]) for c in keep) >= 10
    assert all(sum(c[3][i] for c in keep) > 0 for i in range(3))


# ------------------------------------------------------------- gates and field boundaries
def _plain_t2(S=1):
    return fam.make("T2", 2, S, "plain")


def _lone_arc(inst):
    """An arc between two nodes outside V-bar: a complete chain of its own under every matching."""
    vb = set(int(v) for v in inst.vbar)
    return next(a for a in range(inst.m) if int(inst.tails[a]) not in vb and int(inst.heads[a]) not in vb)


@pytest.mark.parametrize("total,sign", [((1 << 18) - 1, 1), ((1 << 18) - 1, -1), (1 << 18, 1), (1 << 18, -1)])
def test_reward_sum_at_the_32_bit_key_gate(native_lib, total, sign):
    """sum |r| = 2^18 - 1 still takes the 32-bit keys and the 8-byte records, 2^18 the 64-bit ones;
    one single-arc chain carries most of the sum in either sign (the signed 19-bit R field)."""
    inst = _plain_t2()
    a = _lone_arc(inst)
    rest = int(np.abs(inst.reward[:, 0]).sum() - abs(int(inst.reward[a, 0])))
    inst.reward[a, :] = sign * (total - rest)
    assert int(np.abs(inst.reward[:, 0]).sum()) == total
    _case(inst, (864, 0, [0], [0, 0, 0]))


@pytest.mark.parametrize("umax", [2047, 2048, 32767])
def test_upper_bounds_at_the_field_widths(native_lib, umax):
    """11-bit U and x fields of the 8-byte records (2047: last value they hold; 2048: 64-bit
    keys, 16-bit fields) and the 16-bit fields' last value."""
    inst = _plain_t2(2)
    rng = np.random.default_rng(umax)
    inst.ub[:] = rng.integers(umax // 2, umax + 1, size=inst.ub.shape)
    inst.ub[rng.integers(0, inst.m, size=4), rng.integers(0, 2, size=4)] = umax
    _case(inst, (864, 0, [0, 0], [0, 0, 0]))


def _rejected(inst, what, call="subproblem"):
    from sgufp_solver_amd import engine as E
    path, net = _write(inst)
    eng = E.Engine(path, 0, 32)
    try:
        paths = [[-1] * len(net.layer_arcs)]
        with pytest.raises(RuntimeError) as ei:
            getattr(eng, call)(paths)
        assert f"({ERR_CAPACITY})" in str(ei.value) and what in str(ei.value), str(ei.value)
    finally:
        eng.close()


def test_unrepresentable_inputs_are_rejected_with_a_capacity_error(native_lib):
    """Whatever the kernels cannot represent fails in sub_init, before anything is launched, with
    SGUFP_ERR_CAPACITY and the limit's name -- never a wrong number, never SGUFP_ERR_HIP."""
    inst = _plain_t2()
    inst.ub[3, 0] = 32768
    _rejected(inst, "arc bounds outside 16 bits")
    inst = _plain_t2()
    inst.lb[3, 0] = -1
    _rejected(inst, "negative lower bound")
    _rejected(inst, "negative lower bound", call="subproblem_flows")
    cyc = fam.network(6, [(0, 1), (1, 2), (2, 3), (3, 1), (2, 4), (4, 5)], 0, 5, 3, [4], 1)
    _rejected(cyc, "directed cycle")


def _cost_bound(inst):
    return 2 * (1 + 2 * int(np.abs(inst.reward[:, 0]).sum()) * (int(inst.ub.max()) + 1))


def _headroom(extra):
    """T2 seed 2 with the generator's lower bounds, u ~ 3e4 and |r| ~ 7e5, sum |r| set so that
    (n + 2) * cost_bound is the largest value below 2^45 (extra = 0) or the first one past it."""
    inst = fam.make("T2", 2, 2, "gen_lb")
    rng = np.random.default_rng(45)
    inst.ub[:] = rng.integers(20000, 30001, size=inst.ub.shape)
    inst.ub[0, 0] = 30000
    r = rng.integers(-300000, 760000, size=inst.m)
    umax = 30000
    sr_max = ((((1 << 45) - 1) // (inst.n + 2)) // 2 - 1) // (2 * (umax + 1))
    a = _lone_arc(inst)
    r[a] = 0
    r[a] = sr_max + extra - int(np.abs(r).sum())
    assert r[a] > 0
    inst.reward[:] = r[:, None].astype(np.int32)
    return inst


def test_64_bit_key_headroom(native_lib):
    """64-bit keys are (cost << 16) | hops with inf = 2^61, so path costs must stay below 2^45; a
    path has at most n + 1 residual arcs of cost at most cost_bound = 2 + 4 sum|r| (max u + 1).
    The last instance inside (n + 2) * cost_bound < 2^45 equals the exact reference (objectives
    ~ 5e11, far past what an LP solver's tolerance resolves); the first one outside is rejected."""
    inside, outside = _headroom(0), _headroom(1)
    assert (inside.n + 2) * _cost_bound(inside) < 1 << 45 <= (outside.n + 2) * _cost_bound(outside)
    _case(inside, (92, 772, [772, 0], [540, 0, 232]))
    _rejected(outside, "cost_bound reaches 2^45")


def test_negative_upper_bound_is_infeasible_on_complete_and_broken_chains(native_lib):
    """u = -1 with l = 0 on one arc: its chain is infeasible whether the matching completes it
    (kind (ii), l > u) or breaks it (kind (i): a chain fixed at 0 with min u < 0)."""
    counts = (0, 864, [0, 864], [576, 288, 0])
    assert counts[3][0] > 0 and counts[3][1] > 0
    _case(fam.neg_ub("T2", 2, 2), counts)


@pytest.mark.parametrize("n", [2045, 2046, 2047])
def test_node_count_at_the_id_gates(native_lib, n):
    """A tiny network padded with isolated nodes, its inner nodes on the highest ids.  2045: the
    last size with 11-bit ids (0x7FF is "none") and 32-bit keys; 2046: 64-bit keys, warm starts and
    flows still available; 2047: neither -- sgufp_subproblem_flows answers SGUFP_ERR_CAPACITY."""
    from sgufp_solver_amd import engine as E
    inst = fam.padded(fam.make("T0", 2, 2, "plain"), n)
    path, net, ys, Q, res = _case(inst, (81, 0, [0, 0], [0, 0, 0]))
    paths = [_path_of(inst, net, y) for y in ys]
    eng = E.Engine(path, 0, 128)
    try:
        if n <= 2046:
            warm = eng.subproblem(paths, [-1] * len(paths), list(range(len(paths))))
            assert all(a.tobytes() == b.tobytes() for a, b in zip(warm, (res.typ, res.rhs, res.rows, res.obj_mean)))
            st, obj, frew, x, mean = eng.subproblem_flows(paths)
            assert (st == 0).all() and (obj == res.obj).all() and (frew == obj).all()
        else:
            with pytest.raises(RuntimeError) as ei:
                eng.subproblem_flows(paths)
            assert f"({ERR_CAPACITY})" in str(ei.value) and "2048 network nodes" in str(ei.value)
    finally:
        eng.close()


def _line_matchings(K, rng):
    """Matchings of the line network: everything matched, broken at the first, a middle and the
    last V-bar node, and random break patterns (for cut validity)."""
    full = {(v - 1, v, v + 1): 1 for v in range(1, K + 1)}
    ys = [full]
    for cutv in (1, K // 2, K):
        ys.append({k: 1 for k in full if k[1] != cutv})
    for _ in range(40):
        ys.append({k: 1 for k in full if rng.random() < 0.9})
    return ys


@pytest.mark.parametrize("lb_arc", [None, 40])
def test_chain_of_64_arcs(native_lib, lb_arc):
    """K = 63 V-bar nodes in a row: the full matching is one complete chain of kMaxChain = 64 arcs,
    worth max(0, sum R) * min u without a lower bound."""
    inst = fam.line(63, lb_arc)
    ys = _line_matchings(63, np.random.default_rng(63))
    counts = (1, 43, [0, 43], [43, 0, 0]) if lb_arc is not None else (44, 0, [0, 0], [0, 0, 0])
    path, net, ys, Q, res = _case(inst, counts, ys)
    R, U = int(inst.reward[:, 0].sum()), [int(inst.ub[:, s].min()) for s in range(2)]
    assert Q[0][0] == max(0, R) * U[0]
    assert Q[0][1] == (max(0, R) * U[1] if lb_arc is None or R >= 0 else R)


@pytest.mark.parametrize("lb_arc", [None, 40])
def test_chain_of_65_arcs_is_an_error_not_a_cut(native_lib, lb_arc):
    """K = 64: the full matching's chain has 65 arcs, over kMaxChain; that path alone comes back
    as type -1 with a zero row.  Broken at the first or the last node a chain of 64 arcs is left,
    which is solved like any other."""
    inst = fam.line(64, lb_arc)
    path, net = _write(inst)
    ys = _line_matchings(64, np.random.default_rng(64))
    ys = [y for y in ys if len(y) < 64 or y is ys[0]]
    paths = [_path_of(inst, net, y) for y in ys]
    res, keys, layers = _run(path, paths)
    assert res.typ[0] == -1 and res.rhs[0] == 0 and not res.rows[0].any() and res.obj_mean[0] == 0
    Q, counts = _reference(net, ys[1:])
    assert counts[0] + counts[1] == len(ys) - 1 and (counts[1] > 0) == (lb_arc is not None)
    rest = Result(*(a[1:] for a in (res.typ, res.rhs, res.rows, res.obj_mean, res.st, res.obj, res.dual)))
    _check(net, ys[1:], Q, rest, keys, layers)


# ------------------------------------------------------------ topologies the generator never makes
TOPOLOGIES = {
    # a second node without in-arcs and a second node without out-arcs that is not n - 1 (zlist)
    "two_sources_two_sinks": (lambda: fam.two_sources_two_sinks(2), (22, 27, [9, 18], [18, 0, 9])),
    # V-bar nodes with in-degree 1 / out-degree 4 and in-degree 4 / out-degree 1
    "fans": (lambda: fam.fans(2), (12, 13, [0, 13], [5, 0, 8])),
    # an arc source -> sink: carries nothing; with l > 0 (last scenario) the scenario is infeasible
    "direct_arc": (lambda: fam.direct_arc(2, 0), (864, 0, [0, 0], [0, 0, 0])),
    "direct_arc_lb": (lambda: fam.direct_arc(2, 2), (0, 864, [0, 864], [864, 0, 0])),
}


@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_topologies_the_generator_never_makes(native_lib, name):
    make, counts = TOPOLOGIES[name]
    _case(make(), counts)


# ------------------------------------------------------------------ bad paths beside good ones
def test_invalid_paths_do_not_disturb_their_neighbours(native_lib):
    """One launch mixes valid paths with a decision that is not an out-arc of its node, two in-arcs
    choosing one out-arc and a decision >= m: those come back as type -1, the valid neighbours
    exactly as in a launch without them (cut bit for bit; per-scenario detail up to the first
    infeasible scenario -- which later scenarios stop unsolved depends on timing)."""
    inst = fam.make("T2", 2, 2, "gen_lb")
    path, net = _write(inst)
    ys = all_matchings(inst)[::37]
    good = [_path_of(inst, net, y) for y in ys]
    la = [int(a) for a in net.layer_arcs]
    T, H = [int(t) for t in inst.tails], [int(h) for h in inst.heads]
    full = good[-1]
    not_out = list(full)
    not_out[0] = next(b for b in range(inst.m) if T[b] != H[la[0]])
    q = next(v for v in net.vbar if len(net.in_arcs(int(v))) >= 2 and net.out_arcs(int(v)))
    l0, l1 = [l for l, a in enumerate(la) if H[a] == int(q)][:2]
    twice = [-1] * len(la)
    twice[l0] = twice[l1] = net.out_arcs(int(q))[0]
    too_big = list(full)
    too_big[-1] = inst.m
    bad = [not_out, twice, too_big]
    mixed, where = [], []
    for k, p in enumerate(good):
        where.append(len(mixed))
        mixed.append(p)
        if k < len(bad):
            mixed.append(bad[k])
    alone, keys, layers = _run(path, good)
    both, _, _ = _run(path, mixed)
    Q, _ = _reference(net, ys)
    _check(net, ys, Q, alone, keys, layers)
    bad_at = [i for i in range(len(mixed)) if i not in where]
    assert (both.typ[bad_at] == -1).all() and not both.rows[bad_at].any() and not both.rhs[bad_at].any()
    for name in ("typ", "rhs", "rows", "obj_mean"):
        assert getattr(both, name)[where].tobytes() == getattr(alone, name).tobytes(), name
    for k, row in enumerate(Q):
        upto = next((s + 1 for s, v in enumerate(row) if v is None), net.S)
        for name in ("st", "obj", "dual"):
            assert getattr(both, name)[where[k], :upto].tobytes() == getattr(alone, name)[k, :upto].tobytes(), (name, k)


# ------------------------------------------------------------------ every instantiation, same inputs
ROUTE_CASES = [("T2", 2, 4, "plain"), ("T2", 2, 4, "gen_lb")]


@pytest.mark.parametrize("cfg,seed,S,family", ROUTE_CASES, ids=[c[3] for c in ROUTE_CASES])
@pytest.mark.parametrize("knob", ["SGUFP_SUB_KEY64=1", "SGUFP_SUB_PREDS_LDS=1", "SGUFP_SUB_WAVES=8"])
def test_kernel_variants_against_the_exact_reference(native_lib, monkeypatch, cfg, seed, S, family, knob):
    """64-bit keys forced on a launch that would take the 32-bit ones, the predecessors from the
    LDS chain records (the non-ALLREG kernels), and the eight-wave kernel of the large networks
    (32-bit costs in registers; eight waves share a handful of chains here): the same assertions,
    and the same statuses, objectives and cuts as the default kernels bit for bit."""
    inst = fam.make(cfg, seed, S, family)
    path, net, ys, Q, base = _case(inst, FAMILY_CASES[(cfg, seed, S, family)])
    monkeypatch.setenv(*knob.split("="))
    res, keys, layers = _run(path, [_path_of(inst, net, y) for y in ys])
    _check(net, ys, Q, res, keys, layers)
    for name in ("typ", "rhs", "rows", "obj_mean"):
        assert getattr(res, name).tobytes() == getattr(base, name).tobytes(), name


def test_eight_wave_kernel_at_the_32_bit_cost_gate(native_lib, monkeypatch):
    """The eight-wave kernel keeps costs (big-M included) in 32-bit registers; its gate is
    cost_bound < 2^30.  Lower bounds present and sum |r| the largest that stays under the gate."""
    inst = fam.make("T2", 2, 2, "gen_lb")
    rng = np.random.default_rng(30)
    r = rng.integers(-80000, 250000, size=inst.m)
    sr_max = (((1 << 30) - 3) // 4) // (int(inst.ub.max()) + 1)
    a = _lone_arc(inst)
    r[a] = 0
    r[a] = sr_max - int(np.abs(r).sum())
    assert r[a] > 0
    inst.reward[:] = r[:, None].astype(np.int32)
    assert _cost_bound(inst) < 1 << 30 <= _cost_bound(inst) + 4 * (int(inst.ub.max()) + 1)
    monkeypatch.setenv("SGUFP_SUB_WAVES", "8")
    _case(inst, (92, 772, [772, 0], [540, 0, 232]))


@pytest.mark.parametrize("cfg,seed,S,family", ROUTE_CASES, ids=[c[3] for c in ROUTE_CASES])
def test_exported_flows_are_exact_optimal_flows(native_lib, cfg, seed, S, family):
    """sgufp_subproblem_flows (the WARM kernels run cold): statuses and objectives equal the
    reference's, and every optimal scenario's flow is feasible in integer arithmetic (bounds,
    conservation, coupling) and earns sum r x == objective == Q."""
    from sgufp_solver_amd import engine as E
    from tests.test_flows import _check_flow
    inst = fam.make(cfg, seed, S, family)
    path, net = _write(inst)
    ys = all_matchings(inst)
    Q, counts = _reference(net, ys)
    assert counts == FAMILY_CASES[(cfg, seed, S, family)]
    eng = E.Engine(path, 0, 1024)
    try:
        st, obj, frew, x, mean = eng.subproblem_flows([_path_of(inst, net, y) for y in ys])
    finally:
        eng.close()
    reward = np.asarray(inst.reward)[:, 0].astype(np.int64)
    for k, (y, row) in enumerate(zip(ys, Q)):
        fi = next((s for s, q in enumerate(row) if q is None), S)
        for s in range(min(fi + 1, S)):
            assert st[k, s] == (0 if row[s] is not None else 1), (k, s)
            if row[s] is None:
                assert not x[k, s].any()
                continue
            xs = x[k, s].astype(np.int64)
            _check_flow(inst, net, y, s, xs)
            assert int((reward * xs).sum()) == row[s] and obj[k, s] == frew[k, s] == float(row[s]), (k, s)


@pytest.mark.parametrize("cfg,seed,S,family", ROUTE_CASES, ids=[c[3] for c in ROUTE_CASES])
@pytest.mark.parametrize("lib", ["prod", "verify"])
def test_warm_chain_against_the_exact_reference(native_lib, tmp_path, cfg, seed, S, family, lib):
    """Warm starts in two calls (no slot may be read and written in one): the even-numbered
    matchings of the enumeration are solved cold into slots, the odd-numbered ones start from
    their predecessor's slot, which differs at one V-bar node (two where the enumeration wraps).
    Both halves satisfy the assertions of the cold kernels; the verify build re-solves every
    repaired scenario cold inside the kernel and turns a difference into an error."""
    helper = os.path.join(ROOT, "tests", "helpers", "sub_warm_chain.py")
    env = dict(os.environ)
    env.pop("SGUFP_LIB_PATH", None)
    if lib == "verify":
        env["SGUFP_LIB_PATH"] = os.path.join(ROOT, "sgufp_solver_amd", "lib_verify", "libsgufp_hip.so")
        assert os.path.exists(env["SGUFP_LIB_PATH"]), "verify build missing: run __graft_entry__.build()"
    out = str(tmp_path / "warm.npz")
    subprocess.run([sys.executable, helper, cfg, str(seed), str(S), family, out], env=env, check=True, timeout=120)
    r = np.load(out)
    assert (lib == "verify") == str(r["lib"]).endswith("lib_verify/libsgufp_hip.so")
    inst = fam.make(cfg, seed, S, family)
    path, net = _write(inst)
    ys = all_matchings(inst)
    Q, counts = _reference(net, ys)
    assert counts == FAMILY_CASES[(cfg, seed, S, family)]
    keys = [tuple(int(v) for v in k) for k in r["keys"]]
    for half, sel in (("cold", range(0, len(ys), 2)), ("warm", range(1, len(ys), 2))):
        res = Result(*(r[f"{half}_{name}"] for name in ("typ", "rhs", "rows", "obj_mean", "st", "obj", "dual")))
        _check(net, ys, Q, res, keys, int(r["layers"]), sel)
    if lib == "prod":   # (the verify build solves every repaired scenario cold afterwards and reports that)
        ok = (r["warm_st"] == 0) & (r["cold_st"][:len(r["warm_st"])] == 0)      # a stored state to start from
        assert ok.any() and (r["warm_aug"][ok] >= 0).any(), "no scenario was repaired from its predecessor's state"
