"""The exact integer reference of the scenario subproblem (tests/helpers/exact_flow.py: chains,
lower bounds as node demands, networkx network simplex on Python ints) pinned against the two LP
statements of oracle/subproblem_oracle.py (HiGHS), on every data family and hand-made topology
that tests/test_subproblem_exhaustive.py runs on the device, at magnitudes HiGHS resolves
(objectives below 1e5: 1e-6 absolute separates integers).  Same status everywhere; where optimal,
the exact objective equals the primal's and the dual's.
"""
import os
import tempfile

import numpy as np
import pytest

from oracle import subproblem_oracle as so
from tests.helpers import exact_flow as xf
from tests.helpers import sub_families as fam
from tests.helpers.matchings import all_matchings

FAMILIES = ["plain", "gen_lb", "zero_cap", "inner_lb", "fixed", "crossed", "crossed_split", "broken_lb",
            "neg_rewards", "zero_rewards", "ties"]


def _sub_net(inst):
    from sgufp_solver_amd import engine as E
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_xf_"), "net.txt")
    inst.write(path)
    _, la, _ = E.probe_network(path)
    return so.from_instance(inst, la)


def _pin(inst, sample, seed=0):
    net = _sub_net(inst)
    ys = all_matchings(inst)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(ys), size=min(sample, len(ys)), replace=False)
    seen = set()
    for k in pick:
        y = ys[int(k)]
        C = xf.Contraction(net, y)
        for s in range(net.S):
            st, obj = xf.solve(net, y, s, contraction=C)
            pst, pobj = so.primal_lp(net, y, s)
            dst, dobj, _ = so.dual_lp(net, y, s)
            assert st == pst == dst, (int(k), s, st, pst, dst)
            seen.add(st)
            if st == "optimal":
                assert isinstance(obj, int)
                assert abs(pobj - obj) <= 1e-6 and abs(dobj - obj) <= 1e-6, (int(k), s, obj, pobj, dobj)
    return seen


@pytest.mark.parametrize("family", FAMILIES)
def test_exact_reference_equals_both_lps_on_the_families(family):
    seen = _pin(fam.make("T2", 2, 2, family), 10)
    assert "optimal" in seen or family in ("crossed", "crossed_split")
    if family in ("crossed", "crossed_split", "broken_lb", "gen_lb", "inner_lb"):
        assert "infeasible" in seen


@pytest.mark.parametrize("name", ["direct", "direct_lb", "neg_ub", "two_sources_two_sinks", "fans", "line", "line_lb",
                                  "padded", "t1_crossed_split", "t1_broken_lb"])
def test_exact_reference_equals_both_lps_on_the_topologies(name):
    inst = {"direct": lambda: fam.direct_arc(2, 0), "direct_lb": lambda: fam.direct_arc(2, 2),
            "neg_ub": lambda: fam.neg_ub("T2", 2, 2), "two_sources_two_sinks": lambda: fam.two_sources_two_sinks(2),
            "fans": lambda: fam.fans(2), "line": lambda: fam.line(5), "line_lb": lambda: fam.line(5, 2),
            "padded": lambda: fam.padded(fam.make("T0", 2, 2, "gen_lb"), 40),
            "t1_crossed_split": lambda: fam.make("T1", 1, 2, "crossed_split"),
            "t1_broken_lb": lambda: fam.make("T1", 1, 2, "broken_lb")}[name]()
    seen = _pin(inst, 12)
    if name in ("direct_lb", "neg_ub", "t1_crossed_split"):
        assert "infeasible" in seen


def test_source_to_sink_arc_carries_nothing():
    """The reference empties A4 (Network.cpp:80; the 7j rows of grb.cpp:126-133 are commented out),
    so an arc source -> sink has no dual row: it adds nothing to any scenario's objective, and a
    positive lower bound on it makes the dual unbounded, i.e. the scenario infeasible."""
    base = fam.make("T2", 2, 2, "plain")
    net0, net1, net2 = _sub_net(base), _sub_net(fam.direct_arc(2, 0)), _sub_net(fam.direct_arc(2, 2))
    for y in all_matchings(base)[::97]:
        for s in range(2):
            want = xf.solve(net0, y, s)
            assert xf.solve(net1, y, s) == want
            assert xf.solve(net2, y, s) == (want if s == 0 else ("infeasible", None))
            st, obj, x = xf.solve(net1, y, s, want_flow=True)
            assert x[-1] == 0


def test_exact_reference_flow_is_feasible_and_earns_the_objective():
    inst = fam.make("T2", 2, 3, "gen_lb")
    net = _sub_net(inst)
    r = np.asarray(inst.reward)[:, 0].astype(np.int64)
    n_opt = 0
    for y in all_matchings(inst)[::29]:
        for s in range(3):
            st, obj, x = xf.solve(net, y, s, want_flow=True)
            if st != "optimal":
                continue
            n_opt += 1
            x = np.asarray(x, dtype=np.int64)
            assert int((r * x).sum()) == obj
            assert (x >= inst.lb[:, s]).all() and (x <= inst.ub[:, s]).all()
            fin = np.bincount(inst.heads, weights=x, minlength=inst.n)
            fout = np.bincount(inst.tails, weights=x, minlength=inst.n)
            assert (fin[1:-1] == fout[1:-1]).all()
    assert n_opt >= 10


def test_exact_reference_rejects_what_lies_outside_its_domain():
    inst = fam.make("T0", 2, 1, "plain")
    inst.lb[0, 0] = -1
    net = _sub_net(inst)
    with pytest.raises(ValueError, match="negative lower bound"):
        xf.solve(net, all_matchings(inst)[0], 0)
