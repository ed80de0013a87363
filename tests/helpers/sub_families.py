"""Data families for the subproblem tests: a generated tiny network with its scenario data
rewritten so that one class of input is exercised (tests/test_exact_flow.py on the CPU,
tests/test_subproblem_exhaustive.py on the device).  Every family is deterministic in
(config, seed, S); scenarios get different data (rewards are scenario-invariant: the
subproblem reads scenario 0's, grb.cpp:53,71,89)."""
import numpy as np

from sgufp_solver_amd import instance


def _touches_vbar(inst, a):
    vb = set(int(v) for v in inst.vbar)
    return int(inst.tails[a]) in vb or int(inst.heads[a]) in vb


def _set_reward(inst, r):
    inst.reward[:] = np.asarray(r, dtype=np.int32)[:, None]


def make(cfg: str, seed: int, S: int, family: str) -> instance.Instance:
    inst = instance.generate(instance.CONFIGS[cfg], seed, scenarios=S)
    rng = np.random.default_rng([seed, S, sum(family.encode())])
    m = inst.m
    sink = inst.n - 1
    non_sink = np.nonzero(inst.heads != sink)[0]
    if family == "gen_lb":                       # the generator's sink-arc bounds
        pass
    elif family == "plain":
        inst.lb[:] = 0
    elif family == "zero_cap":                   # chains with min u = 0
        inst.lb[:] = 0
        inst.ub[rng.random(size=(m, S)) < 0.25] = 0
    elif family == "inner_lb":                   # lower bounds away from the sink
        inst.lb[:] = 0
        mask = np.zeros((m, S), dtype=bool)
        mask[non_sink] = rng.random(size=(len(non_sink), S)) < 0.025
        for s in range(S):                       # at least one per scenario
            if not mask[:, s].any():
                mask[rng.choice(non_sink), s] = True
        inst.lb[mask] = rng.integers(1, 4, size=int(mask.sum()))
    elif family == "fixed":                      # l == u on two arcs per scenario
        inst.lb[:] = 0
        for s in range(S):
            for a in rng.choice(m, size=2, replace=False):
                inst.lb[a, s] = inst.ub[a, s] = int(rng.integers(1, 4))
    elif family == "crossed":                    # l > u on one arc, last scenario only; the arc is
        inst.lb[:] = 0                           # its chain's max-l and min-u arc (ray_p == ray_q)
        a = int(rng.choice(non_sink))
        inst.ub[a, S - 1] = 1
        inst.lb[a, S - 1] = 2
    elif family == "crossed_split":              # max l on one arc above min u of another arc of the
        inst.lb[:] = 0                           # chain (ray_p != ray_q): u is 5..50 elsewhere
        a = int(rng.choice([b for b in non_sink if _touches_vbar(inst, b)]))
        inst.lb[a, S - 1] = inst.ub[a, S - 1] = 60
    elif family == "broken_lb":                  # l > 0 on an arc a matching can leave unmatched
        inst.lb[:] = 0
        a = int(rng.choice([b for b in range(m) if _touches_vbar(inst, b)]))
        inst.lb[a, S - 1] = 2
    elif family == "neg_rewards":                # optimum: the forced minimum of the lower bounds
        _set_reward(inst, -rng.integers(1, 10, size=m))
    elif family == "zero_rewards":
        _set_reward(inst, np.zeros(m))
    elif family == "ties":                       # many equal-cost augmenting paths
        inst.lb[:] = 0
        inst.ub[:] = 1
        _set_reward(inst, np.ones(m))
    else:
        raise KeyError(family)
    return inst


def network(n, arcs, lb, ub, r, vbar, S):
    """Hand-made network: arcs [(tail, head)], per-arc lb / ub (scalars or [S] lists) and rewards."""
    m = len(arcs)

    def col(v):
        v = np.asarray(v, dtype=np.int32)
        return np.broadcast_to(v if v.ndim == 0 else v.reshape(m, -1), (m, S)).copy()

    return instance.Instance(n=n, tails=np.array([a[0] for a in arcs], dtype=np.int32),
                             heads=np.array([a[1] for a in arcs], dtype=np.int32), lb=col(lb), ub=col(ub),
                             reward=col(r), vbar=list(vbar))


def with_arcs(inst, arcs, lb, ub, r):
    """inst with extra arcs appended (lb / ub per arc: scalars or [S] lists)."""
    S = inst.scenarios
    extra = network(inst.n, arcs, lb, ub, r, inst.vbar, S)
    return instance.Instance(n=inst.n, tails=np.concatenate([inst.tails, extra.tails]),
                             heads=np.concatenate([inst.heads, extra.heads]), lb=np.vstack([inst.lb, extra.lb]),
                             ub=np.vstack([inst.ub, extra.ub]), reward=np.vstack([inst.reward, extra.reward]),
                             vbar=list(inst.vbar))


def direct_arc(S, lb_last):
    """T2 seed 2 without lower bounds plus one arc source -> sink (r = 10, u = 5); lb_last is its
    lower bound in the last scenario (0 elsewhere)."""
    inst = make("T2", 2, S, "plain")
    return with_arcs(inst, [(0, inst.n - 1)], [[0] * (S - 1) + [lb_last]], 5, 10)


def neg_ub(cfg, seed, S):
    """u = -1 < l = 0 on one arc beside a V-bar node, last scenario only: its chain is complete
    under some matchings and broken under others, and infeasible under all."""
    inst = make(cfg, seed, S, "plain")
    rng = np.random.default_rng([seed, S, 77])
    a = int(rng.choice([b for b in range(inst.m) if _touches_vbar(inst, b)]))
    inst.ub[a, S - 1] = -1
    return inst


def two_sources_two_sinks(S, seed=1):
    """Nodes 0 and 1 have no in-arcs, nodes 6 and 7 no out-arcs; V-bar = {2, 3}; 4 and 5 conserve."""
    arcs = [(0, 2), (1, 2), (0, 3), (1, 3), (2, 4), (2, 6), (3, 4), (3, 5), (4, 7), (5, 7), (5, 6)]
    rng = np.random.default_rng([seed, S, 5])
    m = len(arcs)
    lb = np.zeros((m, S), dtype=np.int32)
    lb[5, S - 1] = 2                              # into the second sink
    lb[8, 0] = 1
    return network(8, arcs, lb, rng.integers(3, 12, size=(m, S)), rng.integers(-4, 15, size=m), [2, 3], S)


def fans(S, seed=1):
    """V-bar node 1 with one in-arc and four out-arcs, V-bar node 6 with four in-arcs and one
    out-arc; 2 .. 5 conserve and have side arcs from the source / to the sink."""
    arcs = [(0, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 6), (3, 6), (4, 6), (5, 6), (6, 7), (0, 2), (0, 4), (3, 7), (5, 7)]
    rng = np.random.default_rng([seed, S, 6])
    m = len(arcs)
    lb = np.zeros((m, S), dtype=np.int32)
    lb[9, S - 1] = 1
    return network(8, arcs, lb, rng.integers(2, 9, size=(m, S)), rng.integers(-3, 12, size=m), [1, 6], S)


def line(K, lb_arc=None, seed=1):
    """0 -> 1 -> ... -> K -> K+1 with V-bar = 1 .. K; two scenarios, the second with lb = 1 on
    arc lb_arc (None: no lower bound)."""
    arcs = [(v, v + 1) for v in range(K + 1)]
    rng = np.random.default_rng([seed, K, 9])
    m = K + 1
    lb = np.zeros((m, 2), dtype=np.int32)
    if lb_arc is not None:
        lb[lb_arc, 1] = 1
    return network(K + 2, arcs, lb, rng.integers(3, 9, size=(m, 2)), rng.integers(-3, 5, size=m), range(1, K + 1), 2)


def padded(inst, n):
    """inst inside a network of n nodes: node 0 stays the source, the sink becomes n - 1, the
    other nodes take the highest ids below it and the ids between are isolated nodes."""
    shift = n - inst.n
    f = lambda v: v if v == 0 else v + shift
    return instance.Instance(n=n, tails=np.array([f(int(v)) for v in inst.tails], dtype=np.int32),
                             heads=np.array([f(int(v)) for v in inst.heads], dtype=np.int32), lb=inst.lb.copy(),
                             ub=inst.ub.copy(), reward=inst.reward.copy(), vbar=[f(int(v)) for v in inst.vbar])
