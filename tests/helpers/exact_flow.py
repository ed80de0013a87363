"""Exact integer reference of the scenario subproblem (TEST INFRASTRUCTURE ONLY).

The scenario problem of oracle/subproblem_oracle.py (the primal of the reference's dual LP,
grb.cpp:42-136) restated in Python ints, without an LP solver and without a tolerance:

  * the matching y joins in- and out-arcs at the V-bar nodes into chains.  A chain from a
    non-V-bar tail to a non-V-bar head ("complete") is one arc with bounds [max l, min u] and
    reward sum r; any other chain is fixed at 0, which is infeasible if max l > 0 or min u < 0;
  * an arc from a node without in-arcs to a node without out-arcs (the reference's A4 set, which
    Network.cpp:80 empties: the dual has no row for it) carries nothing and earns nothing; its
    beta / gamma still stand in the dual objective, so l > 0 or u < 0 on it makes the scenario
    infeasible;
  * every node without in-arcs is a free supply and every node without out-arcs a free demand
    (the dual's A1 / A2 rows hold no alpha for them, whichever their ids); every other node
    conserves flow;
  * lower bounds are shifted into node demands and the max-reward flow is solved by
    networkx.network_simplex on a MultiDiGraph (integer data: exact).

Input domain: acyclic networks without parallel arcs, lb >= 0 (ValueError otherwise: with a
negative lower bound an unmatched arc is no longer fixed at 0 and the contraction does not hold).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import networkx as nx

Matching = Dict[Tuple[int, int, int], int]


class Contraction:
    """The chains of one matching (scenario-independent): ``chains`` is a list of
    (tail or -1, head or -1, [arc ids in order]); ``a4`` the dropped source->sink arcs."""

    def __init__(self, net, y: Matching):
        n, m = net.n, net.m
        T = [int(t) for t in net.tails]
        H = [int(h) for h in net.heads]
        vb = set(int(v) for v in net.vbar)
        indeg = [0] * n
        outdeg = [0] * n
        arc = {}
        for a in range(m):
            outdeg[T[a]] += 1
            indeg[H[a]] += 1
            if (T[a], H[a]) in arc:
                raise ValueError("parallel arcs")
            arc[(T[a], H[a])] = a
        nxt = [-1] * m            # the out-arc matched to in-arc a at a V-bar head
        chosen = [False] * m
        for (i, q, j), v in y.items():
            if not v:
                continue
            if q not in vb:
                raise ValueError(f"matching at a node outside V-bar: {q}")
            a, b = arc[(i, q)], arc[(q, j)]
            if nxt[a] != -1 or chosen[b]:
                raise ValueError("not a matching")
            nxt[a] = b
            chosen[b] = True
        self.n, self.m = n, m
        self.src = [indeg[v] == 0 and outdeg[v] > 0 for v in range(n)]
        self.snk = [outdeg[v] == 0 and indeg[v] > 0 for v in range(n)]
        self.a4 = [a for a in range(m) if indeg[T[a]] == 0 and outdeg[H[a]] == 0]
        a4 = set(self.a4)
        self.chains: List[Tuple[int, int, List[int]]] = []
        for a in range(m):
            if a in a4 or (T[a] in vb and chosen[a]):
                continue
            arcs = [a]
            e = a
            h = -1
            while True:
                q = H[e]
                if q not in vb:
                    h = q
                    break
                if nxt[e] < 0:
                    break
                e = nxt[e]
                arcs.append(e)
                if len(arcs) > m:
                    raise ValueError("cyclic chain")
            self.chains.append((-1 if T[a] in vb else T[a], h, arcs))


def solve(net, y: Matching, s: int, want_flow: bool = False, contraction: Optional[Contraction] = None):
    """(status, objective) -- or (status, objective, flow per arc) -- of scenario s under y:
    status 'optimal' with an int objective, or 'infeasible' with None."""
    C = contraction if contraction is not None else Contraction(net, y)
    lb = [int(v) for v in net.lb[:, s]]
    ub = [int(v) for v in net.ub[:, s]]
    rw = [int(v) for v in net.reward[:, 0]]      # scenario-0 rewards (grb.cpp:53,71,89)
    if min(lb, default=0) < 0:
        raise ValueError("negative lower bound: outside the subproblem's input domain")
    bad = ("infeasible", None, None) if want_flow else ("infeasible", None)
    for a in C.a4:
        if lb[a] > 0 or ub[a] < 0:
            return bad
    G = nx.MultiDiGraph()
    Z = C.n
    demand = [0] * (C.n + 1)
    const = 0
    live = []
    for k, (t, h, arcs) in enumerate(C.chains):
        L = max(lb[a] for a in arcs)
        U = min(ub[a] for a in arcs)
        if t < 0 or h < 0:
            if L > 0 or U < 0:
                return bad
            continue
        if L > U:
            return bad
        R = sum(rw[a] for a in arcs)
        const += R * L
        demand[t] += L
        demand[h] -= L
        live.append((k, t, h, L))
        G.add_edge(t, h, key=k, capacity=U - L, weight=-R)
    for v in range(C.n):
        if C.src[v]:
            G.add_edge(Z, v, key=-1, weight=0)
        if C.snk[v]:
            G.add_edge(v, Z, key=-1, weight=0)
    G.add_node(Z)
    for v in list(G.nodes):
        G.nodes[v]["demand"] = demand[v]
    if any(demand[v] for v in range(C.n + 1) if v not in G):
        return bad
    try:
        cost, flow = nx.network_simplex(G)
    except nx.NetworkXUnfeasible:
        return bad
    obj = const - int(cost)
    if not want_flow:
        return "optimal", obj
    x = [0] * C.m
    for k, t, h, L in live:
        f = L + int(flow[t][h][k])
        for a in C.chains[k][2]:
            x[a] = f
    return "optimal", obj, x


def q_table(net, ys: Sequence[Matching]):
    """Q[k][s] = objective (int) of scenario s under ys[k], None where infeasible."""
    out = []
    for y in ys:
        C = Contraction(net, y)
        out.append([solve(net, y, s, contraction=C)[1] for s in range(net.S)])
    return out
