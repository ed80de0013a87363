"""Enumeration of V-bar matchings (shared by the exhaustive tests)."""
import itertools


def node_matchings(ins, outs):
    """All partial matchings between in-arc tails and out-arc heads of one V-bar node."""
    res = [()]
    for k in range(1, min(len(ins), len(outs)) + 1):
        for a in itertools.combinations(ins, k):
            for b in itertools.permutations(outs, k):
                res.append(tuple(zip(a, b)))
    return res


def all_matchings(inst):
    """Every matching y = {(i, q, j): 1} of the instance, in a fixed order (the product of the
    per-node lists in V-bar order)."""
    T, H = inst.tails, inst.heads
    per_node = []
    for q in inst.vbar:
        q = int(q)
        ins = sorted({int(T[a]) for a in range(inst.m) if int(H[a]) == q})
        outs = sorted({int(H[a]) for a in range(inst.m) if int(T[a]) == q})
        per_node.append([tuple((i, q, j) for i, j in mt) for mt in node_matchings(ins, outs)])
    return [{t: 1 for part in combo for t in part} for combo in itertools.product(*per_node)]

