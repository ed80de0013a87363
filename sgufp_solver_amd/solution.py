"""What a search leaves behind besides its value: the incumbent's routing, the proven bound
and the gap.

The reference prints the incumbent's value only (DDSolver.cpp:848-867); everything here is an
extension.  A path is the list of DD decisions of an exact leaf, one per layer: layer ``a``
decides the in-arc ``layer_arcs[a]`` (tail i, head q, q a V-bar node), the decision is the
out-arc of q it is matched to, or -1.  That is the y-bar GuroSolver::solveSubProblem builds
from a path (grb.cpp:139-150).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

from .pools import DOUBLE_MIN


def matching_of_path(layer_arcs: Sequence[int], tails: Sequence[int], heads: Sequence[int],
                     path: Sequence[int]) -> Dict[Tuple[int, int, int], int]:
    """{(i, q, j): 1}: in-arc (i, q) of V-bar node q is routed to its out-arc (q, j)."""
    y = {}
    for a, d in enumerate(path):
        d = int(d)
        if d == -1:
            continue
        arc = int(layer_arcs[a])
        y[(int(tails[arc]), int(heads[arc]), int(heads[d]))] = 1
    return y


def arcs_of_file(network_path: str) -> Tuple[List[int], List[int]]:
    """(tails, heads) of a network file: "n m S", then one line per arc starting "tail head"."""
    with open(network_path) as fh:
        m = int(fh.readline().split()[1])
        tails, heads = [], []
        for _ in range(m):
            t, h = fh.readline().split()[:2]
            tails.append(int(t))
            heads.append(int(h))
    return tails, heads


def gap_of(value: float, bound: Optional[float], complete: bool) -> Optional[float]:
    """(bound - value) / max(1, |value|): exactly 0 for a completed search, inf while there is
    no incumbent, None when no bound is known."""
    if complete:
        return 0.0
    if bound is None:
        return None
    if value == DOUBLE_MIN:
        return float("inf")
    return (bound - value) / max(1.0, abs(value))


@dataclass
class Solution:
    """DDSolver.result(): ``path`` / ``matching`` are None when no routing is known (an engine
    without bnb_incumbent, or a seeded value no leaf beat), ``bound`` / ``gap`` / ``open_nodes``
    are None for an engine without frontier_bound."""
    value: float
    path: Optional[List[int]]
    matching: Optional[Dict[Tuple[int, int, int], int]]
    bound: Optional[float]
    gap: Optional[float]
    open_nodes: Optional[int]
    complete: bool
