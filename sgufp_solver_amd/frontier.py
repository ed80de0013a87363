"""Open-node frontiers for benches and the batched solver driver, and the host statement of
the best-bound selection rule (select_order: what sgufp_frontier_select does on the device).

bfs_frontier follows the survey probe: start from the root record
(DDSolver::startSolver builds the root with Node{}, DDSolver.cpp:788-791) and expand
cutset children breadth-first on the device until ``n`` records exist.
"""
from __future__ import annotations

import numpy as np

from . import engine as E
from .pools import DOUBLE_MAX, DOUBLE_MIN, NodeRecord


def root_batch() -> E.BatchArrays:
    return E.BatchArrays([NodeRecord(0, DOUBLE_MIN, DOUBLE_MAX, [], [])])


def bfs_frontier(eng: E.Engine, n: int, incumbent: float = DOUBLE_MIN) -> E.BatchArrays:
    """First ``n`` records of a BFS over cutset children (relaxed with the engine's pool)."""
    level = root_batch()
    done = []
    count = 0
    queue = [level]
    while queue and count < n:
        cur = queue.pop(0)
        if cur.n == 0:
            continue
        nxt_parts = []
        got = 0
        for s in range(0, cur.n, eng.info.max_batch):
            part = E.batch_slice(cur, np.arange(s, min(cur.n, s + eng.info.max_batch)))
            eng.upload(part)
            eng.relax_async(incumbent)
            eng.sync()
            nxt_parts.append(eng.children_batch())
            got += nxt_parts[-1].n
            if count + got >= n:
                break   # the first n records of BFS order are complete: stop relaxing this level
        nxt = E.batch_concat(nxt_parts)
        take = min(n - count, nxt.n)
        done.append(E.batch_slice(nxt, np.arange(take)))
        count += take
        queue.append(nxt)
    return E.batch_concat(done) if done else root_batch()


def select_order(ub, k: int) -> np.ndarray:
    """The permutation sgufp_frontier_select(k, SGUFP_SELECT_BEST_BOUND) applies to a stack whose
    records have upper bounds ``ub`` (index 0 = bottom): entry j of the new stack is entry
    ``perm[j]`` of the old one.

    Records are ordered by ub descending, compared as doubles (-0.0 and 0.0 tie); among equal ub
    the record nearer the top (larger index) comes first.  The first k of that order are
    selected; the others keep entries [0, n - k) and the selected ones get [n - k, n), both in
    their previous relative order.  k is clamped to [0, n] (the device call clamps to max_batch
    before): k >= n or k == 0 gives the identity."""
    ub = np.asarray(ub, dtype=np.float64)
    n = ub.size
    k = min(max(int(k), 0), n)
    idx = np.arange(n, dtype=np.int64)
    if k == 0 or k == n:
        return idx
    key = ub + 0.0                                # -0.0 + 0.0 == +0.0
    order = np.lexsort((-idx, -key))              # ub descending, then index descending
    sel = np.zeros(n, dtype=bool)
    sel[order[:k]] = True
    return np.concatenate([idx[~sel], idx[sel]])
