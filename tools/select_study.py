"""Measurements of the best-bound node selection (sgufp_frontier_select):

    python tools/select_study.py cost [--sizes 1000,100000,1000000] [--ks 64,1024] [--reps 21] [--out F.json]
        host-clock median of one select over synthetic stacks of real C4 records (the first
        records of a BFS over cutset children, repeated cyclically, random ub), next to the
        bytes the scatter moves.  Under `rocprofv3 --kernel-trace --stats -- python ...` the
        same run gives the kernel times.
    python tools/select_study.py seeded [--config C4] [--policy lifo|best_bound] [--seconds 20] [--out F.json]
        the seeded leg of bench.py --full (bnb_run(config, 1, "zero", seconds, 1024, 5 s,
        heuristic=128)) under one policy, with best_bound / gap / open_nodes sampled every second.

Each prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sgufp_solver_amd import engine as E  # noqa: E402
from sgufp_solver_amd import frontier, instance  # noqa: E402
from sgufp_solver_amd.pools import DOUBLE_MIN  # noqa: E402
from sgufp_solver_amd.solution import gap_of  # noqa: E402
from sgufp_solver_amd.solver import DDSolver  # noqa: E402

HBM_BYTES_PER_S = 6.3e12   # what VERDICT.md takes as achievable on the MI355X
RECORD_BYTES = 2 + 8 + 8 + 4 + 1 + 8 + 2   # gl, lb, ub, mask, valid, sol_off, sol_len


def network(cfg_name, seed=1):
    inst = instance.generate(instance.CONFIGS[cfg_name], seed)
    inst.lb[:] = 0
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_sel_"), f"{cfg_name}.txt")
    inst.write(path)
    return path


def repeat(b, n):
    """n records: those of b cyclically (vectorised batch_slice)."""
    idx = np.arange(n, dtype=np.int64) % b.n

    def ragged(off, data):
        lens = off[idx + 1] - off[idx]
        new = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=new[1:])
        return new, data[np.repeat(off[idx] - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)]
    st_off, st = ragged(b.states_off, b.states)
    so_off, so = ragged(b.sol_off, b.sol)
    return E.batch_from_arrays(b.gl[idx], b.lb[idx], b.ub[idx], st_off, st, so_off, so)


def cost(args):
    eng = E.Engine(network(args.config), 0, 1024)
    base = frontier.bfs_frontier(eng, 2048)
    rows = []
    for n in [int(x) for x in args.sizes.split(",")]:
        b = repeat(base, n)
        b.ub = np.ascontiguousarray(np.round(np.random.default_rng(n).uniform(0.0, 1e4, size=n), 2))
        sol_entries = int(b.sol_off[-1])
        for k in [int(x) for x in args.ks.split(",")]:
            eng.frontier_clear()
            eng.frontier_push(b)
            perm = frontier.select_order(b.ub, k)
            moved = int((perm != np.arange(n)).sum())
            lowest = int(perm[n - k]) if k < n else n          # lowest selected index
            suffix_entries = int(b.sol_off[-1] - b.sol_off[lowest]) if lowest < n else 0
            t = []
            for _ in range(args.reps):   # every call runs every kernel, the scatter included
                eng.sync()
                t0 = time.perf_counter()
                eng.frontier_select(k)
                t.append(time.perf_counter() - t0)
            if k < n:   # the selected records are on top, in stack order
                assert eng.frontier_peek(n - k, k).ub.tobytes() == b.ub[perm[n - k:]].tobytes()
            scatter = 2 * (n * RECORD_BYTES + 2 * sol_entries)
            suffix = 2 * ((n - lowest) * RECORD_BYTES + 2 * suffix_entries)
            rows.append({"n": n, "k": k, "moved_by_first_select": moved, "mean_sol_len": round(sol_entries / n, 1),
                         "first_call_ms": round(t[0] * 1e3, 3), "median_ms": round(float(np.median(t[1:])) * 1e3, 3),
                         "min_ms": round(min(t[1:]) * 1e3, 3), "scatter_bytes": scatter,
                         "scatter_us_at_6.3TBps": round(scatter / HBM_BYTES_PER_S * 1e6, 2),
                         "suffix_bytes": suffix, "suffix_share": round(suffix / scatter, 4)})
            print(rows[-1], file=sys.stderr, flush=True)
    eng.close()
    return {"study": "cost of one sgufp_frontier_select", "config": args.config, "launches": 21, "rows": rows}


class Sampled(E.Engine):
    """Engine that samples the bound over the frontier about once a second between rounds."""

    def __init__(self, *a):
        super().__init__(*a)
        self.samples, self.t0, self.next = [], None, 1.0

    def bnb_step(self, incumbent, max_nodes=0):
        z, st = super().bnb_step(incumbent, max_nodes)
        if self.t0 is not None and time.perf_counter() - self.t0 >= self.next:
            mx, op = self.frontier_bound(z)
            bound = max(z, mx)
            self.samples.append({"t": round(time.perf_counter() - self.t0, 2), "z": z, "best_bound": bound,
                                 "gap": gap_of(z, bound, False), "open_nodes": op, "stack": self.frontier_size()})
            self.next += 1.0
        return z, st


def seeded(args):
    net = network(args.config)
    eng = Sampled(net, 0, 1024)
    solver = DDSolver(net, engine=eng, verbose=False, time_budget=2.0, round_seconds=2.0,
                      node_selection=args.policy)
    solver.start_solver(DOUBLE_MIN)      # warm-up, as bench.bnb_run
    eng.clear_cuts()
    solver.time_budget, solver.round_seconds, solver.restricted_width = args.seconds, 5.0, 128
    eng.t0 = t0 = time.perf_counter()
    z = solver.start_solver(DOUBLE_MIN)
    elapsed = time.perf_counter() - t0
    r = solver.result()
    out = {"study": "seeded search under one node selection policy", "config": args.config, "policy": args.policy,
           "seconds": round(elapsed, 3), "rounds": solver.rounds, "incumbent": z,
           "heuristic_incumbent": solver.heuristic_incumbent,
           "relaxations_per_s": round(solver.counters["relaxed"] / elapsed, 2), "best_bound": r.bound, "gap": r.gap,
           "open_nodes": r.open_nodes, "frontier_left": eng.frontier_size(), "complete": r.complete,
           "pool": [eng.cuts_count(1), eng.cuts_count(0)], "counters": dict(solver.counters), "trajectory": eng.samples}
    eng.close()
    return out


def finite(x):
    """inf -> "inf" so that the line is strict JSON."""
    if isinstance(x, float) and x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    if isinstance(x, dict):
        return {k: finite(v) for k, v in x.items()}
    if isinstance(x, list):
        return [finite(v) for v in x]
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("study", choices=["cost", "seeded"])
    ap.add_argument("--config", default="C4")
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--ks", default="64,1024")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--policy", default="best_bound", choices=["lifo", "best_bound"])
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = cost(args) if args.study == "cost" else seeded(args)
    line = json.dumps(finite(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
