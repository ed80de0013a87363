"""List-scheduling simulator of k_relax's launch tail, replayed from measured per-record clocks.

    python tools/tail_sim.py DUMP.npz [--slots 2048] [--xcds 8] [--q 16 32] [--reentry-us 9] [--empty-us 2]

DUMP.npz comes from `tools/relax_diag.py --nodes 8192 --chunk 0 --dump DUMP.npz` run with the
profiling library (SGUFP_LIB_PATH=sgufp_solver_amd/lib_prof/libsgufp_hip.so): per record the wave's
wall-clock ticks, its phase clocks, the cuts it applied and its status.

A record is one wave; the device holds `slots` of them (CUs x k_relax's occupancy), dealt over
--xcds XCDs: workgroup b of a launch belongs to XCD b % xcds, and an XCD hands a free slot to its
next workgroup of the launch in dispatch order (the library's fixed permutation of the batch).  Three shapes are replayed:

  one launch            every record is one indivisible job (what the parent commit runs);
  chunks, one stream    a head launch (build, feasibility batches, screen) and ceil(O / q) chunk
                        launches of q pool positions, each launch starting when the one before has
                        drained: every launch has its own tail;
  chunks, S streams     the dispatch order in S contiguous parts, each an in-order chain of such
                        launches; the chains share the slots, so one chain's draining launch leaves
                        its free slots to the other chain's current launch.

Per-record cost model: the head costs the build clock plus the share of the rest that the
feasibility and screened cuts have among the record's applied cuts; the remaining time is spread
evenly over the in-order optimality positions, and a chunk launch costs its positions plus
--reentry-us (restore and save of the resume state); a workgroup whose record is not suspended
costs --empty-us.  The first shape uses the measured wave times unchanged, so it checks the
scheduler against the measured launch: the two must agree within a few percent before the other
shapes mean anything.
"""
import argparse
import heapq

import numpy as np


def dispatch_order(n):
    """The library's dispatch permutation (sgufp_ctx::relax_order: Fisher-Yates over splitmix64)."""
    m = (1 << 64) - 1
    p = list(range(n))
    if n < 3:
        return np.array(p)
    x = 0x9E3779B97F4A7C15 ^ n
    for i in range(n - 1, 0, -1):
        x = (x + 0x9E3779B97F4A7C15) & m
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        j = z % (i + 1)
        p[i], p[j] = p[j], p[i]
    return np.array(p)


def simulate(chains, slots, xcds=8):
    """chains: per chain a list of launches, each a list of job costs in dispatch order.  Workgroup
    b of a launch runs on XCD b % xcds (the hardware deals a grid's workgroups round-robin over the
    XCDs), each XCD holding slots / xcds waves.  A launch of a chain starts when the chain's previous
    launch has finished on every XCD; an XCD's free slot goes to the chains' current launches in
    turn.  Returns the makespan."""
    per = slots // xcds
    free = [(0.0, x) for x in range(xcds) for _ in range(per)]
    heapq.heapify(free)
    parked = []   # slots with no job to take until some chain starts its next launch
    # per chain: current launch, next job index per XCD, jobs left in the launch, start and end time
    state = []
    for ch in chains:
        state.append({"launch": 0, "next": list(range(xcds)), "left": len(ch[0]) if ch else 0, "ready": 0.0, "end": 0.0})
    turn = 0
    end = 0.0
    while free:
        t, x = heapq.heappop(free)
        cand = [c for c in range(len(chains)) if state[c]["launch"] < len(chains[c]) and
                state[c]["next"][x] < len(chains[c][state[c]["launch"]])]
        if not cand:
            if any(state[c]["launch"] < len(chains[c]) for c in range(len(chains))):
                parked.append((t, x))
            continue
        ok = [c for c in cand if state[c]["ready"] <= t]
        if ok:
            c = min(ok, key=lambda k: (k - turn) % len(chains))
            turn = (c + 1) % len(chains)
        else:
            c = min(cand, key=lambda k: state[k]["ready"])
        s = state[c]
        jobs = chains[c][s["launch"]]
        fin = max(t, s["ready"]) + jobs[s["next"][x]]
        s["next"][x] += xcds
        heapq.heappush(free, (fin, x))
        s["end"] = max(s["end"], fin)
        end = max(end, fin)
        s["left"] -= 1
        if s["left"] == 0:
            s["launch"] += 1
            s["next"] = list(range(xcds))
            s["ready"] = s["end"]
            if s["launch"] < len(chains[c]):
                s["left"] = len(chains[c][s["launch"]])
            for it in parked:
                heapq.heappush(free, it)
            parked = []
    return end


def chunk_jobs(us, build, sweeps, n_feas, n_opt, screen, q, reentry, empty):
    """Per record the head cost and the chunk costs (`empty` for launches after its last)."""
    n = len(us)
    nchunk = (n_opt + q - 1) // q
    head = np.empty(n)
    chunks = np.full((n, nchunk), empty)
    for k in range(n):
        applied = max(int(sweeps[k]), 1)
        pre = min(applied, n_feas + screen)
        inorder = applied - pre
        rest = max(us[k] - build[k], 0.0)
        if inorder <= 0:
            head[k] = us[k]
            continue
        head[k] = build[k] + rest * pre / applied
        per = rest / applied
        left, c = inorder, 0
        while left > 0 and c < nchunk:
            take = left if c == nchunk - 1 else min(left, q)
            chunks[k, c] = per * take + reentry
            left -= take
            c += 1
    return head, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dump")
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--xcds", type=int, default=8, help="XCDs the workgroups are dealt over (1: one shared pool of slots)")
    ap.add_argument("--q", type=int, nargs="*", default=[8, 16, 32])
    ap.add_argument("--reentry-us", type=float, nargs="*", default=[0.0, 20.0, 100.0, 250.0])
    ap.add_argument("--empty-us", type=float, default=2.0)
    ap.add_argument("--screen", type=int, default=4, help="optimality cuts the screen applies (the cut-batch size)")
    ap.add_argument("--streams", type=int, nargs="*", default=[1, 2, 4])
    args = ap.parse_args()
    d = np.load(args.dump)
    us = d["ticks"] / 100.0
    build = d["phases"][:, 0] / 100.0
    sweeps = d["sweeps"]
    n_feas, n_opt = int(d["n_feas"]), int(d["n_opt"])
    order = dispatch_order(len(us))
    one = simulate([[list(us[order])]], args.slots, args.xcds)
    measured = float(d["ms_relax"]) * 1e3
    print(f"records {len(us)}, slots {args.slots}: wave us mean {us.mean():.0f} max {us.max():.0f}; "
          f"sum / slots {us.sum() / args.slots:.0f} us")
    print(f"one launch: simulated {one:.0f} us, measured {measured:.0f} us ({100 * (one / measured - 1):+.1f} %)")
    for q in args.q:
        for re_us in args.reentry_us:
            head, chunks = chunk_jobs(us, build, sweeps, n_feas, n_opt, args.screen, q, re_us, args.empty_us)
            line = f"q {q:3d} re-entry {re_us:5.0f} us:"
            for s in args.streams:
                chains = []
                for p in range(s):
                    part = order[len(order) * p // s:len(order) * (p + 1) // s]
                    chains.append([list(head[part])] + [list(chunks[part, c]) for c in range(chunks.shape[1])])
                t = simulate(chains, args.slots, args.xcds)
                line += f"  {s} stream{'s' if s > 1 else ' '} {t:7.0f} us ({100 * (t / one - 1):+5.1f} %)"
            print(line)


if __name__ == "__main__":
    main()
