"""Per-node diagnostics of one relaxation step on the bench workload (GPU).

    python tools/relax_diag.py [--config C4 --seed 1 --nodes 4096 --cb 16 --refold]
                               [--chunk Q --streams S] [--dump FILE.npz]
    python tools/relax_diag.py --trace KERNEL_TRACE.csv

Prints the k_relax time, the distribution of per-wave wall-clock ticks against DD
size / status / cuts applied / batched-sweep restarts.  --chunk / --streams set the split
relaxation (SGUFP_RELAX_CHUNK / SGUFP_RELAX_STREAMS; --chunk 0: one launch); --dump writes the
per-record clocks for tools/tail_sim.py.  The per-wave clocks of a split step are summed over the
record's launches; phase 7 (epilogue) then holds every save and restore.

--trace reads a `rocprofv3 --kernel-trace --output-format csv` file of a run instead (no GPU):
per step -- the k_relax launches between two k_scan2 -- every launch's queue, start, duration and
the time it shared the device with a k_relax launch of another queue."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trace_report(path, steps=2):
    """Per-launch times of the last `steps` relaxation steps in a rocprofv3 kernel trace."""
    import csv
    import re
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            if "k_relax" in name or "k_scan2" in name:
                m = re.search(r"k_relax<\d+, (\d)>", name)
                kind = "scan" if "k_scan2" in name else ("whole", "head", "chunk")[int(m.group(1))] if m else "whole"
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), kind,
                             int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0)))
    rows.sort()
    groups, cur = [], []
    for r in rows:
        if r[3] == "scan":
            if cur:
                groups.append(cur)
            cur = []
        else:
            cur.append(r)
    for g in groups[-steps:]:
        t0, t1 = g[0][0], max(r[1] for r in g)
        print(f"step: {len(g)} k_relax launches on {len({r[2] for r in g})} queue(s), {(t1 - t0) / 1e6:.3f} ms "
              f"from the first start to the last end, {sum(r[1] - r[0] for r in g) / 1e6:.3f} ms summed")
        for a, b, q, kind, grid in g:
            shared = sum(max(0, min(b, d) - max(a, c)) for c, d, q2, _, _ in g if q2 != q)
            print(f"  queue {q} {kind:5s} grid {grid:7d} start {(a - t0) / 1e6:8.3f} ms  {(b - a) / 1e6:7.3f} ms  "
                  f"shared with another queue {shared / 1e6:7.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--cb", default=None)
    ap.add_argument("--incumbent", default="p40")
    ap.add_argument("--refold", action="store_true", help="also print the exact redos' refold counters")
    ap.add_argument("--chunk", default=None, help="SGUFP_RELAX_CHUNK (0: one launch)")
    ap.add_argument("--streams", default=None, help="SGUFP_RELAX_STREAMS")
    ap.add_argument("--dump", default=None, help="write the per-record clocks (tools/tail_sim.py) to this .npz")
    ap.add_argument("--trace", default=None, help="a rocprofv3 kernel trace CSV to report on (no GPU)")
    args = ap.parse_args()
    if args.trace:
        return trace_report(args.trace)
    if args.chunk is not None:
        os.environ["SGUFP_RELAX_CHUNK"] = args.chunk
    if args.streams is not None:
        os.environ["SGUFP_RELAX_STREAMS"] = args.streams
    if args.refold:
        os.environ["SGUFP_REFOLD_STATS"] = "1"
    if args.cb:
        os.environ["SGUFP_CUT_BATCH"] = args.cb
    from sgufp_solver_amd import engine as E
    from sgufp_solver_amd import frontier, instance, pools
    inst = instance.generate(instance.CONFIGS[args.config], args.seed, scenarios=1)
    d = tempfile.mkdtemp()
    inst.write(f"{d}/net.txt")
    eng = E.Engine(f"{d}/net.txt", 0, args.nodes)
    fr = frontier.bfs_frontier(eng, args.nodes)
    eng.add_cuts(pools.synthetic_pool(inst, 16, 64, args.seed))
    eng.upload(fr)
    if args.incumbent.startswith("p"):
        eng.relax_async(pools.DOUBLE_MIN)
        eng.sync()
        st, ex, lb, ub, nc = eng.results_arrays()
        inc = float(np.percentile(ub[(st == 0) | (st == 3)], float(args.incumbent[1:])))
    else:
        inc = float(args.incumbent)
    eng.set_timing(True)
    for _ in range(2):
        eng.relax_async(inc)
        eng.sync()
    t0 = time.perf_counter()
    eng.relax_async(inc)
    eng.sync()
    wall = time.perf_counter() - t0
    ms_relax, ms_emit = eng.last_timing()
    st, ex, lb, ub, nc = eng.results_arrays()
    dn, da, dl, sw = eng.stats()
    ticks, rinfo = eng.debug()
    rinfo = rinfo.astype(np.int64) & 0xFFFFFFFF
    redo = rinfo & 0xFF
    stream = (rinfo >> 31) & 1
    mirsz = (rinfo >> 8) & 0x7FFFFF
    us = ticks / 100.0
    print(f"cb={os.environ.get('SGUFP_CUT_BATCH', 'default')} inc={inc:.3f} k_relax={ms_relax:.2f} ms "
          f"emit={ms_emit:.3f} ms wall={wall * 1e3:.2f} ms")
    print(f"status {dict(zip(*np.unique(st, return_counts=True)))} exact={int(ex.sum())}")
    if hasattr(eng.lib, "sgufp_relax_launches"):
        print(f"k_relax launches {eng.relax_launches()} (SGUFP_RELAX_CHUNK={os.environ.get('SGUFP_RELAX_CHUNK', 'default')}, "
              f"SGUFP_RELAX_STREAMS={os.environ.get('SGUFP_RELAX_STREAMS', 'default')})")
    # census of the DD templates' classes (Templates, dd_device.hpp): eligible records -- valid, not
    # bound-pruned (a staged batch prunes none), sol_len == gl -- by (g, mask, aligned)
    # (the state set stands for the mask; BFS children are valid records)
    sol_len = np.diff(fr.sol_off)
    classes = {}
    for k in range(fr.n):
        if sol_len[k] == fr.gl[k] and st[k] != 16:
            key = (int(fr.gl[k]), fr.states[fr.states_off[k]:fr.states_off[k + 1]].tobytes())
            classes[key] = classes.get(key, 0) + 1
    sizes = np.array(sorted(classes.values()), dtype=np.int64)
    hist = {int(s): int(c) for s, c in zip(*np.unique(sizes, return_counts=True))}
    shared = int(sizes[sizes >= 2].sum())
    print(f"template census: {int(sizes.sum())} eligible of {fr.n} records, {len(sizes)} distinct (g, mask, aligned) keys, "
          f"{shared} records ({100.0 * shared / max(1, fr.n):.1f} %) in classes >= 2; class size: classes {hist}")
    if hasattr(eng.lib, "sgufp_relax_templates"):
        built, copied = eng.relax_templates()
        print(f"templates built {built}, records instantiated {copied} "
              f"(SGUFP_RELAX_TEMPLATES={os.environ.get('SGUFP_RELAX_TEMPLATES', 'default')})")
    if args.dump:
        np.savez(args.dump, ticks=ticks, phases=eng.phases(), sweeps=sw, status=st, n_feas=16, n_opt=64,
                 ms_relax=ms_relax, nodes=args.nodes)
    print(f"wave us: mean {us.mean():.1f} p50 {np.median(us):.1f} p90 {np.percentile(us, 90):.1f} "
          f"max {us.max():.1f}; sum/CU(256) {us.sum() / 256 / 1e3:.2f} ms")
    print(f"dd nodes mean {dn.mean():.0f} max {dn.max()}; sweeps mean {sw.mean():.1f}; redo mean {redo.mean():.2f} "
          f"max {redo.max()}; stream {stream.mean():.2f} (entries mean {mirsz.mean():.0f} max {mirsz.max()}) "
          f"cap {eng.info.node_capacity}")
    for s in np.unique(st):
        m = st == s
        print(f"  status {s}: n={m.sum()} us/node {us[m].mean():.1f} sweeps {sw[m].mean():.1f} "
              f"us/sweep {np.mean(us[m] / np.maximum(sw[m], 1)):.2f} redo {redo[m].mean():.2f}")
    slow = us >= np.percentile(us, 90)
    print(f"redo per record: mean {redo.mean():.2f} max {redo.max()} slowest decile mean {redo[slow].mean():.2f} "
          f"(sweeps {sw[slow].mean():.1f}, us {us[slow].mean():.0f}); records with a redo {np.mean(redo > 0):.3f}")
    ph = eng.phases() / 100.0
    names = ["build", "narrow", "tail", "last", "post", "redo", "finish", "epilog"]
    print("phase us/node: " + ", ".join(f"{nm} {ph[:, k].mean():.0f}" for k, nm in enumerate(names)))
    ns = eng.narrow_split() / 100.0
    print("narrow us/node: " + ", ".join(f"{nm} {ns[:, k].mean():.0f}" for k, nm in enumerate(["merged layers", "group switches", "folded runs"])))
    if args.refold:
        # depth = tree layers folded again between the nearest width-1 summary and the parent
        # layer of a firing merged layer (Engine.refold_stats)
        rs = eng.refold_stats().astype(np.int64)
        hist = rs[:, 6:].sum(0)
        n_ref = int(rs[:, 0].sum())
        p90 = int(np.searchsorted(np.cumsum(hist), 0.9 * n_ref)) if n_ref else 0
        print(f"refolds per record: mean {rs[:, 0].mean():.2f} max {rs[:, 0].max()}; per redo with one "
              f"{n_ref / max(1, rs[:, 5].sum()):.2f} (most {rs[:, 3].max()}); redos with a refold {rs[:, 5].sum()} of {redo.sum()}; "
              f"in feasibility batches {rs[:, 4].sum()}")
        print(f"refold depth (layers): mean {rs[:, 1].sum() / max(1, n_ref):.2f} p90 {p90}{'+' if p90 >= 9 else ''} "
              f"max {rs[:, 2].max()}; layers refolded per record {rs[:, 1].mean():.1f}; histogram 0..9+ {hist.tolist()}")
    big = np.argsort(-us)[:5]
    for k in big:
        print(f"  slow node {k}: {us[k]:.0f} us, dd {dn[k]} nodes, {dl[k]} layers, sweeps {sw[k]}, status {st[k]}, "
              f"redo {redo[k]}")


if __name__ == "__main__":
    main()
