"""Subprocess helper for tests/test_subproblem_exhaustive.py: every matching of a data family's
network through the warm-start kernels, in two calls.  The library is the one SGUFP_LIB_PATH names.

    sub_warm_chain.py cfg seed S family out.npz

Call 1 solves the even-numbered matchings of the enumeration cold and stores their states in
ring slots 0, 1, ...; call 2 solves the odd-numbered ones, each from its predecessor's slot."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(cfg, seed, S, family, out):
    from oracle import subproblem_oracle as so
    from sgufp_solver_amd import engine as E
    from tests.helpers import sub_families as fam
    from tests.helpers.matchings import all_matchings
    from tests.test_subproblem import _keys, _path_of
    inst = fam.make(cfg, seed, S, family)
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_subw_"), "net.txt")
    inst.write(path)
    net = so.from_instance(inst, E.probe_network(path)[1])
    paths = [_path_of(inst, net, y) for y in all_matchings(inst)]
    even, odd = paths[0::2], paths[1::2]
    eng = E.Engine(path, 0, max(len(even), 32))
    res = {"keys": np.array(_keys(eng), dtype=np.int64).reshape(-1, 3), "layers": np.array(eng.info.total_layers)}
    names = ("typ", "rhs", "rows", "obj_mean", "st", "obj", "dual")
    cold = eng.subproblem(even, [-1] * len(even), list(range(len(even)))) + eng.subproblem_detail(len(even))
    warm = eng.subproblem(odd, list(range(len(odd))), [-1] * len(odd)) + eng.subproblem_detail(len(odd))
    res["warm_aug"], _ = eng.subproblem_stats(len(odd))
    eng.close()
    for half, vals in (("cold", cold), ("warm", warm)):
        for name, v in zip(names, vals):
            res[f"{half}_{name}"] = v
    np.savez(out, lib=np.array(E.LIB_PATH), **res)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
