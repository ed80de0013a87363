"""The C++ host API's routing, bound and flows (Inavap::DDSolver::bestPath / bestBound /
openNodes / gap, Inavap::GuroSolver::solveFlows; tests/host/solution_test.cpp).

CPU: the host library exports the new members and the driver was built.  GPU: on T4-3-3 the
C++ solver's value equals the Python driver's bit for bit (the same rounds on the same
library), its routing gives that value back through the device subproblem within 1e-9
relative (tests/test_subproblem.py's tolerance), and its bound equals its value.
"""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sgufp_solver_amd", "lib")


def test_host_library_exports_the_solution_api(native_lib):
    out = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(LIB, "libsgufp_host.so")],
                         capture_output=True, text=True, check=True).stdout
    for sym in ["Inavap::DDSolver::gap(", "Inavap::GuroSolver::solveFlows("]:
        assert sym in out, sym
    assert os.access(os.path.join(LIB, "solution_test"), os.X_OK)


def _run(args):
    r = subprocess.run([os.path.join(LIB, "solution_test")] + args, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    out = {"flows": []}
    for line in r.stdout.splitlines():
        p = line.split()
        if p[0] == "solution":
            out.update(value=float.fromhex(p[1]), bound=float.fromhex(p[2]), open=int(p[3]), complete=int(p[4]),
                       gap=float.fromhex(p[5]))
        elif p[0] == "path":
            out["path"] = [int(x) for x in p[2:]]
            assert len(out["path"]) == int(p[1])
        elif p[0] == "flows":
            out["flows"].append((int(p[1]), int(p[2]), int(p[3])))
    return out


@pytest.mark.gpu
def test_cpp_solution_matches_the_python_driver():
    from sgufp_solver_amd import instance
    from sgufp_solver_amd.pools import DOUBLE_MIN
    from sgufp_solver_amd.solver import DDSolver
    inst = instance.generate(instance.CONFIGS["T4"], 3, scenarios=3)
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_hsol_"), "net.txt")
    inst.write(path)
    got = _run([path, "none"])
    solver = DDSolver(path, verbose=False, max_rounds=20000)
    try:
        z = solver.start_solver(DOUBLE_MIN)
        r = solver.result()
        print(f"C++ value {got['value']!r} bound {got['bound']!r}; Python value {z!r}")
        assert got["value"].hex() == z.hex()
        assert got["complete"] == 1 and got["bound"] == got["value"] and got["open"] == 0 and got["gap"] == 0.0
        assert 0 < len(got["path"]) <= solver.eng.info.total_layers
        typ, _, _, obj_mean = solver.eng.subproblem([got["path"]])
        assert typ[0] == 0 and abs(obj_mean[0] - got["value"]) <= 1e-9 * max(1.0, abs(got["value"]))
        assert got["path"] == r.path          # the same rounds close the same leaf
        # GuroSolver::solveFlows on that routing: every scenario optimal, the flows of the Python engine
        st, _, _, x, _ = solver.eng.subproblem_flows([got["path"]])
        assert got["flows"] == [(s, int(st[0, s]), int(x[0, s].sum())) for s in range(3)]
        assert all(f[1] == 0 for f in got["flows"])
    finally:
        solver.eng.close()


@pytest.mark.gpu
def test_cpp_solution_stopped_early_reports_a_gap():
    from oracle import extensive_form as ef
    from sgufp_solver_amd import instance
    inst = instance.generate(instance.CONFIGS["T4"], 3, scenarios=3)
    path = os.path.join(tempfile.mkdtemp(prefix="sgufp_hsol_"), "net.txt")
    inst.write(path)
    opt = ef.solve(inst)
    got = _run([path, "none", "1"])
    tol = 1e-5 * max(1.0, abs(opt))
    if got["complete"]:
        assert got["gap"] == 0.0 and got["open"] == 0
    else:
        assert got["open"] > 0 and got["value"] <= opt + tol and opt <= got["bound"] + tol
        assert got["gap"] > 0
