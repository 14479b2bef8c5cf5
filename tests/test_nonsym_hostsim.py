"""CPU: nonsym_driver (Fortran driver + dla_geev + host logic) on the host-memory engine (tests/hostsim.py) with host callbacks,
every case of tests/nonsym_cases.py, against the truth (the spectrum of the untransformed matrix) and against what the unmodified
reference returned on the same inputs (tests/golden/reference_nonsym_fixtures.npz).

One worker process runs all solves (the host-simulation library takes the place of the HIP library in a process) and leaves its
results in a file; the tests read it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import nonsym_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_nonsym_fixtures.npz")
RESTART_CASE = nc.RESTART_CASE

WORKER = r"""
import os, sys
os.environ.setdefault("OMP_NUM_THREADS", "2")
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import hostsim, nonsym_cases as nc
from diaglib_amd import capi
capi.load(hostsim.build())
ctx = capi.Context()
assert ctx.backend.startswith("hostsim")
fix = np.load({fixture!r})
out = {{}}

def solve(case, side, u, v):
    n, n_targ, n_max, max_dav, tol, _, t = case
    a, a0 = nc.matrix(n, t, u, v)
    at = np.asfortranarray(a.T)
    cols = [0, 0]
    def mv(x):
        cols[0] += x.shape[1]; return a @ x
    def mvl(x):
        cols[1] += x.shape[1]; return at @ x
    g = nc.guess(n, n_max)
    eig, r, l, ok, info = ctx.nonsym_driver(n, n_targ, n_max, nc.MAX_ITER, tol, max_dav, 0.0, mv, mvl,
                                            nc.mprec(np.diag(a).copy()), g, g, side)
    return dict(eig=eig, r=r, l=l, ok=ok, cols=np.array(cols), info=np.array([info["iters"], info["matvec_cols"], info["restarts"]]))

for case in nc.CASES + [nc.RESTART_CASE]:
    name = nc.case_name(case)
    u, v = fix[name + "__u"], fix[name + "__v"]
    res = solve(case, case[5], u, v)
    for k, val in res.items():
        out[name + "__" + k] = val
    again = solve(case, case[5], u, v)
    out[name + "__repeat"] = all(np.array_equal(res[k], again[k]) for k in res)
    if case[5] == "c":
        other = solve(case, "s", u, v)
        out[name + "__s_equals_c"] = all(np.array_equal(res[k], other[k]) for k in res)
np.savez({out!r}, **out)
"""

BAD_SIDE = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import hostsim, nonsym_cases as nc
from diaglib_amd import capi
capi.load(hostsim.build())
ctx = capi.Context()
g = nc.guess(20, 2)
f = lambda x: x
ctx.nonsym_driver(20, 2, 2, 10, 1e-6, 2, 0.0, f, f, lambda fac, x: x, g, g, "x")
print("returned")
"""


@pytest.fixture(scope="module")
def fix():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("nonsym")
    out = str(d / "runs.npz")
    script = d / "worker.py"
    script.write_text(WORKER.format(root=ROOT, fixture=FIXTURE, out=out))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    return np.load(out)


def check_case(case, get, fix):
    """the checks of one solve, shared with the GPU test: `get(key)` returns eig, r, l, ok, cols of the run"""
    n, n_targ, n_max, max_dav, tol, side, t = case
    name = nc.case_name(case)
    a, a0 = nc.matrix(n, t, fix[name + "__u"], fix[name + "__v"])
    tr = nc.truth(a0)
    eig, r, l = get("eig"), get("r"), get("l")
    assert bool(get("ok"))
    err = np.abs(eig[:n_targ] - tr[:n_targ]).max()
    print(f"{name}: eig error {err:.2e}, matvec columns {get('cols')} (reference {fix[name + '__cols']})")
    # Bauer-Fike with an rms residual below tol: |eig - truth| <= cond(eigenvectors) sqrt(n) tol, cond <= (1 + t)^2
    assert err <= (1 + t) ** 2 * np.sqrt(n) * tol
    if side == "r":
        res = nc.rms_residuals(a, r, eig, n_targ)
        print("   rms residuals", res)
        assert res.max() <= 2 * tol
    elif side == "l":
        res = nc.rms_residuals(a.T, l, eig, n_targ)
        print("   rms residuals", res)
        assert res.max() <= 2 * tol
    else:
        bi = nc.biorth_error(l, r)
        print(f"   max |L^T R - I| {bi:.2e} (reference {float(fix[name + '__biorth']):.2e})")
        assert bi <= max(100 * float(fix[name + "__biorth"]), n * EPS)
        if n_targ == n_max:
            sub, ref = nc.subspace_residual(a, l, r), float(fix[name + "__subres"])
            small = np.sort(np.linalg.eigvals(l.T @ a @ r).real)
            print(f"   subspace residual {sub:.2e} (reference {ref:.2e}), eig(L^T A R) - eig {np.abs(small - np.sort(eig)).max():.2e}")
            assert sub <= 10 * ref
            assert np.abs(small - np.sort(eig)).max() <= 10 * ref
    assert int(get("cols").sum()) <= 1.25 * int(fix[name + "__cols"].sum()) + n_max


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_name)
def test_case_against_truth_and_reference(runs, fix, case):
    name = nc.case_name(case)
    check_case(case, lambda k: runs[name + "__" + k], fix)
    iters, cols, restarts = runs[name + "__info"]
    assert cols == runs[name + "__cols"].sum()                # the solve report counts both passes
    assert bool(runs[name + "__repeat"])                      # a repeated solve is bit-identical
    if case[5] == "c":
        assert bool(runs[name + "__s_equals_c"])              # 's' is 'c', bit for bit


def test_restarts(runs, fix):
    name = nc.case_name(RESTART_CASE)
    check_case(RESTART_CASE, lambda k: runs[name + "__" + k], fix)
    assert runs[name + "__info"][2] >= 2                      # both passes ran into a full basis
    assert bool(runs[name + "__repeat"]) and bool(runs[name + "__s_equals_c"])


def test_invalid_side_ends_the_process_with_the_reference_message(tmp_path):
    script = tmp_path / "bad_side.py"
    script.write_text(BAD_SIDE.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "choice for side is not correct. can be r,l,s,c." in p.stdout + p.stderr
    assert "returned" not in p.stdout
