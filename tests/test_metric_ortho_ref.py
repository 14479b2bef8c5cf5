"""CPU: what tests/test_metric_ortho_gpu.py rests on, shown without a GPU (tests/metric_ortho_ref.py holds references, cases, checkers).

1. The long-double references reproduce what the UNMODIFIED reference computed (the bo_* entries of tests/golden/reference_fixtures.npz)
   within the checkers' own bounds.
2. On every case of the GPU test the double-precision oracle (b_ortho_vs_x, then b_ortho on B @ u from scipy; b_ortho alone for the
   direct cases) passes the same checkers with a worst ratio of 0.25: the bounds leave the device a factor 4 over what double
   arithmetic in the reference's own order achieves.  A condition on the inputs, not on the library.
3. The generators deliver what they promise.
4. The same cases through the product's host logic (dla_b_ortho: dla_potrf_lower, dla_trtri_lower, the explicit-inverse update;
   dla_b_ortho_vs_x; dla_expand_project_metric modes 0 to 2 with its error return) on the host-memory engine, in a worker process
   (tests/hostsim.py; the library a process has loaded cannot be exchanged).  That engine stores no metric: B and A are ctypes
   callbacks that call scipy.

$DIAGLIB_METRIC_ORTHO_RECORD names a file the worst ratios of every case are appended to (profiles/metric_ortho.txt)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import metric_ortho_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.environ.get("DIAGLIB_METRIC_ORTHO_RECORD")
EPS = R.EPS

B_ORTHO_ALL = list(dict.fromkeys(R.B_ORTHO_CASES + [R.B_ORTHO_FEW_ROWS, R.B_ORTHO_VIEWS] + R.B_ORTHO_WIDE))    # (the views' block is one of the matrix)
BLOCK_CASES = list(dict.fromkeys(R.VS_X_CASES + [key for key, _ in R.EXPAND_CASES]))     # (each block once, whatever the mode)


@pytest.fixture(scope="module")
def cases():
    """every case with its references, built once (the worker of test 4 reads them from a file instead of computing them again)"""
    for key in B_ORTHO_ALL:
        R.case(*key).ref_b_ortho()
    for key in BLOCK_CASES:
        R.case(*key).ref_expand(); R.case(*key).ref_vs_x()
    return R


# ------------------------------------------------------------------------------------------------------------------ 1. the golden fixture
def test_references_reproduce_the_unmodified_reference():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "reference_fixtures.npz"))
    x, bx, u = gold["bo_x"], gold["bo_bx"], gold["bo_u"]
    c = types.SimpleNamespace(x=x, bx=bx, m=x.shape[1])
    rv = R.ref_b_ortho_vs_x(x, bx, u)
    r1 = R.check_b_ortho_vs_x(gold["bo_vsx_out"], rv, c, what="golden b_ortho_vs_x")
    rb = R.ref_b_ortho(gold["bo_vsx_out"], gold["bo_bu"])
    r2 = R.check_b_ortho(gold["bo_u_out"], gold["bo_bu_out"], rb, what="golden b_ortho")
    R.record(RECORD, [("reference golden_vs_x", r1), ("reference golden_b_ortho", r2)])
    # the fixture is a well-conditioned one: the bounds it is held to are tight ones
    assert rb.kappa < 10 and rv.pi * rv.a < 10


# ------------------------------------------------------------------------------------------------------------------ 2. the oracle at a quarter
def test_oracle_b_ortho_meets_a_quarter_of_every_bound(cases, oracle):
    rows = []
    for key in B_ORTHO_ALL:
        c = R.case(*key)
        q, bq = oracle.b_ortho(c.u, c.bu)
        rows.append(("oracle b_ortho " + c.name, R.check_b_ortho(q, bq, c.ref_b_ortho(), what=c.name, limit=0.25)))
    R.record(RECORD, rows)


def test_oracle_vs_x_and_expansion_meet_a_quarter_of_every_bound(cases, oracle):
    rows = []
    for key in BLOCK_CASES:
        c = R.case(*key)
        q1, st = oracle.b_ortho_vs_x(c.x, c.bx, c.u)
        assert st == 0
        rows.append(("oracle vs_x " + c.name, R.check_b_ortho_vs_x(q1, c.ref_vs_x(), c, what=c.name, limit=0.25)))
        q, bq = oracle.b_ortho(q1, np.asfortranarray(c.b @ q1))
        rows.append(("oracle expand " + c.name, R.check_expand(q, bq, c.ref_expand(), c, what=c.name, limit=0.25)))
    R.record(RECORD, rows)


# ------------------------------------------------------------------------------------------------------------------ 3. the generators
def test_generators_deliver_what_they_promise(cases):
    seen = {"mix": 0, "near_span": 0, "x": 0}
    for key in B_ORTHO_ALL + BLOCK_CASES:
        c = R.case(*key)
        direct = key in B_ORTHO_ALL
        # (a 1 x 1 Gram matrix has condition 1, and the unscaled metric has no spread to select from)
        if c.kind == "mix" and c.metric_name == "scaled" and c.k >= 2:
            kappa = (c.ref_b_ortho() if direct else c.ref_expand()).kappa
            assert 1e3 <= kappa <= 1e6, (c.name, kappa)
            seen["mix"] += 1
        if c.kind == "near_span":
            assert c.ref_vs_x().a >= 1e5, (c.name, c.ref_vs_x().a)
            seen["near_span"] += 1
        if c.kind == "colscaled":
            r = c.ref_b_ortho()
            assert r.kappa > 1e25 and r.kappa_eq < 10, (c.name, r.kappa, r.kappa_eq)
        if c.m:
            xl = np.asarray(c.x, R.LD)
            dev = np.abs(xl.T @ R.bmul(c.b, xl) - np.eye(c.m)).max()
            assert dev <= 8 * EPS * c.ref_vs_x().pi, (c.name, float(dev))
            seen["x"] += 1
    assert seen["mix"] >= 20 and seen["near_span"] == 3 and seen["x"] == sum(1 for key in BLOCK_CASES if key[1]), seen


def test_the_indefinite_blocks_are_what_the_error_path_needs():
    b, x, bx, u = R.indef_blocks()
    n, m, k = R.INDEF_CASE
    xl = np.asarray(x, R.LD)
    assert np.abs(xl.T @ R.bmul(b, xl) - np.eye(m)).max() <= 8 * EPS * np.linalg.norm(x, 2) * np.linalg.norm(bx, 2)
    with pytest.raises(np.linalg.LinAlgError):
        R.ref_b_ortho(u, b @ u)
    q1 = R.ref_b_ortho_vs_x(x, bx, u).q
    with pytest.raises(np.linalg.LinAlgError):
        R.chol_lower(q1.T @ R.bmul(b, q1))


# ------------------------------------------------------------------------------------------------------------------ 4. the host logic
WORKER = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import hostsim
import metric_ortho_ref as R
from diaglib_amd import capi
capi.load(hostsim.build())
R.load_cases({cases!r})
ctx = capi.Context()
assert ctx.backend.startswith("hostsim")
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)          # (this engine's "device" blocks are host memory: the callbacks see them directly)
mats = {{}}

def callback(which):
    def cb(pn, pm, px, py):
        n, m = pn[0], pm[0]
        x, y = np.ctypeslib.as_array(px, (m, n)).T, np.ctypeslib.as_array(py, (m, n)).T
        y[:, :] = mats[which] @ x
    return capi.MATVEC_T(cb)

cb_a, cb_b = callback("a"), callback("b")
fn_a, fn_b = C.cast(cb_a, C.c_void_p).value, C.cast(cb_b, C.c_void_p).value
out = {{}}
MSG = "b_ortho: metric not positive definite"

def expand(c, mode, x=None, bx=None, u=None):
    x, bx, u = (c.x, c.bx, c.u) if x is None else (x, bx, u)
    n, m = x.shape
    k = u.shape[1]
    shift = R.SHIFT[mode]
    ax = np.asfortranarray(mats["a"] @ x + shift * x)
    basis = ctx.panel(np.asfortranarray(np.hstack([x, u])))
    bbasis = ctx.panel(np.asfortranarray(np.hstack([bx, np.zeros((n, k))])))
    abasis = ctx.panel(np.asfortranarray(np.hstack([ax, np.zeros((n, k))])))
    h = np.zeros((m + k, k if mode == 0 else m + k), order="F")
    st = ctx.lib.dla_expand_project_metric(ctx.h, mode, n, m, k, basis.ptr, bbasis.ptr, abasis.ptr, fn_a, fn_b, shift,
                                           h.ctypes.data_as(capi.c_dp), m + k)
    return st, basis.download(), bbasis.download(), abasis.download(), h, ax

# ---- dla_b_ortho: Gram matrix, dla_potrf_lower, dla_trtri_lower, the explicit-inverse update of both blocks
for key in {b_ortho_all!r}:
    c = R.case(*key)
    pu, pbu = ctx.panel(c.u), ctx.panel(c.bu)
    ctx.b_ortho(pu, pbu)
    out["hostsim b_ortho " + c.name] = R.check_b_ortho(pu.download(), pbu.download(), c.ref_b_ortho(), what=c.name)

# ---- dla_b_ortho_vs_x: X and U in separate panels, and U behind X in one panel (the pending last factor of the combined sweep)
for key in {vs_x!r}:
    c = R.case(*key)
    got = []
    for one_panel in (False, True):
        pbx = ctx.panel(c.bx)
        if one_panel:
            p = ctx.panel(np.asfortranarray(np.hstack([c.x, c.u]))); px, pu = p.col(0, c.m), p.col(c.m, c.k)
        else:
            px, pu = ctx.panel(c.x), ctx.panel(c.u)
        ctx.b_ortho_vs_x(px, pbx, pu)
        got.append(pu.download())
        out[f"hostsim vs_x panels={{2 - one_panel}} " + c.name] = R.check_b_ortho_vs_x(got[-1], c.ref_vs_x(), c, px.download(), pbx.download(), what=c.name)
    rv = c.ref_vs_x()
    assert np.abs(got[0] - got[1]).max() <= 64 * R.EPS * rv.pi * rv.a, c.name

# ---- dla_expand_project_metric, modes 0 to 2
for key, mode in {expand!r}:
    c = R.case(*key)
    mats["a"], mats["b"] = R.operator(c.n), c.b
    st, gb, gbb, gab, h, ax = expand(c, mode)
    assert st == 0, (c.name, mode, ctx.lib.dla_last_error(ctx.h).decode())
    out[f"hostsim expand mode={{mode}} " + c.name] = R.check_expand(gb[:, c.m:], gbb[:, c.m:], c.ref_expand(), c, mode, mats["a"], R.SHIFT[mode], ax,
                                                                  gab[:, c.m:], h, gb[:, :c.m], what=f"{{c.name}} mode {{mode}}")
    assert np.array_equal(gbb[:, :c.m], c.bx)

# ---- the metric that is not positive definite: DLA_ERR_LAPACK with its text, and the context goes on working
b, x, bx, u = R.indef_blocks()
n, m, k = R.INDEF_CASE
mats["a"], mats["b"] = R.operator(n), b
pu, pbu = ctx.panel(u), ctx.panel(np.asfortranarray(b @ u))
assert ctx.lib.dla_b_ortho(ctx.h, n, k, pu.ptr, pbu.ptr) == capi.ERR_LAPACK and ctx.lib.dla_last_error(ctx.h).decode() == MSG
for mode in (2, 0):
    st = expand(None, mode, x, bx, u)[0]
    assert st == capi.ERR_LAPACK and ctx.lib.dla_last_error(ctx.h).decode() == MSG, (mode, st)
key, mode = {expand!r}[0]
c = R.case(*key)
mats["a"], mats["b"] = R.operator(c.n), c.b
st, gb, gbb, gab, h, ax = expand(c, mode)
assert st == 0
R.check_expand(gb[:, c.m:], gbb[:, c.m:], c.ref_expand(), c, mode, what="after the error return")
with open({out!r}, "w") as f:
    json.dump(out, f)
print("host logic: ok")
"""


def test_the_host_logic_passes_the_same_checkers_on_the_host_engine(cases, tmp_path):
    cases_file, out_file = str(tmp_path / "cases.pkl"), str(tmp_path / "ratios.json")
    R.dump_cases(cases_file)
    script = tmp_path / "metric_ortho_worker.py"
    script.write_text(WORKER.format(root=ROOT, cases=cases_file, out=out_file, b_ortho_all=B_ORTHO_ALL, vs_x=R.VS_X_CASES,
                                    expand=R.EXPAND_CASES))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "host logic: ok" in p.stdout
    with open(out_file) as f:
        ratios = json.load(f)
    assert len(ratios) == len(B_ORTHO_ALL) + 2 * len(R.VS_X_CASES) + len(R.EXPAND_CASES)
    R.record(RECORD, sorted(ratios.items()))
