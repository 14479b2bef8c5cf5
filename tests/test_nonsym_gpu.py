"""GPU: nonsym_driver in device mode -- the cases and the checks of tests/test_nonsym_hostsim.py with the whole solve in HBM: the
matrix is stored once (dla_dense_setup) and the operators are dla_dense_matvec, dla_dense_matvec_t (the transposed product from the
same copy) and dla_dense_precnd.  One case also runs with the explicitly transposed array in the metric slot and dla_dense_bvec as
matvec_l, under the same bounds: that run does not touch the transposed kernel, so it separates the driver from it."""
import os

import numpy as np
import pytest

import nonsym_cases as nc
from diaglib_amd import capi
from test_nonsym_hostsim import FIXTURE, check_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return np.load(FIXTURE)


@pytest.fixture(autouse=True)
def _device_callbacks_and_empty_slots(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield
    ctx.dense_drop(False)
    ctx.dense_drop(True)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.set_option(capi.OPT_EVEC_ON_DEVICE, 0)


def solve(ctx, case, fix, left="dla_dense_matvec_t", side=None, evec_on_device=True):
    n, n_targ, n_max, max_dav, tol, case_side, t = case
    name = nc.case_name(case)
    a, _ = nc.matrix(n, t, fix[name + "__u"], fix[name + "__v"])
    ctx.dense_setup(a)
    if left == "dla_dense_bvec":
        ctx.dense_setup(np.asfortranarray(a.T), metric=True)
    mv, mvl, pc = (capi.fn_address(f) for f in ("dla_dense_matvec", left, "dla_dense_precnd"))
    g = nc.guess(n, n_max)
    r, l = (ctx.panel(g), ctx.panel(g)) if evec_on_device else (g, g)
    eig, r, l, ok, info = ctx.nonsym_driver(n, n_targ, n_max, nc.MAX_ITER, tol, max_dav, 0.0, mv, mvl, pc, r, l, side or case_side)
    if evec_on_device:
        rp, lp = r, l
        r, l = rp.download(), lp.download()
        rp.free(); lp.free()
    return dict(eig=eig, r=r, l=l, ok=ok, cols=np.array([info["matvec_cols"]]), info=info)


@pytest.mark.parametrize("case", nc.CASES + [nc.RESTART_CASE], ids=nc.case_name)
def test_case_in_device_mode(ctx, fix, case):
    res = solve(ctx, case, fix)
    check_case(case, res.__getitem__, fix)
    if case == nc.RESTART_CASE:
        assert res["info"]["restarts"] >= 2


def test_host_eigenvector_blocks_repeat_and_s_is_c(ctx, fix):
    """device callbacks with the eigenvector blocks on the host; a repeated solve and side = 's' return the same bits"""
    case = nc.CASES[0]
    first = solve(ctx, case, fix, evec_on_device=False)
    check_case(case, first.__getitem__, fix)
    for other in (solve(ctx, case, fix, evec_on_device=False), solve(ctx, case, fix, side="s"), solve(ctx, case, fix)):
        assert all(np.array_equal(first[k], other[k]) for k in ("eig", "r", "l", "cols"))


def test_one_case_with_the_transposed_array_in_the_metric_slot(ctx, fix):
    case = nc.CASES[3]
    check_case(case, solve(ctx, case, fix, left="dla_dense_bvec").__getitem__, fix)
