"""GPU: the metric (B-) orthogonalisation -- dla_b_ortho, dla_b_ortho_vs_x and the fused dla_expand_project_metric (modes 0, 1 and 2) --
against the long-double references of tests/metric_ortho_ref.py, with bounds that follow each case's conditioning (kappa_2 of the Gram
matrix that is factored, the norm pi of the oblique projector, the cancellation a of the projection; see that module).  The CPU
test tests/test_metric_ortho_ref.py shows on the same cases that the double-precision oracle meets a quarter of every bound.

What runs here and nowhere else at kernel level:
  * bortho_tail_kernel, the one-wave device step of b_ortho (lds_potrf, lds_trtri, W = L^-T packed as [kt][k4][16] for the two predicated
    triangular updates): one column, widths that are no multiple of 4 (k4 padded), the tile edges 15/16/17, 31/32/33, 47/48, behind a
    chain (need_chain) and without one (m = 0), a metric that is not positive definite (status -seq) and the call after it;
    k = 49 declines and takes the host step with the wide triangular update;
  * the device chain with a metric (measures against BX, updates with X; last factor dropped under ChainPolicy::metric_drop());
  * mode 2, the linear-response expansion.
The metrics are sparse: Context.spmm_setup_metric and dla_spmm_bvec; A is dla_spmm_matvec on a second sparse matrix.

$DIAGLIB_METRIC_ORTHO_RECORD names a file the worst ratios error / bound of every case are appended to (profiles/metric_ortho.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import metric_ortho_ref as R
from diaglib_amd import capi

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("DIAGLIB_METRIC_ORTHO_RECORD")
TUNE6 = 100 + 6
MSG = "b_ortho: metric not positive definite"
GUARD = 1e30


def ident(key):
    return "-".join(str(v) for v in key)


@pytest.fixture()
def dev(ctx):
    """device callbacks on; the session's context goes back as tests/conftest.py expects it, without a metric"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(TUNE6, 0)
    ctx.set_option(capi.OPT_RUN_AHEAD, 1)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.set_shard(-1, 0)
    ctx.spmm_drop_metric()


def tail_launches(ctx):
    """launches of the device step of b_ortho so far (the name the engine books it under)"""
    buf = (capi.KernelStat * 1024)()
    n = ctx.lib.dla_get_kernel_stats(ctx.h, C.cast(buf, C.POINTER(capi.KernelStat)), 1024)
    return sum(int(buf[j].launches) for j in range(n) if buf[j].name.decode() == "bortho_tail_kernel")


# ------------------------------------------------------------------------------------------------------------------ 1. b_ortho
@pytest.mark.parametrize("key", R.B_ORTHO_CASES + [R.B_ORTHO_FEW_ROWS] + R.B_ORTHO_WIDE, ids=ident)
def test_b_ortho_against_the_long_double_cholesky_qr(ctx, key):
    """the host step over the device Gram and triangular-update kernels, the pair (U, BU) as given; the widths above 48 take the
    triangular update in column blocks from right to left"""
    c = R.case(*key)
    pu, pbu = ctx.panel(c.u), ctx.panel(c.bu)
    ctx.b_ortho(pu, pbu)
    ratios = R.check_b_ortho(pu.download(), pbu.download(), c.ref_b_ortho(), what=c.name)
    R.record(RECORD, [("device b_ortho " + c.name, ratios)])


def test_b_ortho_on_column_views_between_guard_columns(ctx):
    """U and BU as views at an odd column offset of wider panels (n odd: the blocks are 8-byte aligned only), 1e30 on both sides"""
    c = R.case(*R.B_ORTHO_VIEWS)
    wall = np.full((c.n, 1), GUARD)
    pu = ctx.panel(np.asfortranarray(np.hstack([wall, c.u, wall])))
    pbu = ctx.panel(np.asfortranarray(np.hstack([wall, wall, wall, c.bu, wall])))
    ctx.b_ortho(pu.col(1, c.k), pbu.col(3, c.k))
    gu, gbu = pu.download(), pbu.download()
    assert np.all(gu[:, [0, -1]] == GUARD) and np.all(gbu[:, [0, 1, 2, -1]] == GUARD)
    ratios = R.check_b_ortho(gu[:, 1:-1], gbu[:, 3:-1], c.ref_b_ortho(), what=c.name + " (views)")
    R.record(RECORD, [("device b_ortho views " + c.name, ratios)])


# ------------------------------------------------------------------------------------------------------------------ 2. b_ortho_vs_x
def _vs_x(ctx, c, one_panel):
    pbx = ctx.panel(c.bx)
    if one_panel:
        p = ctx.panel(np.asfortranarray(np.hstack([c.x, c.u])))
        px, pu = p.col(0, c.m), p.col(c.m, c.k)
    else:
        px, pu = ctx.panel(c.x), ctx.panel(c.u)
    ctx.b_ortho_vs_x(px, pbx, pu)
    return pu.download(), px.download(), pbx.download()


@pytest.mark.parametrize("key", R.VS_X_CASES, ids=ident)
def test_b_ortho_vs_x_on_both_routes(ctx, key):
    """X and U in separate panels (the host-driven loop) and U behind X in one panel with BX in a second one (the device chain, under
    the schedules of tune knob 6: default, five-sweep, three-pass): every route passes the checker, and they agree with each other
    within the bound on |Q - Q_ref|"""
    c = R.case(*key)
    ref = c.ref_vs_x()
    rows, got = [], {}
    try:
        for route, knob in (("separate", 0), ("chain", 0), ("chain", 12), ("chain", 13)):
            ctx.set_option(TUNE6, knob)
            q, x_after, bx_after = _vs_x(ctx, c, route == "chain")
            what = f"{c.name} {route} knob6={knob}"
            rows.append(("device vs_x " + what, R.check_b_ortho_vs_x(q, ref, c, x_after, bx_after, what=what)))
            got[(route, knob)] = q
    finally:
        ctx.set_option(TUNE6, 0)
    for other in list(got)[1:]:
        assert np.abs(got[other] - got[("separate", 0)]).max() <= 64 * R.EPS * ref.pi * ref.a, (c.name, other)
    R.record(RECORD, rows)


def test_b_ortho_vs_x_on_a_rank_deficient_block(ctx):
    """last column = the sum of the first two: no unique answer, the invariants only"""
    c = R.case(*R.VS_X_RANK_DEFICIENT)
    rows = []
    for one_panel in (False, True):
        q, x_after, bx_after = _vs_x(ctx, c, one_panel)
        what = f"{c.name} panels={2 - one_panel}"
        rows.append(("device vs_x " + what, R.check_b_ortho_vs_x(q, None, c, x_after, bx_after, what=what, vs_reference=False)))
    R.record(RECORD, rows)


# ------------------------------------------------------------------------------------------------------------------ 3. the expansion
def _expand(ctx, mode, a, x, bx, u, ahead):
    n, m = x.shape
    k = u.shape[1]
    shift = R.SHIFT[mode]
    ax = np.asfortranarray(a @ x + shift * x)
    ctx.set_option(capi.OPT_RUN_AHEAD, ahead)
    basis = ctx.panel(np.asfortranarray(np.hstack([x, u])))
    bbasis = ctx.panel(np.asfortranarray(np.hstack([bx, np.zeros((n, k))])))
    abasis = ctx.panel(np.asfortranarray(np.hstack([ax, np.zeros((n, k))])))
    h = np.zeros((m + k, k if mode == 0 else m + k), order="F")
    t0, s0 = tail_launches(ctx), ctx.stats()["host_syncs"]
    st = ctx.lib.dla_expand_project_metric(ctx.h, mode, n, m, k, basis.ptr, bbasis.ptr, abasis.ptr, capi.fn_address("dla_spmm_matvec"),
                                           capi.fn_address("dla_spmm_bvec"), shift, h.ctypes.data_as(capi.c_dp), m + k)
    syncs, tails = ctx.stats()["host_syncs"] - s0, tail_launches(ctx) - t0
    return dict(st=st, msg=ctx.lib.dla_last_error(ctx.h).decode(), basis=basis.download(), bbasis=bbasis.download(),
                abasis=abasis.download(), h=h, ax=ax, syncs=syncs, tails=tails)


def _check_expand(c, mode, a, r, what):
    assert r["st"] == 0, (what, r["st"], r["msg"])
    assert np.array_equal(r["bbasis"][:, :c.m], c.bx) and np.array_equal(r["abasis"][:, :c.m], r["ax"]), what
    return R.check_expand(r["basis"][:, c.m:], r["bbasis"][:, c.m:], c.ref_expand(), c, mode, a, R.SHIFT[mode], r["ax"],
                          r["abasis"][:, c.m:], r["h"], r["basis"][:, :c.m], what=what)


@pytest.mark.parametrize("key,mode,fmt", [(key, mode, "ell") for key, mode in R.EXPAND_CASES] + [(R.expand_width_case(16), 2, "sell"), (R.expand_width_case(17), 0, "sell")],
                         ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_expand_project_metric_against_the_long_double_reference(dev, key, mode, fmt):
    """run ahead of the chain's report (first call of the shape, then with its history), then one call after the other (the host step
    of b_ortho), then run ahead with the device step of b_ortho switched off (tune knob 6 = 11): all four pass the same checker.  For the plain random blocks the device
    step ran in the steady state -- its kernel was launched and the whole expansion cost fewer host waits than with the knob, under
    which it was not launched; k = 49 never launches it."""
    c = R.case(*key)
    a = R.operator(c.n)
    dev.spmm_setup(a, fmt=fmt)
    dev.spmm_setup_metric(c.b, fmt=fmt)
    assert dev.spmm_metric_info()["format"] == fmt
    rows, runs = [], []
    for ahead, knob in ((1, 0), (1, 0), (0, 0), (1, 11)):
        dev.set_option(TUNE6, knob)
        r = _expand(dev, mode, a, c.x, c.bx, c.u, ahead)
        what = f"{c.name} mode={mode} {fmt} ahead={ahead} knob6={knob} (host waits {r['syncs']}, device steps {r['tails']})"
        rows.append(("device expand " + what, _check_expand(c, mode, a, r, what)))
        runs.append(r)
    R.record(RECORD, rows)
    first, steady, in_turn, no_device_step = runs
    assert no_device_step["tails"] == 0
    if c.k > 48:
        assert all(r["tails"] == 0 for r in runs)               # the device step declines: the host step took every call
    elif c.kind == "random":
        assert first["tails"] == 1 and steady["tails"] == 1
        assert in_turn["tails"] == 0                             # (without the run-ahead the host step factors: the reference's order)
        assert steady["syncs"] < no_device_step["syncs"], (steady["syncs"], no_device_step["syncs"])
        if c.m:
            assert steady["syncs"] == 1, steady["syncs"]         # one host wait for the whole expansion once the plan holds


# ------------------------------------------------------------------------------------------------------------------ 4. the indefinite metric
def test_a_metric_that_is_not_positive_definite_is_reported_and_the_next_call_passes(dev):
    """through dla_b_ortho and through the expansion in mode 2 and mode 0, run-ahead on and off: DLA_ERR_LAPACK with its text each time;
    then a passing case on the same context (the status word, the word the updates are predicated on and the sequence number
    after a negative outcome).  An error RETURN of a one-wave kernel: nothing faults, each route runs once."""
    b, x, bx, u = R.indef_blocks()
    n, m, k = R.INDEF_CASE
    a = R.operator(n)
    pu, pbu = dev.panel(u), dev.panel(np.asfortranarray(b @ u))
    assert dev.lib.dla_b_ortho(dev.h, n, k, pu.ptr, pbu.ptr) == capi.ERR_LAPACK
    assert dev.lib.dla_last_error(dev.h).decode() == MSG
    good = R.case(*R.expand_width_case(17))
    rows = []
    for mode in (2, 0):
        for ahead in (1, 0):
            dev.spmm_setup(a)
            dev.spmm_setup_metric(b)
            r = _expand(dev, mode, a, x, bx, u, ahead)
            assert (r["st"], r["msg"]) == (capi.ERR_LAPACK, MSG), (mode, ahead, r["st"], r["msg"])
            assert np.array_equal(r["basis"][:, :m], x) and np.array_equal(r["bbasis"][:, :m], bx)
            ag = R.operator(good.n)
            dev.spmm_setup(ag)
            dev.spmm_setup_metric(good.b)
            rg = _expand(dev, mode, ag, good.x, good.bx, good.u, ahead)
            what = f"{good.name} mode={mode} ahead={ahead} after the error return"
            rows.append(("device expand " + what, _check_expand(good, mode, ag, rg, what)))
            assert rg["tails"] == ahead
    R.record(RECORD, rows)
