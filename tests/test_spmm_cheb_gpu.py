"""GPU: the Chebyshev polynomial preconditioner on the stored sparse operator (include/diaglib_amd.h, dla_spmm_precnd_cheb).

The steps are held element by element to twice the running bound of tests/cheb_ref.py around its long-double reference; the
Gershgorin bound, the guard, the formats' agreement, determinism, the launch count and every refusal to the sentences of the
contract; and whole solves on the 32 x 32 Laplacian to the oracle's iteration counts.  The step tests run on a context of their own
(the configuration is not an option tests/conftest.py could reset); the solves need the drivers' context and put it back by hand."""
import ctypes as C

import numpy as np
import pytest

import cheb_ref
import spmm_cases
import spmm_slots
from diaglib_amd import capi
from test_operators_gpu import SENT, Guarded

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAME = "dla_spmm_precnd_cheb"
N = 777
F = 0.02


@pytest.fixture(scope="module")
def own():
    with spmm_slots.fresh_context() as c:
        yield c


def apply(ctx, x, fac, status=False):
    """one call on x between sentinel columns: px (x must come back unchanged), or (status, message, px) of a call that may be refused"""
    n, m = x.shape
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    st = ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(NAME), n, m, float(fac), gx.ptr, gy.ptr)
    ctx.sync()
    got = gy.body().copy()
    gx.assert_unchanged()
    gx.free(); gy.free()
    if status:
        return st, spmm_slots.last_error(ctx), got
    assert st == 0, spmm_slots.last_error(ctx)
    return got


def panel(n, m, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, m)))


def assert_within_bound(ctx, csr, x, fac, d):
    """px of a d-step call against the reference on the bound the library itself reports"""
    ctx.spmm_cheb_config(d, F)
    g = ctx.spmm_cheb_info()["upper"]
    got = apply(ctx, x, fac)
    z, e = cheb_ref.reference(*csr, x, g, fac, d, F)
    teeth = cheb_ref.assert_bound_has_teeth(z, e)
    share = float((np.abs(got.astype(LD) - z) / (2 * e)).max())
    print("d = %d, m = %d, fac = %+.2f: %.3f of the tolerance (2 E_d / |z_d| = %.1e)" % (d, x.shape[1], fac, share, teeth))
    assert np.all(np.abs(got.astype(LD) - z) <= 2 * e), share
    return got


# ------------------------------------------------------------------------------------------------------------------ the steps
# half-bands 1, 3, 6, 12, 17: widths 3, 7, 13, 25, 35, one per rung of the ladder 4 / 8 / 16 / 32 / generic; every width with d = 8,
# every d with m = 13, every m and fac more than once.  n = 777 is four blocks of 256 rows, the last one partial.
ELL_CASES = [(1, 1, 8, 0.0), (3, 3, 8, -1.25), (6, 8, 8, 0.5), (12, 13, 8, 0.0), (17, 3, 8, -1.25), (17, 13, 1, 0.5), (3, 13, 2, 0.0),
             (6, 13, 3, -1.25), (1, 8, 2, 0.5), (12, 1, 3, 0.5), (17, 8, 1, 0.0), (6, 1, 2, -1.25)]


@pytest.mark.parametrize("half_band,m,d,fac", ELL_CASES)
def test_ellpack_steps_stay_inside_the_running_bound(own, half_band, m, d, fac):
    a = cheb_ref.banded(N, half_band)
    own.spmm_setup(a, "ell")
    assert own.spmm_info()["stored"] == (2 * half_band + 1) * N
    assert_within_bound(own, cheb_ref.raw(a), panel(N, m), fac, d)


def _sliced_matrix(which):
    if which == "ragged":
        return cheb_ref.raw(cheb_ref.banded(N, 6, ragged=True))
    n = {"skewed777": N, "skewed5000": 5000}[which]
    indptr, indices, data = spmm_cases.skewed_csr(np.random.default_rng(7), n)
    return n, indptr, indices, data


# m = 1, 5, 9: one past the column chunks 4 and 8 of the tail kernel and the slice kernel
@pytest.mark.parametrize("which,long_rows,multi", [("ragged", False, False), ("skewed777", True, False), ("skewed5000", True, True)])
@pytest.mark.parametrize("m,d,fac", [(1, 3, 0.0), (5, 8, 0.5), (9, 8, 0.0), (9, 3, 0.5)])
def test_sliced_steps_stay_inside_the_running_bound(own, which, long_rows, multi, m, d, fac):
    csr = _sliced_matrix(which)
    spmm_slots.setup(own, "A", *csr, "sell")
    info = own.spmm_info()
    assert info["format"] == "sell" and (info["long_rows"] > 0) == long_rows and (info["multi_segments"] > 0) == multi, info
    if which == "skewed5000":
        assert info["multi_segments"] >= 2 and info["long_segment_entries"] == 4096, info       # (the dense row: two segments)
    assert_within_bound(own, csr, panel(csr[0], m), fac, d)


def test_formats_agree_bit_for_bit(own):
    a = cheb_ref.banded(N, 6, ragged=True)
    x = panel(N, 9)
    own.spmm_cheb_config(8, F)
    got = {}
    for fmt in ("ell", "sell"):
        own.spmm_setup(a, fmt)
        assert own.spmm_info()["format"] == fmt
        got[fmt] = (own.spmm_cheb_info()["upper"], apply(own, x, 0.5))
    assert got["ell"][0] == got["sell"][0]
    assert spmm_slots.same_bits(got["ell"][1], got["sell"][1])


def test_host_and_device_set_ups_agree_bit_for_bit(own):
    n, indptr, indices, data = _sliced_matrix("skewed777")
    x = panel(n, 9)
    own.spmm_cheb_config(8, F)
    got = {}
    for where in ("host", "device"):
        spmm_slots.setup(own, "A", n, indptr, indices, data, "sell", where)
        got[where] = (own.spmm_cheb_info()["upper"], apply(own, x, 0.0))
    assert np.float64(got["host"][0]).view(np.uint64) == np.float64(got["device"][0]).view(np.uint64)
    short = np.diff(indptr) <= spmm_cases.LONG_ROW
    assert 0 < short.sum() < n
    assert spmm_slots.same_bits(got["host"][1][short], got["device"][1][short])
    assert spmm_slots.same_bits(got["host"][1], got["device"][1])        # (and the tail rows: one fixed order there as well)


# ------------------------------------------------------------------------------------------------------------------ the bound g
def _assert_upper(ctx, csr):
    g, slack = cheb_ref.gershgorin(*csr)
    got = ctx.spmm_cheb_info()["upper"]
    assert abs(LD(got) - g) <= slack, (got, float(g), float(slack))
    return got


@pytest.mark.parametrize("which,fmt", [("banded", "ell"), ("banded", "sell"), ("ragged", "sell"), ("skewed777", "sell"), ("skewed5000", "sell"),
                                       ("skewed777", "ell")])
def test_gershgorin_bound(own, which, fmt):
    csr = cheb_ref.raw(cheb_ref.banded(N, 3)) if which == "banded" else _sliced_matrix(which)
    own.spmm_cheb_config(3, F)
    got = {}
    for where in ("host", "device"):
        spmm_slots.setup(own, "A", *csr, fmt, where)
        got[where] = _assert_upper(own, csr)
    assert np.float64(got["host"]).view(np.uint64) == np.float64(got["device"]).view(np.uint64)
    if which == "banded":
        assert got["host"] >= np.linalg.eigvalsh(cheb_ref.banded(N, 3).toarray())[-1]


def test_gershgorin_bound_follows_the_stored_matrix(own):
    n, indptr, indices, data = _sliced_matrix("skewed777")
    own.spmm_cheb_config(3, F)
    spmm_slots.setup(own, "A", n, indptr, indices, data, "sell")
    first = _assert_upper(own, (n, indptr, indices, data))
    spmm_slots.refresh(own, "A", n, indptr, indices, 3.0 * data)
    tripled = _assert_upper(own, (n, indptr, indices, 3.0 * data))
    assert tripled > 2.9 * first
    other = cheb_ref.raw(cheb_ref.banded(N, 3))
    spmm_slots.setup(own, "A", *other, "ell")
    assert _assert_upper(own, other) < 0.5 * first
    # the configuration is the context's: it has survived the refresh and both set-ups
    assert own.spmm_cheb_info()["steps"] == 3 and own.spmm_cheb_info()["lo_fraction"] == F


# ------------------------------------------------------------------------------------------------------------------ guard, determinism, booking
def test_guard_returns_x_bit_for_bit(own):
    a = cheb_ref.banded(N, 3)
    own.spmm_setup(a, "ell")
    own.spmm_cheb_config(8, F)
    x = panel(N, 5)
    upper = own.spmm_cheb_info()["upper"]
    assert spmm_slots.same_bits(apply(own, x, -(upper + 1.0)), x)
    assert spmm_slots.same_bits(apply(own, x, -upper), x)                # hi = 0: still the guard


@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_repeated_calls_are_bit_identical_and_booked_per_step(own, fmt, d):
    if fmt == "ell":
        own.spmm_setup(cheb_ref.banded(N, 6), "ell")
    else:
        spmm_slots.setup(own, "A", *_sliced_matrix("skewed5000"), "sell")
    n = own.spmm_info()["n"]
    own.spmm_cheb_config(d, F)
    own.spmm_cheb_info()
    x = panel(n, 5)
    own.reset_stats()
    first = apply(own, x, 0.5)
    launches = own.stats()["precnd"]["launches"]
    assert spmm_slots.same_bits(apply(own, x, 0.5), first)
    assert own.stats()["precnd"]["launches"] == 2 * launches
    if fmt == "ell":
        assert launches == max(1, d - 1)
        ks = own.kernel_stats()
        if d > 1:
            w = own.spmm_info()["stored"] // n
            assert ks["ell_cheb_step_kernel"]["launches"] == 2 * (d - 1)
            assert ks["ell_cheb_step_kernel"]["alg_bytes"] == 2 * (d - 1) * (12.0 * w * n + 32.0 * n * 5)
            assert ks["ell_cheb_step_kernel"]["flops"] == 2 * (d - 1) * (2.0 * w * n * 5 + 7.0 * n * 5)
        assert own.stats()["matvec"]["launches"] == 0


def test_the_unfused_path_gives_the_fused_bits(own):
    """knob 7 = 30 (Knobs::cheb_unfused, the A/B comparand): the product kernel plus one combining sweep"""
    x = panel(5000, 9)
    own.spmm_cheb_config(8, F)
    for fmt, csr in (("ell", cheb_ref.raw(cheb_ref.banded(5000, 6))), ("sell", _sliced_matrix("skewed5000"))):
        spmm_slots.setup(own, "A", *csr, fmt)
        fused = apply(own, x, 0.5)
        own.set_option(107, 30)
        try:
            unfused = apply(own, x, 0.5)
        finally:
            own.set_option(107, 0)
        assert spmm_slots.same_bits(fused, unfused), fmt


# ------------------------------------------------------------------------------------------------------------------ refusals
def _assert_refused(ctx, n, cause):
    st, msg, px = apply(ctx, panel(n, 3), 0.0, status=True)
    assert st == capi.ERR_ARG, (st, msg)
    assert NAME in msg and cause in msg, msg
    assert np.all(px == SENT), "a refused call wrote to px"


def test_refusals():
    a = cheb_ref.banded(N, 3)
    with spmm_slots.fresh_context() as c:
        # (a refused set-up of A still makes c the context this thread's callbacks act on)
        assert spmm_slots.setup_status(c, "A", 0, *cheb_ref.raw(a)[1:], "ell") == capi.ERR_ARG
        info = capi.SpmmChebInfo()
        assert c.lib.dla_spmm_cheb_info(c.h, C.byref(info)) == capi.ERR_ARG
        c.spmm_cheb_config(8, F)
        _assert_refused(c, N, "no operator")
        assert c.lib.dla_spmm_cheb_info(c.h, C.byref(info)) == capi.ERR_ARG
        c.spmm_cheb_config(0, F)
        c.spmm_setup(a, "ell")
        _assert_refused(c, N, "nothing is configured")
        assert c.lib.dla_spmm_cheb_info(c.h, C.byref(info)) == capi.ERR_ARG
        c.spmm_cheb_config(8, F)
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        _assert_refused(c, N - 1, "n = 776 differs")
        c.spmm_cheb_config(0, F)
        _assert_refused(c, N, "nothing is configured")
        c.spmm_cheb_config(8, F)
        c.spmm_setup_sharded(a, 0, N)
        _assert_refused(c, N, "row-sharded")
        assert c.lib.dla_spmm_cheb_info(c.h, C.byref(info)) == capi.ERR_ARG
        c.spmm_setup(a, "ell")                          # (A is whole again)
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)


def test_config_refuses_bad_values_and_keeps_the_earlier_configuration(own):
    own.spmm_setup(cheb_ref.banded(N, 3), "ell")
    own.spmm_cheb_config(3, 0.125)
    before = apply(own, panel(N, 3), 0.0)
    for steps, f in ((-1, 0.02), (8, 0.0), (8, 1.0), (8, -0.1), (8, float("nan"))):
        assert own.lib.dla_spmm_cheb_config(own.h, steps, f) == capi.ERR_ARG, (steps, f)
        assert "spmm_cheb_config" in spmm_slots.last_error(own)
        info = own.spmm_cheb_info()
        assert info["steps"] == 3 and info["lo_fraction"] == 0.125, info
    assert spmm_slots.same_bits(apply(own, panel(N, 3), 0.0), before)


# ------------------------------------------------------------------------------------------------------------------ whole solves
@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("driver", ["davidson", "lobpcg"])
def test_solves_follow_the_oracle(ctx, oracle, driver, fmt):
    """the drivers run on the thread's default context, so this test configures that one and switches the preconditioner off again"""
    s = cheb_ref.SOLVE
    a = cheb_ref.laplacian()
    n, t, n_max = a.shape[0], s["n_targ"], s["n_max"]
    want = np.linalg.eigvalsh(a.toarray())[:t]
    ok_o, iters_o, _ = cheb_ref.oracle_counts(oracle, "cheb")[driver]
    assert ok_o
    ctx.spmm_setup(a, fmt)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.spmm_cheb_config(s["steps"], s["lo_fraction"])
    try:
        mv = capi.fn_address("dla_spmm_matvec")
        res = {}
        for pc in (NAME, "dla_spmm_precnd"):
            ev = ctx.panel(cheb_ref.guess(n, n_max))
            if driver == "davidson":
                eig, _, ok, info = ctx.davidson_driver(n, t, n_max, s["max_iter"], s["tol"], s["max_dav"], 0.0, mv, capi.fn_address(pc), ev)
            else:
                eig, _, ok, info = ctx.lobpcg_driver(n, t, n_max, s["max_iter"], s["tol"], 0.0, mv, capi.fn_address(pc), ev)
            res[pc] = (ok, info["iters"], eig[:t].copy())
            ev.free()
    finally:
        ctx.spmm_cheb_config(0, 0.0)
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ok, iters, eig = res[NAME]
    print("%s, %s: %d iterations, the oracle %d; diagonal: ok = %s after %d" % (driver, fmt, iters, iters_o, res["dla_spmm_precnd"][0], res["dla_spmm_precnd"][1]))
    assert ok, res
    assert np.abs(eig - want).max() <= 1e-9, (eig, want)
    assert abs(iters - iters_o) <= max(1, iters_o // 5), (iters, iters_o)
    assert not res["dla_spmm_precnd"][0], res
