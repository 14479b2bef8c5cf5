"""GPU: the diagonally scaled Chebyshev preconditioner on the stored sparse operator (include/diaglib_amd.h,
dla_spmm_precnd_cheb_jacobi).

The steps are held element by element to twice the running bound of tests/cheb_jacobi_ref.py around its long-double reference, on
the hi the library itself reports; hi, the guard, the formats' and the set-ups' agreement, determinism, the booking and every refusal
to the sentences of the contract; and whole solves on diffusion(32, 1e3) to the oracle's iteration counts.  As in
tests/test_spmm_cheb_gpu.py the step tests run on a context of their own and the solves on the drivers' context."""
import ctypes as C

import numpy as np
import pytest

import cheb_jacobi_ref as ref
import cheb_ref
import spmm_cases
import spmm_slots
from diaglib_amd import capi
from test_operators_gpu import SENT, Guarded

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAME = "dla_spmm_precnd_cheb_jacobi"
PLAIN = "dla_spmm_precnd_cheb"
N = 777
F = 0.02
GUARD_FAC = -(2.0 + 7 / 50.0)          # row 7 of banded(): diag[7] + fac = 0 exactly


@pytest.fixture(scope="module")
def own():
    with spmm_slots.fresh_context() as c:
        yield c


def apply(ctx, x, fac, status=False, name=NAME):
    """one call on x between sentinel columns: px (x must come back unchanged), or (status, message, px) of a call that may be refused"""
    n, m = x.shape
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    st = ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, float(fac), gx.ptr, gy.ptr)
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


def bits(v):
    return np.float64(v).view(np.uint64)


def assert_within_bound(ctx, csr, x, fac, d):
    """px of a d-step call against the reference on the hi the library itself reports"""
    ctx.spmm_cheb_config(d, F)
    hi = ctx.spmm_cheb_jacobi_upper(fac)
    got = apply(ctx, x, fac)
    z, e = ref.reference(*csr, x, hi, fac, d, F)
    teeth = cheb_ref.assert_bound_has_teeth(z, e)
    share = float((np.abs(got.astype(LD) - z) / (2 * e)).max())
    print("d = %d, m = %d, fac = %+.2f: %.3f of the tolerance (2 E_d / |z_d| = %.1e)" % (d, x.shape[1], fac, share, teeth))
    assert np.all(np.abs(got.astype(LD) - z) <= 2 * e), share
    return got


# ------------------------------------------------------------------------------------------------------------------ the steps
# half-bands 1, 3, 6, 12, 17: one per rung of the ladder 4 / 8 / 16 / 32 / generic, each with d = 8 (fac 0 or 0.5 only) and with a
# short d; m = 1, 3, 8, 13; d = 1, 2, 3 also with fac = -1.25; the row that hits the guard exactly; rows with a_ii + fac < 0.
ELL_CASES = [(1, 1, 8, 0.0), (3, 3, 8, 0.5), (6, 8, 8, 0.5), (12, 13, 8, 0.0), (17, 3, 8, 0.5), (17, 13, 1, 0.5), (3, 13, 2, 0.0),
             (6, 13, 3, -1.25), (1, 8, 2, -1.25), (12, 1, 3, 0.5), (17, 8, 1, -1.25), (6, 1, 2, 0.5), (12, 8, 3, -1.25),
             (6, 5, 3, GUARD_FAC), (3, 8, 3, -3.0), (17, 13, 2, -3.0), (1, 3, 1, -3.0)]


@pytest.mark.parametrize("half_band,m,d,fac", ELL_CASES)
def test_ellpack_steps_stay_inside_the_running_bound(own, half_band, m, d, fac):
    a = cheb_ref.banded(N, half_band)
    own.spmm_setup(a, "ell")
    assert own.spmm_info()["stored"] == (2 * half_band + 1) * N
    if fac == GUARD_FAC:
        assert a.diagonal()[7] + fac == 0.0
    if fac == -3.0:
        assert 0 < (a.diagonal() + fac < 0).sum() < N
    assert_within_bound(own, cheb_ref.raw(a), panel(N, m), fac, d)


def _sliced_matrix(which):
    if which == "ragged":
        return cheb_ref.raw(cheb_ref.banded(N, 6, ragged=True))
    if which == "diffusion":
        return cheb_ref.raw(ref.diffusion(ref.ORDER, ref.CONTRAST))
    n = {"skewed777": N, "skewed5000": 5000}[which]
    indptr, indices, data = spmm_cases.skewed_csr(np.random.default_rng(7), n)
    return n, indptr, indices, data


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


def test_sliced_steps_on_the_diffusion_matrix(own):
    csr = _sliced_matrix("diffusion")
    spmm_slots.setup(own, "A", *csr, "sell")
    assert own.spmm_info()["format"] == "sell"
    assert_within_bound(own, csr, panel(csr[0], 5), -0.3, 8)


# ------------------------------------------------------------------------------------------------------------------ hi
def _assert_upper(ctx, csr, fac):
    hi, slack = ref.upper(*csr, fac)
    got = ctx.spmm_cheb_jacobi_upper(fac)
    assert abs(LD(got) - hi) <= slack, (got, float(hi), float(slack))
    return got


@pytest.mark.parametrize("which,fmt", [("banded", "ell"), ("banded", "sell"), ("ragged", "sell"), ("skewed777", "sell"), ("skewed5000", "sell"),
                                       ("skewed777", "ell"), ("diffusion", "ell")])
def test_upper_against_the_long_double_reference(own, which, fmt):
    csr = cheb_ref.raw(cheb_ref.banded(N, 3)) if which == "banded" else _sliced_matrix(which)
    own.spmm_cheb_config(3, F)
    for fac in (0.0, 0.5, -1.25):
        got = {}
        for where in ("host", "device"):
            spmm_slots.setup(own, "A", *csr, fmt, where)
            got[where] = _assert_upper(own, csr, fac)
        assert bits(got["host"]) == bits(got["device"])
        if which == "banded":
            m = cheb_ref.banded(N, 3).toarray() + fac * np.eye(N)
            den = ref.scaling(np.diag(m).copy(), 0.0)[1]
            assert got["host"] >= np.abs(np.linalg.eigvals(m / den[:, None])).max()


def test_upper_follows_the_stored_matrix(own):
    n, indptr, indices, data = _sliced_matrix("skewed777")
    own.spmm_cheb_config(3, F)
    spmm_slots.setup(own, "A", n, indptr, indices, data, "sell")
    first = _assert_upper(own, (n, indptr, indices, data), 0.5)
    g = own.spmm_cheb_info()["upper"]
    spmm_slots.refresh(own, "A", n, indptr, indices, 3.0 * data)
    assert _assert_upper(own, (n, indptr, indices, 3.0 * data), 1.5) == pytest.approx(first, rel=1e-13)
    moved = _assert_upper(own, (n, indptr, indices, 3.0 * data), 0.5)
    assert moved != first
    assert own.spmm_cheb_info()["upper"] > 2.9 * g
    other = cheb_ref.raw(cheb_ref.banded(N, 3))
    spmm_slots.setup(own, "A", *other, "ell")
    assert _assert_upper(own, other, 0.5) != moved
    spmm_slots.setup(own, "A", n, indptr, indices, data, "sell")
    assert bits(_assert_upper(own, (n, indptr, indices, data), 0.5)) == bits(first)


# ------------------------------------------------------------------------------------------------------------------ bits
def test_formats_agree_bit_for_bit(own):
    a = cheb_ref.banded(N, 6, ragged=True)
    x = panel(N, 9)
    own.spmm_cheb_config(8, F)
    got = {}
    for fmt in ("ell", "sell"):
        own.spmm_setup(a, fmt)
        assert own.spmm_info()["format"] == fmt
        got[fmt] = (own.spmm_cheb_jacobi_upper(0.5), apply(own, x, 0.5))
    assert bits(got["ell"][0]) == bits(got["sell"][0])
    assert spmm_slots.same_bits(got["ell"][1], got["sell"][1])


def test_host_and_device_set_ups_agree_bit_for_bit(own):
    n, indptr, indices, data = _sliced_matrix("skewed777")
    x = panel(n, 9)
    own.spmm_cheb_config(8, F)
    got = {}
    for where in ("host", "device"):
        spmm_slots.setup(own, "A", n, indptr, indices, data, "sell", where)
        got[where] = (own.spmm_cheb_jacobi_upper(0.0), apply(own, x, 0.0))
    assert own.spmm_info()["long_rows"] > 0
    assert bits(got["host"][0]) == bits(got["device"][0])
    assert spmm_slots.same_bits(got["host"][1], got["device"][1])        # (the tail rows included: one fixed order there as well)


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


def test_guard_returns_x_bit_for_bit(own):
    """A = 3 I with fac = -3: every s_i = 0, so every den_i = 1 and hi = 0"""
    import scipy.sparse as sp
    own.spmm_setup((3.0 * sp.identity(N)).tocsr(), "ell")
    own.spmm_cheb_config(8, F)
    x = panel(N, 5)
    assert own.spmm_cheb_jacobi_upper(-3.0) == 0.0
    assert spmm_slots.same_bits(apply(own, x, -3.0), x)
    assert own.spmm_cheb_jacobi_upper(0.0) == 1.0


def test_one_step_is_the_diagonal_preconditioner(own):
    a = cheb_ref.banded(N, 6)
    own.spmm_setup(a, "ell")
    own.spmm_cheb_config(1, F)
    x = panel(N, 5)
    fac = 0.5
    hi = own.spmm_cheb_jacobi_upper(fac)
    theta = float(cheb_ref.scalars(hi, F * hi, 1)[0])        # (lo = f hi is a double product, theta is rounded once)
    r = 1.0 / ref.scaling(a.diagonal(), fac)[1]
    assert spmm_slots.same_bits(apply(own, x, fac), (x * r[:, None]) / theta)


@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_repeated_calls_are_bit_identical_and_booked_per_step(own, fmt, d):
    m = 5
    if fmt == "ell":
        own.spmm_setup(cheb_ref.banded(N, 6), "ell")
    else:
        spmm_slots.setup(own, "A", *_sliced_matrix("skewed5000"), "sell")
    n = own.spmm_info()["n"]
    own.spmm_cheb_config(d, F)
    own.spmm_cheb_jacobi_upper(0.5)
    x = panel(n, m)
    own.reset_stats()
    first = apply(own, x, 0.5)
    launches, syncs = own.stats()["precnd"]["launches"], own.stats()["host_syncs"]
    assert spmm_slots.same_bits(apply(own, x, 0.5), first)
    assert own.stats()["precnd"]["launches"] == 2 * launches
    ks = own.kernel_stats()
    assert ks["cheb_jacobi_bound_kernel"]["launches"] == 2 and ks["cheb_jacobi_bound_kernel"]["alg_bytes"] == 2 * 24.0 * n
    assert ks["cheb_jacobi_scale_kernel"]["launches"] == 2 and ks["cheb_jacobi_scale_kernel"]["alg_bytes"] == 2 * (16.0 * n * m + 8.0 * n)
    for plain in ("ell_cheb_step_kernel", "sell_cheb_step_kernel", "cheb_scale_kernel", "cheb_combine_kernel"):
        assert ks.get(plain, {"launches": 0})["launches"] == 0, plain
    assert own.stats()["matvec"]["launches"] == 0
    if fmt == "ell":
        assert launches == 2 + max(0, d - 1)
        if d > 1:
            w = own.spmm_info()["stored"] // n
            assert ks["ell_cheb_jacobi_step_kernel"]["launches"] == 2 * (d - 1)
            assert ks["ell_cheb_jacobi_step_kernel"]["alg_bytes"] == 2 * (d - 1) * (12.0 * w * n + 32.0 * n * m + 8.0 * n)
            assert ks["ell_cheb_jacobi_step_kernel"]["flops"] == 2 * (d - 1) * (2.0 * w * n * m + 10.0 * n * m)
    elif d > 1:
        assert ks["sell_cheb_jacobi_step_kernel"]["launches"] == 2 * (d - 1)
    # one host wait per call, on top of what apply() itself costs around a call of the plain callback (which has none)
    per_call = own.stats()["host_syncs"] - syncs
    own.spmm_cheb_info()
    before = own.stats()["host_syncs"]
    apply(own, x, 0.5, name=PLAIN)
    assert per_call == own.stats()["host_syncs"] - before + 1, (per_call, before)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _assert_refused(ctx, n, cause):
    st, msg, px = apply(ctx, panel(n, 3), 0.0, status=True)
    assert st == capi.ERR_ARG, (st, msg)
    assert NAME in msg and cause in msg, msg
    assert np.all(px == SENT), "a refused call wrote to px"
    hi = C.c_double(-1.0)
    if "differs" not in cause:
        assert ctx.lib.dla_spmm_cheb_jacobi_upper(ctx.h, 0.0, C.byref(hi)) == capi.ERR_ARG and hi.value == -1.0


def test_refusals():
    a = cheb_ref.banded(N, 3)
    with spmm_slots.fresh_context() as c:
        # (a refused set-up of A still makes c the context this thread's callbacks act on)
        assert spmm_slots.setup_status(c, "A", 0, *cheb_ref.raw(a)[1:], "ell") == capi.ERR_ARG
        c.spmm_cheb_config(8, F)
        _assert_refused(c, N, "no operator")
        c.spmm_cheb_config(0, F)
        c.spmm_setup(a, "ell")
        _assert_refused(c, N, "nothing is configured")
        c.spmm_cheb_config(8, F)
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        _assert_refused(c, N - 1, "n = 776 differs")
        c.spmm_cheb_config(0, F)
        _assert_refused(c, N, "nothing is configured")
        c.spmm_cheb_config(8, F)
        c.spmm_setup_sharded(a, 0, N)
        _assert_refused(c, N, "row-sharded")
        c.spmm_setup(a, "ell")                          # (A is whole again)
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        assert c.lib.dla_spmm_cheb_jacobi_upper(c.h, 0.0, None) == capi.ERR_ARG


def test_a_bad_configuration_keeps_the_earlier_one(own):
    own.spmm_setup(cheb_ref.banded(N, 3), "ell")
    own.spmm_cheb_config(3, 0.125)
    before = apply(own, panel(N, 3), 0.0)
    for steps, f in ((-1, 0.02), (8, 0.0), (8, 1.0), (8, -0.1), (8, float("nan"))):
        assert own.lib.dla_spmm_cheb_config(own.h, steps, f) == capi.ERR_ARG, (steps, f)
    assert spmm_slots.same_bits(apply(own, panel(N, 3), 0.0), before)


def test_the_plain_callback_is_untouched(own):
    """plain, scaled, plain on one context: the two share the configuration and the work panels, and nothing else"""
    x = panel(5000, 9)
    own.spmm_cheb_config(8, F)
    for fmt, csr in (("ell", cheb_ref.raw(cheb_ref.banded(5000, 6))), ("sell", _sliced_matrix("skewed5000"))):
        spmm_slots.setup(own, "A", *csr, fmt)
        g = own.spmm_cheb_info()["upper"]
        first = apply(own, x, 0.5, name=PLAIN)
        scaled = apply(own, x, 0.5)
        assert not spmm_slots.same_bits(scaled, first)
        assert spmm_slots.same_bits(apply(own, x, 0.5, name=PLAIN), first), fmt
        assert bits(own.spmm_cheb_info()["upper"]) == bits(g)


# ------------------------------------------------------------------------------------------------------------------ whole solves
@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("driver", ["davidson", "lobpcg"])
def test_solves_follow_the_oracle(ctx, oracle, driver, fmt):
    """the drivers run on the thread's default context, so this test configures that one and switches the preconditioner off again"""
    s = ref.SOLVE
    a = ref.diffusion(ref.ORDER, ref.CONTRAST)
    n, t, n_max = a.shape[0], s["n_targ"], s["n_max"]
    want = np.linalg.eigvalsh(a.toarray())[:t]
    ok_o, iters_o, _ = ref.oracle_counts(oracle, "scaled")[driver]
    assert ok_o
    ctx.spmm_setup(a, fmt)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.spmm_cheb_config(s["steps"], s["lo_fraction"])
    try:
        mv = capi.fn_address("dla_spmm_matvec")
        res = {}
        for pc in (NAME, PLAIN, "dla_spmm_precnd"):
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
    print("%s, %s: %d iterations, the oracle %d; plain: ok = %s after %d; diagonal: ok = %s after %d"
          % (driver, fmt, iters, iters_o, res[PLAIN][0], res[PLAIN][1], res["dla_spmm_precnd"][0], res["dla_spmm_precnd"][1]))
    assert ok, res
    assert np.abs(eig - want).max() <= 1e-9, (eig, want)
    assert abs(iters - iters_o) <= max(1, iters_o // 5), (iters, iters_o)
    assert iters < res[PLAIN][1], res
    assert not res["dla_spmm_precnd"][0], res
