"""GPU: the Chebyshev preconditioner on the scaled pencil A + fac B of the stored operator and the stored metric
(include/diaglib_amd.h, dla_spmm_precnd_cheb_pencil).

The steps are held element by element to twice the running bound of tests/cheb_pencil_ref.py around its long-double reference, on
the hi the library itself reports; hi, the guard, the agreement of the three ways to run a step, of the formats and of the set-ups,
the reduction to the scaled form for B = I, determinism, the booking and every refusal to the sentences of the contract; and whole
solves on (diffusion(32, 1e3), mass(32)) to the oracle's iteration counts.  As in tests/test_spmm_cheb_jacobi_gpu.py the step tests
run on a context of their own and the solves on the drivers' context."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cheb_pencil_ref as ref
import cheb_ref
import spmm_cases
import spmm_slots
from diaglib_amd import capi
from test_operators_gpu import SENT, Guarded

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAME = "dla_spmm_precnd_cheb_pencil"
SCALED = "dla_spmm_precnd_cheb_jacobi"
PLAIN = "dla_spmm_precnd_cheb"
DIAG = "dla_spmm_precnd_pencil"
N, F = ref.N, ref.F
FUSED = "ell_cheb_pencil_step_kernel"
PANEL = {"ell": "ell_cheb_pencil_panel_step_kernel", "sell": "sell_cheb_pencil_panel_step_kernel"}
COMBINE = "cheb_pencil_combine_kernel"
panel = ref.panel


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


def bits(v):
    return np.float64(v).view(np.uint64)


def launches(ctx, kernel):
    return ctx.kernel_stats().get(kernel, {"launches": 0})["launches"]


def store(ctx, csr_a, fmt_a, csr_b, fmt_b, where="host"):
    spmm_slots.setup(ctx, "A", *csr_a, fmt_a, where)
    spmm_slots.setup(ctx, "B", *csr_b, fmt_b, where)
    ia, ib = ctx.spmm_info(), ctx.spmm_metric_info()
    assert ia["format"] == fmt_a and ib["format"] == fmt_b, (ia, ib)
    return ia, ib


def assert_within_bound(ctx, csr_a, csr_b, x, fac, d):
    """px of a d-step call against the reference on the hi the library itself reports"""
    ctx.spmm_cheb_config(d, F)
    hi = ctx.spmm_cheb_pencil_upper(fac)
    got = apply(ctx, x, fac)
    z, e = ref.reference(csr_a, csr_b, x, hi, fac, d, F)
    teeth = cheb_ref.assert_bound_has_teeth(z, e)
    share = float((np.abs(got.astype(LD) - z) / (2 * e)).max())
    print("d = %d, m = %d, fac = %+.3f: %.3f of the tolerance (2 E_d / |z_d| = %.1e)" % (d, x.shape[1], fac, share, teeth))
    assert np.all(np.abs(got.astype(LD) - z) <= 2 * e), share
    return got


_BIG = {}


def big(name):
    if name not in _BIG:
        _BIG[name] = ref.big_matrix(name)
    return _BIG[name]


def big_fmt(name):
    """the skewed matrix has a dense row: sliced only"""
    return "sell" if name == "skewed" else "ell"


# ------------------------------------------------------------------------------------------------------------------ the steps
@pytest.mark.parametrize("hba,hbb,m,d,fac", ref.BAND_CASES)
def test_ellpack_pairs_stay_inside_the_running_bound(own, hba, hbb, m, d, fac):
    a, b = ref.band_pair(hba, hbb)
    ia, ib = store(own, cheb_ref.raw(a), "ell", cheb_ref.raw(b), "ell")
    assert ia["stored"] == (2 * hba + 1) * N and ib["stored"] == (2 * hbb + 1) * N
    den0 = ref.scaling(a.diagonal(), b.diagonal(), fac)[0]
    if fac == ref.GUARD_FAC:
        assert den0[77] == 0.0
    if fac == -3.0:
        assert (den0 < 0).sum() == 51
    own.reset_stats()
    assert_within_bound(own, cheb_ref.raw(a), cheb_ref.raw(b), panel(N, m), fac, d)
    assert launches(own, FUSED) == d - 1 and own.stats()["matvec"]["launches"] == 0


@pytest.mark.parametrize("m,d,fac", ref.BIG_RUNS)
@pytest.mark.parametrize("pair", ref.BIG_PAIRS)
def test_mixed_and_sliced_pairs_stay_inside_the_running_bound(own, pair, m, d, fac):
    csr_a, csr_b = big(pair[0]), big(pair[1])
    infos = store(own, csr_a, big_fmt(pair[0]), csr_b, big_fmt(pair[1]))
    for name, info in zip(pair, infos):
        if name == "skewed":
            assert info["long_rows"] > 0 and info["multi_segments"] >= 2 and info["long_segment_entries"] == 4096, info   # (the dense row: two segments)
        else:
            assert info["format"] == "ell", info
    own.reset_stats()
    assert_within_bound(own, csr_a, csr_b, panel(5000, m), fac, d)
    assert launches(own, FUSED) == 0 and launches(own, PANEL[big_fmt(pair[0])]) == d - 1


def test_sliced_steps_on_diffusion_and_mass(own):
    csr_a, csr_b = cheb_ref.raw(ref.diffusion(ref.ORDER, ref.CONTRAST)), cheb_ref.raw(ref.mass(ref.ORDER))
    store(own, csr_a, "sell", csr_b, "ell")
    assert_within_bound(own, csr_a, csr_b, panel(csr_a[0], 5), -0.3, 8)


# ------------------------------------------------------------------------------------------------------------------ hi
def _assert_upper(ctx, csr_a, csr_b, fac):
    hi, slack = ref.upper(csr_a, csr_b, fac)
    got = ctx.spmm_cheb_pencil_upper(fac)
    assert abs(LD(got) - hi) <= slack, (got, float(hi), float(slack))
    return got


def _upper_case(which):
    if which == "banded":
        return cheb_ref.raw(cheb_ref.banded(N, 3)), cheb_ref.raw(ref.metric_band(N, 6))
    if which == "diffusion":
        return cheb_ref.raw(ref.diffusion(ref.ORDER, ref.CONTRAST)), cheb_ref.raw(ref.mass(ref.ORDER))
    return {"skewedA": (big("skewed"), big("metric3")), "skewedB": (big("banded6"), big("skewed"))}[which]


@pytest.mark.parametrize("which,fmt_a,fmt_b", [("banded", "ell", "ell"), ("banded", "sell", "sell"), ("banded", "ell", "sell"),
                                               ("skewedA", "sell", "ell"), ("skewedB", "ell", "sell"), ("diffusion", "ell", "ell")])
def test_upper_against_the_long_double_reference(own, which, fmt_a, fmt_b):
    csr_a, csr_b = _upper_case(which)
    own.spmm_cheb_config(3, F)
    for fac in (0.0, 0.5, -1.25):
        got = {}
        for where in ("host", "device"):
            store(own, csr_a, fmt_a, csr_b, fmt_b, where)
            got[where] = _assert_upper(own, csr_a, csr_b, fac)
        assert bits(got["host"]) == bits(got["device"])


def test_upper_follows_the_stored_matrices(own):
    csr_a, csr_b = cheb_ref.raw(cheb_ref.banded(N, 3)), cheb_ref.raw(ref.metric_band(N, 6))
    n, indptr, indices, data = csr_b
    own.spmm_cheb_config(3, F)
    store(own, csr_a, "ell", csr_b, "sell")
    first = _assert_upper(own, csr_a, csr_b, 0.5)
    g = own.spmm_cheb_info()["upper"]
    scaled = own.spmm_cheb_jacobi_upper(0.5)
    # new values for the metric: offB is the stored metric's
    spmm_slots.refresh(own, "B", n, indptr, indices, 3.0 * data)
    moved = _assert_upper(own, csr_a, (n, indptr, indices, 3.0 * data), 0.5)
    assert moved != first
    assert bits(own.spmm_cheb_info()["upper"]) == bits(g) and bits(own.spmm_cheb_jacobi_upper(0.5)) == bits(scaled)      # (slot A keeps its bits)
    spmm_slots.refresh(own, "B", n, indptr, indices, data)
    assert bits(_assert_upper(own, csr_a, csr_b, 0.5)) == bits(first)
    # a new A
    other = cheb_ref.raw(cheb_ref.banded(N, 6))
    spmm_slots.setup(own, "A", *other, "ell")
    assert _assert_upper(own, other, csr_b, 0.5) != first
    # a new B
    wide = cheb_ref.raw(ref.metric_band(N, 17))
    spmm_slots.setup(own, "B", *wide, "ell")
    assert _assert_upper(own, other, wide, 0.5) != first
    # the same arrays again
    store(own, csr_a, "ell", csr_b, "sell")
    assert bits(_assert_upper(own, csr_a, csr_b, 0.5)) == bits(first)
    # no metric: both entries refuse
    own.spmm_drop_metric()
    hi = C.c_double(-1.0)
    assert own.lib.dla_spmm_cheb_pencil_upper(own.h, 0.5, C.byref(hi)) == capi.ERR_ARG and hi.value == -1.0
    st, msg, px = apply(own, panel(N, 2), 0.5, status=True)
    assert st == capi.ERR_ARG and NAME in msg and "no metric" in msg and np.all(px == SENT), (st, msg)


# ------------------------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_identity_metric_gives_the_bits_of_the_scaled_form(own, fmt):
    csr_a = cheb_ref.raw(cheb_ref.banded(N, 6)) if fmt == "ell" else (N,) + tuple(spmm_cases.skewed_csr(np.random.default_rng(7), N))
    eye = cheb_ref.raw(sp.identity(N, format="csr"))
    x = panel(N, 9)
    for fmt_b in ("ell", "sell"):
        store(own, csr_a, fmt, eye, fmt_b)
        for d in (1, 3, 8):
            own.spmm_cheb_config(d, F)
            for fac in (0.5, -1.25):
                assert bits(own.spmm_cheb_pencil_upper(fac)) == bits(own.spmm_cheb_jacobi_upper(fac)), (d, fac)
                assert spmm_slots.same_bits(apply(own, x, fac), apply(own, x, fac, name=SCALED)), (fmt, fmt_b, d, fac)


def test_the_three_paths_agree_bit_for_bit(own):
    """one row loop for two ELLPACK matrices, B u through a panel for every other pair of formats, and knob 7 = 30 (Knobs::cheb_unfused):
    both products and one combining sweep"""
    d, m, fac = 8, 9, 0.5
    x = panel(5000, m)
    own.spmm_cheb_config(d, F)

    def run(unfused):
        own.set_option(107, 30 if unfused else 0)
        try:
            own.reset_stats()
            return apply(own, x, fac), own.stats()["matvec"]["launches"], {k: launches(own, k) for k in (FUSED, COMBINE, PANEL["ell"], PANEL["sell"])}
        finally:
            own.set_option(107, 0)

    # no tails: the same two matrices in all four pairs of formats
    csr_a, csr_b = big("banded6"), big("metric3")
    store(own, csr_a, "ell", csr_b, "ell")
    fused, mv, ks = run(False)
    assert mv == 0 and ks[FUSED] == d - 1 and ks[COMBINE] == 0 and ks[PANEL["ell"]] == 0, (mv, ks)
    unfused, mv, ks = run(True)
    assert mv == 2 * (d - 1) and ks[COMBINE] == d - 1 and ks[FUSED] == 0, (mv, ks)
    assert spmm_slots.same_bits(fused, unfused)
    for fmt_a, fmt_b in (("ell", "sell"), ("sell", "ell"), ("sell", "sell")):
        store(own, csr_a, fmt_a, csr_b, fmt_b)
        got, mv, ks = run(False)
        assert mv == d - 1 and ks[PANEL[fmt_a]] == d - 1 and ks[FUSED] == 0 and ks[COMBINE] == 0, (fmt_a, fmt_b, mv, ks)       # (B's product: d - 1)
        assert spmm_slots.same_bits(got, fused), (fmt_a, fmt_b)
        assert spmm_slots.same_bits(run(True)[0], fused), (fmt_a, fmt_b)
    # tails in either slot and in both
    for pair in ref.BIG_PAIRS:
        store(own, big(pair[0]), big_fmt(pair[0]), big(pair[1]), big_fmt(pair[1]))
        got, mv, ks = run(False)
        assert mv == d - 1 and ks[PANEL[big_fmt(pair[0])]] == d - 1 and ks[FUSED] == 0, (pair, mv, ks)
        other, mv, ks = run(True)
        assert mv == 2 * (d - 1) and ks[COMBINE] == d - 1, (pair, mv, ks)
        assert spmm_slots.same_bits(got, other), pair


def test_host_and_device_set_ups_agree_bit_for_bit(own):
    x = panel(5000, 9)
    own.spmm_cheb_config(8, F)
    for pair in (("skewed", "skewed"), ("banded6", "metric3")):
        got = {}
        for where in ("host", "device"):
            store(own, big(pair[0]), big_fmt(pair[0]), big(pair[1]), big_fmt(pair[1]), where)
            got[where] = (own.spmm_cheb_pencil_upper(0.5), apply(own, x, 0.5))
        assert bits(got["host"][0]) == bits(got["device"][0]), pair
        assert spmm_slots.same_bits(got["host"][1], got["device"][1]), pair


def test_guard_returns_x_bit_for_bit(own):
    """A = 3 I, B = I, fac = -3: every s_i = 0, so every den_i = 1 and hi = 0"""
    eye = sp.identity(N, format="csr")
    store(own, cheb_ref.raw(3.0 * eye), "ell", cheb_ref.raw(eye), "ell")
    own.spmm_cheb_config(8, F)
    x = panel(N, 5)
    assert own.spmm_cheb_pencil_upper(-3.0) == 0.0
    assert spmm_slots.same_bits(apply(own, x, -3.0), x)
    assert own.spmm_cheb_pencil_upper(0.0) == 1.0


def test_one_step_is_the_diagonal_preconditioner(own):
    a, b = ref.band_pair(6, 2)
    store(own, cheb_ref.raw(a), "ell", cheb_ref.raw(b), "ell")
    own.spmm_cheb_config(1, F)
    x = panel(N, 5)
    fac = 0.5
    hi = own.spmm_cheb_pencil_upper(fac)
    theta = float(cheb_ref.scalars(hi, F * hi, 1)[0])        # (lo = f hi is a double product, theta is rounded once)
    r = 1.0 / ref.scaling(a.diagonal(), b.diagonal(), fac)[2]
    assert spmm_slots.same_bits(apply(own, x, fac), (x * r[:, None]) / theta)


@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_repeated_calls_are_bit_identical_and_booked_per_step(own, d):
    m = 5
    a, b = ref.band_pair(6, 2)
    ia, ib = store(own, cheb_ref.raw(a), "ell", cheb_ref.raw(b), "ell")
    n, wa, wb = N, ia["stored"] // N, ib["stored"] // N
    own.spmm_cheb_config(d, F)
    own.spmm_cheb_pencil_upper(0.5)
    x = panel(n, m)
    own.reset_stats()
    first = apply(own, x, 0.5)
    count, syncs = own.stats()["precnd"]["launches"], own.stats()["host_syncs"]
    assert spmm_slots.same_bits(apply(own, x, 0.5), first)
    assert own.stats()["precnd"]["launches"] == 2 * count and count == 2 + (d - 1)
    ks = own.kernel_stats()
    assert ks["cheb_pencil_bound_kernel"]["launches"] == 2 and ks["cheb_pencil_bound_kernel"]["alg_bytes"] == 2 * 40.0 * n
    assert ks["cheb_jacobi_scale_kernel"]["launches"] == 2 and ks["cheb_jacobi_scale_kernel"]["alg_bytes"] == 2 * (16.0 * n * m + 8.0 * n)
    for other in ("ell_cheb_step_kernel", "ell_cheb_jacobi_step_kernel", "cheb_jacobi_bound_kernel", "cheb_scale_kernel", COMBINE, PANEL["ell"]):
        assert ks.get(other, {"launches": 0})["launches"] == 0, other
    assert own.stats()["matvec"]["launches"] == 0
    if d > 1:
        assert ks[FUSED]["launches"] == 2 * (d - 1)
        assert ks[FUSED]["alg_bytes"] == 2 * (d - 1) * (12.0 * (wa + wb) * n + 32.0 * n * m + 8.0 * n)
        assert ks[FUSED]["flops"] == 2 * (d - 1) * (2.0 * (wa + wb) * n * m + 10.0 * n * m)
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
        assert ctx.lib.dla_spmm_cheb_pencil_upper(ctx.h, 0.0, C.byref(hi)) == capi.ERR_ARG and hi.value == -1.0
        assert cause in spmm_slots.last_error(ctx), spmm_slots.last_error(ctx)


def test_refusals():
    a, b = ref.band_pair(3, 2)
    with spmm_slots.fresh_context() as c:
        # (a refused set-up of A still makes c the context this thread's callbacks act on)
        assert spmm_slots.setup_status(c, "A", 0, *cheb_ref.raw(a)[1:], "ell") == capi.ERR_ARG
        c.spmm_cheb_config(8, F)
        _assert_refused(c, N, "no operator")
        c.spmm_setup(a, "ell")
        _assert_refused(c, N, "no metric")
        c.spmm_setup_metric(b, "ell")
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        _assert_refused(c, N - 1, "n = 776 differs")
        c.spmm_setup(cheb_ref.banded(700, 3), "ell")
        _assert_refused(c, 700, "the operator has 700 rows and the metric 777")
        c.spmm_setup(a, "ell")
        c.spmm_cheb_config(0, F)
        _assert_refused(c, N, "nothing is configured")
        c.spmm_cheb_config(8, F)
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        c.spmm_drop_metric()                            # (a metric beside a row-sharded operator is refused at the set-up)
        c.spmm_setup_sharded(a, 0, N)
        _assert_refused(c, N, "row-sharded")
        c.spmm_setup(a, "ell")                          # (A is whole again)
        c.spmm_setup_metric(b, "sell")
        assert apply(c, panel(N, 3), 0.0).shape == (N, 3)
        assert c.lib.dla_spmm_cheb_pencil_upper(c.h, 0.0, None) == capi.ERR_ARG


def test_the_other_callbacks_are_untouched(own):
    """plain, scaled, pencil, the diagonal of the pencil and the metric's product on one context: they share the configuration and the
    work panels, and nothing else"""
    x = panel(5000, 9)
    own.spmm_cheb_config(8, F)
    for pair in (("banded6", "metric3"), ("skewed", "skewed")):
        store(own, big(pair[0]), big_fmt(pair[0]), big(pair[1]), big_fmt(pair[1]))
        g = own.spmm_cheb_info()["upper"]
        first = [apply(own, x, 0.5, name=PLAIN), apply(own, x, 0.5, name=SCALED), apply(own, x, 0.5), apply(own, x, 0.5, name=DIAG),
                 spmm_slots.product(own, "B", x)]
        assert not spmm_slots.same_bits(first[2], first[1]) and not spmm_slots.same_bits(first[2], first[3])
        again = [apply(own, x, 0.5, name=PLAIN), apply(own, x, 0.5, name=SCALED), apply(own, x, 0.5), apply(own, x, 0.5, name=DIAG),
                 spmm_slots.product(own, "B", x)]
        for k, (p, q) in enumerate(zip(first, again)):
            assert spmm_slots.same_bits(p, q), (pair, k)
        assert bits(own.spmm_cheb_info()["upper"]) == bits(g)


# ------------------------------------------------------------------------------------------------------------------ whole solves
@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("driver", ["davidson", "lobpcg"])
def test_solves_follow_the_oracle(ctx, oracle, driver, fmt):
    """the drivers run on the thread's default context, so this test configures that one, and switches the preconditioner off and drops
    the metric again"""
    import scipy.linalg
    s = ref.SOLVE
    a, b = ref.diffusion(ref.ORDER, ref.CONTRAST), ref.mass(ref.ORDER)
    n, t, n_max = a.shape[0], s["n_targ"], s["n_max"]
    want = scipy.linalg.eigh(a.toarray(), b.toarray(), eigvals_only=True)[:t]
    ok_o, iters_o, _ = ref.oracle_counts(oracle, "pencil")[driver]
    assert ok_o and iters_o == {"davidson": 47, "lobpcg": 36}[driver], (ok_o, iters_o)
    ctx.spmm_setup(a, fmt)
    ctx.spmm_setup_metric(b, fmt)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.spmm_cheb_config(s["steps"], s["lo_fraction"])
    try:
        mv, bv = capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_bvec")
        res = {}
        for pc in (NAME, DIAG):
            ev = ctx.panel(cheb_ref.guess(n, n_max))
            if driver == "davidson":
                eig, _, ok, info = ctx.gen_david_driver(n, t, n_max, s["max_iter"], s["tol"], s["max_dav"], 0.0, mv, capi.fn_address(pc), bv, ev)
            else:
                eig, _, ok, info = ctx.lobpcg_driver(n, t, n_max, s["max_iter"], s["tol"], 0.0, mv, capi.fn_address(pc), ev, bvec=bv)
            res[pc] = (ok, info["iters"], eig[:t].copy())
            ev.free()
    finally:
        ctx.spmm_cheb_config(0, 0.0)
        ctx.spmm_drop_metric()
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ok, iters, eig = res[NAME]
    print("%s, %s: %d iterations, the oracle %d; the diagonal of the pencil: ok = %s after %d" % (driver, fmt, iters, iters_o, res[DIAG][0], res[DIAG][1]))
    assert ok, res
    assert np.allclose(eig, want, rtol=1e-9, atol=0.0), (eig, want)
    assert abs(iters - iters_o) <= max(1, iters_o // 5), (iters, iters_o)
    assert not res[DIAG][0] and res[DIAG][1] >= s["max_iter"], res
