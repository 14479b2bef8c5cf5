"""GPU: the sparse metric of a generalised problem A x = lambda B x beside the sparse operator -- dla_spmm_setup_metric_csr,
dla_spmm_metric_info, dla_spmm_drop_metric, dla_spmm_bvec (bvec of reference diaglib.f90:1855) and dla_spmm_precnd_pencil
(pencil_precnd_kernel), and whole gen_david_driver / lobpcg_driver(gen_eig) solves that stay in HBM.

Oracles: scipy.sparse for the products (the dot-product bound 64 eps |B| |x| tests/test_spmm_gpu.py holds A to), the operator slot
for the bits of B x (the same kernels on a second instance of the storage), the oracle's gen_davidson / lobpcg_gen with the same
pencil applied by scipy on the host and scipy.linalg.eigh of the dense pencil for the solves.

Where a matrix has rows longer than 62 entries (the skewed ones: rows of up to 256 entries in the slices, one dense row in the CSR
tail) 64 eps |B||x| is not a worst-case bound but the bound of the existing product test carried over: the rounding errors of a sum
of len terms grow like sqrt(len) eps |B||x| (16 for the longest slice row; the tail row sums 64 lanes of n / 64 terms through a
butterfly, sqrt(n / 64 + 6) < 10 at n = 5000), a quarter of the bound at the most."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from diaglib_amd import capi
from spmm_cases import LONG_ROW, skewed_csr
from test_operators_gpu import EPS, Guarded, call_precnd, csr_product_reference, setup_csr, setup_csr_one_shard
from spmm_slots import product, setup, within_scipy_bound
from test_spmm_gpu import _banded, _laplacian_2d

pytestmark = pytest.mark.gpu
FMT = capi.SPMM_FORMATS


@pytest.fixture()
def dev(ctx):
    """device callbacks on; the session's context is handed back without a metric"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.spmm_drop_metric()


def setup_fmt(ctx, *csr_and_format):
    setup(ctx, "A", *csr_and_format)


def setup_metric(ctx, *csr_and_format):
    setup(ctx, "B", *csr_and_format)


def within_bound_raw(got, indptr, indices, data, x):
    ref, mag = csr_product_reference(indptr, indices, data, x)
    return np.all(np.abs(got.astype(np.longdouble) - ref) <= 64 * EPS * mag + 1e-300)


def _matrix(kind, n, rng):
    if kind == "lap":
        return _laplacian_2d(301, n // 301)
    return _banded(n, int(kind[4:]), rng)


# ------------------------------------------------------------------------------------------------------------------ 1. bvec against scipy
@pytest.mark.parametrize("kind,n,m", [("band3", 5000, 8), ("lap", 301 * 7, 5), ("band20", 2000, 3)])
def test_bvec_matches_scipy_beside_another_operator(dev, rng, kind, n, m):
    b = _matrix(kind, n, rng)
    a = _banded(n, 2, rng)                      # another matrix, another width bucket
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dev.spmm_setup(a)
    dev.spmm_setup_metric(b)
    got = product(dev, "dla_spmm_bvec", x)
    assert within_scipy_bound(got, b, x)
    gota = product(dev, "dla_spmm_matvec", x)
    assert within_scipy_bound(gota, a, x)
    assert not np.array_equal(got, gota)


# ------------------------------------------------------------------------------------------------------------------ 2. the operator's bits
@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_bvec_returns_the_bits_of_the_operator_slot(dev, rng, fmt):
    """one matrix as A and as metric; 13 columns = one full chunk of 8 right-hand sides and a ragged one"""
    n, m = 5000, 13
    x = np.asfortranarray(rng.standard_normal((n, m)))
    if fmt == "ell":
        a = _banded(n, 3, rng)
        dev.spmm_setup(a)
        dev.spmm_setup_metric(a)
    else:
        mat = skewed_csr(rng, n)
        lens = np.diff(mat[0])
        assert (lens == LONG_ROW + 1).any() and lens.max() == n           # a tail row just above the threshold and the dense row
        setup_fmt(dev, n, *mat, FMT["sell"])
        setup_metric(dev, n, *mat, FMT["sell"])
        assert dev.spmm_metric_info()["long_rows"] >= 2 and dev.spmm_metric_info()["slices"] == -(-n // 64)
    assert dev.spmm_info()["format"] == dev.spmm_metric_info()["format"] == fmt
    assert np.array_equal(product(dev, "dla_spmm_bvec", x), product(dev, "dla_spmm_matvec", x))


# ------------------------------------------------------------------------------------------------------------------ 3. A is untouched
def test_the_operator_is_untouched_by_a_metric(dev, rng):
    n, m = 2000, 5
    a, b = _banded(n, 3, rng), _banded(n, 5, rng)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dev.spmm_drop_metric()
    dev.spmm_setup(a)
    info0, ax0 = dev.spmm_info(), product(dev, "dla_spmm_matvec", x)
    dev.spmm_setup_metric(b, fmt="sell")
    mi = dev.spmm_metric_info()
    assert (mi["format"], mi["n"], mi["nnz"]) == ("sell", n, b.nnz) and b.nnz <= mi["stored"] <= 11 * 64 * -(-n // 64)
    assert dev.spmm_info() == info0 and np.array_equal(product(dev, "dla_spmm_matvec", x), ax0)
    dev.spmm_setup_metric(b)
    mi = dev.spmm_metric_info()
    assert (mi["format"], mi["n"], mi["nnz"], mi["stored"]) == ("ell", n, b.nnz, 11 * n)
    assert dev.spmm_info() == info0 and np.array_equal(product(dev, "dla_spmm_matvec", x), ax0)
    dev.spmm_drop_metric()
    assert dev.spmm_info() == info0 and np.array_equal(product(dev, "dla_spmm_matvec", x), ax0)
    with pytest.raises(capi.DlaError, match="no metric"):
        dev.spmm_metric_info()
    dev.spmm_drop_metric()                      # (nothing to drop: no error)


# ------------------------------------------------------------------------------------------------------------------ 4. mixed formats
def test_operator_and_metric_in_different_formats(dev, rng):
    n, m = 5000, 13
    band = _banded(n, 3, rng)
    skew = skewed_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dev.spmm_setup(band, fmt="ell")
    setup_metric(dev, n, *skew, FMT["sell"])
    assert (dev.spmm_info()["format"], dev.spmm_metric_info()["format"]) == ("ell", "sell")
    assert within_scipy_bound(product(dev, "dla_spmm_matvec", x), band, x)
    assert within_bound_raw(product(dev, "dla_spmm_bvec", x), *skew, x)
    setup_fmt(dev, n, *skew, FMT["sell"])
    dev.spmm_setup_metric(band, fmt="ell")
    assert (dev.spmm_info()["format"], dev.spmm_metric_info()["format"]) == ("sell", "ell")
    assert within_bound_raw(product(dev, "dla_spmm_matvec", x), *skew, x)
    assert within_scipy_bound(product(dev, "dla_spmm_bvec", x), band, x)


# ------------------------------------------------------------------------------------------------------------------ 5. pencil preconditioner
@pytest.mark.parametrize("n,m,fmt_b", [(2001, 5, "ell"), (700, 1, "sell")])
def test_pencil_preconditioner(dev, rng, n, m, fmt_b):
    """px = x / (a_ii + fac b_ii) with the 1e-5 guard; row `hit` has a_ii = 1.25 b_ii exactly (2.5 and 2.0), so that fac = -1.25
    takes the guard there and nowhere else: elsewhere a_ii >= 2.01 and 1.25 b_ii <= 1.5625"""
    fac, hit = -1.25, n // 3
    a, b = _banded(n, 3, rng).tolil(), _banded(n, 2, rng).tolil()
    b.setdiag(1.0 + 0.25 * np.sin(0.003 * np.arange(n)) ** 2)
    a[hit, hit], b[hit, hit] = 2.5, 2.0
    a, b = a.tocsr(), b.tocsr()
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dev.spmm_setup(a)
    dev.spmm_setup_metric(b, fmt=fmt_b)
    gx, gp = Guarded(dev, n, m, x), Guarded(dev, n, m)
    call_precnd(dev, "dla_spmm_precnd_pencil", n, m, fac, gx.ptr, gp.ptr)
    got = gp.body()
    gx.assert_unchanged()
    den = a.diagonal() + fac * b.diagonal()
    assert den[hit] == 0.0 and np.abs(np.delete(den, hit)).min() > 0.4
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)
    assert np.abs(got - want).max() <= 4 * EPS * np.abs(want).max()
    assert np.array_equal(got[hit], x[hit])
    # the harness' preconditioner is what it was: the operator's diagonal alone
    call_precnd(dev, "dla_spmm_precnd", n, m, fac, gx.ptr, gp.ptr)
    den = a.diagonal() + fac
    wantp = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)
    assert np.abs(gp.body() - wantp).max() <= 4 * EPS * np.abs(wantp).max()
    # booked: one launch each under no kernel name, with the bytes and flops of the elementwise pass
    for name, nbytes, flops in (("dla_spmm_precnd_pencil", 16.0 * n * m + 16.0 * n, 2.0 * n * m), ("dla_spmm_precnd", 8.0 * n * (2.0 * m + 1.0), 1.0 * n * m)):
        dev.reset_stats()
        call_precnd(dev, name, n, m, fac, gx.ptr, gp.ptr)
        dev.sync()
        assert not any(v["launches"] for v in dev.kernel_stats().values()), dev.kernel_stats()
        pc = dev.stats()["precnd"]
        assert (pc["launches"], pc["alg_bytes"], pc["flops"]) == (1, nbytes, flops), pc
    gx.free(); gp.free()


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def _status_and_message(ctx, kind, name, n, m=2):
    gx, gy = Guarded(ctx, n, m, np.ones((n, m))), Guarded(ctx, n, m)
    if kind == "matvec":
        st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, gx.ptr, gy.ptr)
    else:
        st = ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, -1.25, gx.ptr, gy.ptr)
    msg = ctx.lib.dla_last_error(ctx.h).decode()
    assert np.all(gy.body() == 7.0), "a refused callback wrote its output block"
    gx.free(); gy.free()
    return st, msg


def test_callbacks_refuse_a_missing_or_mismatched_matrix(dev, rng):
    n = 1000
    a = _banded(n, 3, rng)
    dev.spmm_setup(a)
    dev.spmm_drop_metric()
    for kind, name in (("matvec", "dla_spmm_bvec"), ("precnd", "dla_spmm_precnd_pencil")):
        st, msg = _status_and_message(dev, kind, name, n)
        assert st != 0 and name in msg and "no metric" in msg, (st, msg)
    dev.spmm_setup_metric(_banded(n - 100, 2, rng))
    st, msg = _status_and_message(dev, "matvec", "dla_spmm_bvec", n)
    assert st != 0 and "dla_spmm_bvec" in msg and "n differs" in msg, (st, msg)
    for n_call in (n, n - 100):
        st, msg = _status_and_message(dev, "precnd", "dla_spmm_precnd_pencil", n_call)
        assert st != 0 and "dla_spmm_precnd_pencil" in msg and "1000 rows and the metric 900" in msg, (st, msg)
    # the context goes on working
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    assert within_scipy_bound(product(dev, "dla_spmm_matvec", x), a, x)


def test_a_refused_metric_setup_replaces_nothing(dev, rng):
    n, m = 1500, 5
    a = _banded(n, 2, rng)
    mat = skewed_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dev.spmm_setup(a)
    setup_metric(dev, n, *mat, FMT["sell"])
    info, before, ax = dev.spmm_metric_info(), product(dev, "dla_spmm_bvec", x), product(dev, "dla_spmm_matvec", x)
    ok, val = np.array([0, 1, 2, 3, 3, 3, 3], np.int64), np.ones(8)
    with pytest.raises(capi.DlaError, match="spmm_setup_metric_csr.*column index out of range"):
        setup_metric(dev, 6, ok, np.array([0, 6, 1, 0, 0, 0, 0, 0], np.int32), val, FMT["sell"])
    assert dev.spmm_metric_info() == info and np.array_equal(product(dev, "dla_spmm_bvec", x), before)
    with pytest.raises(capi.DlaError, match="spmm_setup_metric_csr.*column index out of range"):
        setup_metric(dev, 6, ok, np.array([0, -1, 1, 0, 0, 0, 0, 0], np.int32), val, FMT["ell"])
    assert dev.spmm_metric_info() == info and np.array_equal(product(dev, "dla_spmm_bvec", x), before)
    with pytest.raises(capi.DlaError, match="spmm_setup_metric_csr.*unknown format"):
        setup_metric(dev, 6, ok, np.zeros(8, np.int32), val, 3)
    assert dev.spmm_metric_info() == info and np.array_equal(product(dev, "dla_spmm_bvec", x), before)
    with pytest.raises(ValueError):
        dev.spmm_setup_metric(a, fmt="csr")
    assert np.array_equal(product(dev, "dla_spmm_matvec", x), ax)


def test_a_sharded_operator_and_a_metric_exclude_each_other(dev, rng):
    """a row-sharded metric does not exist: the metric is refused beside a sharded operator, the sharded setup beside a metric"""
    n = 600
    a = _banded(n, 3, rng)
    ia, ja, va = a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)
    x = np.asfortranarray(rng.standard_normal((n, 3)))
    dev.spmm_drop_metric()
    setup_csr_one_shard(dev, n, ia, ja, va)
    ax = product(dev, "dla_spmm_matvec", x)
    with pytest.raises(capi.DlaError, match="spmm_setup_metric_csr.*row-sharded"):
        dev.spmm_setup_metric(a)
    with pytest.raises(capi.DlaError, match="no metric"):
        dev.spmm_metric_info()
    assert np.array_equal(product(dev, "dla_spmm_matvec", x), ax)
    setup_csr(dev, n, ia, ja, va)
    dev.spmm_setup_metric(a)
    bx = product(dev, "dla_spmm_bvec", x)
    with pytest.raises(capi.DlaError, match="spmm_setup_csr_sharded.*metric"):
        setup_csr_one_shard(dev, n, ia, ja, va)
    assert np.array_equal(product(dev, "dla_spmm_bvec", x), bx) and np.array_equal(product(dev, "dla_spmm_matvec", x), ax)


# ------------------------------------------------------------------------------------------------------------------ 7. whole solves
N, T, M = 3000, 6, 11


@pytest.fixture(scope="module")
def pencil():
    """A: the sparse band of tests/test_spmm_gpu.py (diagonal i + 1, six off-diagonals 1 / (i + j)).  B: diagonal
    1 + 0.25 sin^2(0.003 i), off-diagonals k = 1, 2 of 0.15 / k cos(0.01 i): the off-diagonal row sums stay below 0.45, so B is
    strictly diagonally dominant and positive definite.  The lowest pairs come from the dense eigensolver, once."""
    idx = np.arange(1.0, N + 1.0)
    a = sp.diags([1.0 / (idx[:-k] + idx[k:]) for k in range(1, 7)], list(range(1, 7)), shape=(N, N))
    a = (a + a.T + sp.diags(idx + 1.0)).tocsr()
    i = np.arange(N, dtype=np.float64)
    b = sp.diags([0.15 / k * np.cos(0.01 * i[:N - k]) for k in (1, 2)], [1, 2], shape=(N, N))
    b = (b + b.T + sp.diags(1.0 + 0.25 * np.sin(0.003 * i) ** 2)).tocsr()
    g = np.asfortranarray(np.random.default_rng(5).random((N, M)) - 0.5)
    g[200:] *= 1e-3
    want = sl.eigh(a.toarray(), b.toarray(), eigvals_only=True, subset_by_index=[0, T - 1])
    return {"a": a, "b": b, "guess": g, "dense": want, "oracle": {}}


def _oracle_solve(oracle, pencil, solver, precnd):
    """the oracle's driver with the pencil applied by scipy on the host; one run per (solver, preconditioner), shared"""
    key = (solver, precnd)
    if key in pencil["oracle"]:
        return pencil["oracle"][key]
    a, b = pencil["a"], pencil["b"]
    da, db = a.diagonal(), b.diagonal()
    c_dp, c_ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def blocks(pm, *ptrs):
        return [np.ctypeslib.as_array(p, (pm[0], N)).T for p in ptrs]

    def h_mv(pn, pm, px, pax):
        x, ax = blocks(pm, px, pax)
        ax[:, :] = a @ x

    def h_bv(pn, pm, px, pbx):
        x, bx = blocks(pm, px, pbx)
        bx[:, :] = b @ x

    def h_pc(pn, pm, pf, px, ppx):
        x, y = blocks(pm, px, ppx)
        den = da + pf[0] * db if precnd == "pencil" else da + pf[0]
        y[:, :] = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)

    mv_t, pc_t = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp), C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)
    cmv, cbv, cpc = mv_t(h_mv), mv_t(h_bv), pc_t(h_pc)
    amv, abv, apc = (C.cast(f, C.c_void_p).value for f in (cmv, cbv, cpc))
    if solver == "gen_david":
        eo, vo, oko, tr = oracle.gen_davidson(N, T, M, 500, 1e-9, 20, 0.0, amv, apc, abv, pencil["guess"])
    else:
        eo, vo, oko, tr = oracle.lobpcg_gen(N, T, M, 500, 1e-9, 0.0, amv, apc, abv, pencil["guess"])
    assert oko
    pencil["oracle"][key] = (eo, tr.iters)
    return pencil["oracle"][key]


@pytest.mark.parametrize("solver,precnd,fmt_b", [("gen_david", "harness", "ell"), ("gen_david", "pencil", "ell"), ("lobpcg", "harness", "ell"),
                                                 ("lobpcg", "pencil", "ell"), ("gen_david", "harness", "sell")])
def test_generalised_solve_with_the_sparse_pencil_on_the_device(ctx, oracle, pencil, solver, precnd, fmt_b):
    """panels, both matrices and the preconditioner stay in HBM through the whole solve"""
    a, b = pencil["a"], pencil["b"]
    ctx.spmm_setup(a)
    ctx.spmm_setup_metric(b, fmt=fmt_b)
    assert ctx.spmm_metric_info()["format"] == fmt_b
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    try:
        ev = ctx.panel(pencil["guess"])
        mv, bv = capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_bvec")
        pc = capi.fn_address("dla_spmm_precnd_pencil" if precnd == "pencil" else "dla_spmm_precnd")
        if solver == "gen_david":
            eig, _, ok, info = ctx.gen_david_driver(N, T, M, 500, 1e-9, 20, 0.0, mv, pc, bv, ev)
        else:
            eig, _, ok, info = ctx.lobpcg_driver(N, T, M, 500, 1e-9, 0.0, mv, pc, ev, bvec=bv)
        vec = ev.download()
    finally:
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
        ctx.spmm_drop_metric()
    assert ok, info
    eo, iters = _oracle_solve(oracle, pencil, solver, precnd)
    print(f"{solver} / {precnd} / metric in {fmt_b}: iterations {info['iters']} (oracle {iters}), "
          f"max rel. eigenvalue difference to the oracle {np.abs(eig[:T] / eo[:T] - 1).max():.2e}, to eigh {np.abs(eig[:T] / pencil['dense'] - 1).max():.2e}")
    assert np.allclose(eig[:T], eo[:T], rtol=1e-9, atol=0)
    assert np.allclose(eig[:T], pencil["dense"], rtol=1e-9, atol=0)
    assert abs(info["iters"] - iters) <= max(2, iters // 10), (info, iters)
    x = vec[:, :T]
    bx = b @ x
    assert np.abs(x.T @ bx - np.eye(T)).max() < 1e-10
    assert np.linalg.norm(a @ x - bx * eig[None, :T], axis=0).max() < 1e-6
