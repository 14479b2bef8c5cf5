"""GPU: the storage formats of the sparse operator -- dla_spmm_setup_csr_fmt (DLA_SPMM_ELL / _SELL / _AUTO), dla_spmm_info,
sell_spmm_kernel and csr_long_rows_kernel behind the unchanged callbacks dla_spmm_matvec / dla_spmm_precnd.

Conventions of tests/test_operators_gpu.py: references in np.longdouble from the raw triplets, outputs between sentinel columns,
inputs checked unchanged.  The bound of a row of len entries is (len + 2) eps |A||x|: len fused multiply-adds in ANY order
(the tail sums 64 strided partial sums through a butterfly) stay below gamma_len, with room for the reference's own rounding.
Sizes sit on the edges of the layout: one slice of 64 rows, a sorting window of 4096, a partial last slice, tail rows whose
length is no multiple of 64; block widths below, at and above the columns a kernel keeps per matrix entry (8 and 4)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from diaglib_amd import capi
from spmm_cases import LONG_ROW, SLICE, WINDOW, csr_from_lengths, fma, skewed_csr
from spmm_slots import setup
from test_operators_gpu import (EPS, LD, N_TRIP, SENT, Guarded, _assert_second_trip, assert_within, call_matvec, call_precnd, csr_diagonal,
                                csr_product_reference, csr_rows, ragged_csr, setup_csr, spmm_product)
from test_spmm_gpu import _laplacian_2d

pytestmark = pytest.mark.gpu
ELL, SELL, AUTO = capi.SPMM_ELL, capi.SPMM_SELL, capi.SPMM_AUTO


@pytest.fixture()
def dev(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def setup_fmt(ctx, *csr_and_format):
    setup(ctx, "A", *csr_and_format)


def check_product(ctx, n, indptr, indices, data, x, what):
    """one product of the operator that is set up against the triplets, row by row; exact zeros on empty rows"""
    m = x.shape[1]
    got = spmm_product(ctx, n, m, x)
    ref, mag = csr_product_reference(indptr, indices, data, x)
    lens = np.diff(indptr)
    ratio = assert_within(got, ref, {"(len+2) eps |A||x|": (lens[:, None] + 2) * EPS * mag, "tiny": LD(1e-300)}, f"{what} n={n} m={m}")
    print(f"{what} n={n} m={m}: worst |got - ref| / bound = {ratio:.3f}")
    assert np.all(got[lens == 0] == 0.0), "an empty row must give exactly 0.0"
    return got


def check_precnd(ctx, rng, n, indptr, indices, data, m):
    """dla_spmm_precnd against x / (diag + fac) with the 1e-5 guard on a matrix of eighths (the expected diagonal is exact), as
    check_spmm_precnd of tests/test_operators_gpu.py does for ELLPACK"""
    diag = csr_diagonal(indptr, indices, data)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    rows = csr_rows(indptr)
    has_diag = np.zeros(n, bool)
    has_diag[rows[indices == rows]] = True
    gx = Guarded(ctx, n, m, x)
    j = int(rng.choice(np.flatnonzero(has_diag))) if has_diag.any() else 0
    facs = [(-diag[j] + delta, delta) for delta in (0.0, 2.0 ** -17, -2.0 ** -17, 2.0 ** -16, -2.0 ** -16)] + [(0.0, None), (1.0, None), (0.5, None)]
    for fac, delta in facs:
        gp = Guarded(ctx, n, m)
        call_precnd(ctx, "dla_spmm_precnd", n, m, fac, gx.ptr, gp.ptr)
        got = gp.body()
        den = (diag + fac)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(np.abs(den) > 1e-5, x / den, x)
        assert_within(got, want.astype(LD), {"4 eps |want|": 4 * EPS * np.abs(want), "tiny": LD(1e-300)}, f"spmm_precnd (sell) n={n} fac={fac!r}")
        if delta is not None and has_diag.any():
            assert diag[j] + fac == delta
            assert np.array_equal(got[j], x[j] if abs(delta) <= 2.0 ** -17 else x[j] / delta), ("the guard", delta)
        elif delta is None:
            assert np.array_equal(got[~has_diag], x[~has_diag] / fac if fac else x[~has_diag]), ("rows without a diagonal entry", fac)
        gp.free()
    gx.assert_unchanged()
    gx.free()


# ------------------------------------------------------------------------------------------------------------------ 1. ragged matrices
# every block width at the small sizes; four each at the window edge; two at n = 20000 (the reference costs nnz x m)
_M_ALL = [1, 3, 4, 5, 7, 8, 9, 13, 37]
SKEWED_CASES = [(1, _M_ALL), (63, _M_ALL), (64, _M_ALL), (65, _M_ALL), (257, _M_ALL), (4095, [1, 7, 13, 37]), (4096, [4, 5, 8, 37]),
                (4097, [3, 5, 9, 13]), (20000, [9, 13])]


@pytest.mark.parametrize("n,ms", SKEWED_CASES, ids=[f"n{n}" for n, _ in SKEWED_CASES])
def test_sell_product_on_skewed_matrices(dev, n, ms):
    """power-law rows, one dense row, one empty row, the last slice row (LONG_ROW entries) and the first tail row (LONG_ROW + 1);
    unsorted uniform columns with duplicates, explicit zeros"""
    rng = np.random.default_rng(1000 + n)
    indptr, indices, data = skewed_csr(rng, n)
    setup_fmt(dev, n, indptr, indices, data, SELL)
    info = dev.spmm_info()
    assert info["format"] == "sell" and info["n"] == n and info["long_rows"] == int((np.diff(indptr) > LONG_ROW).sum())
    for m in ms:
        check_product(dev, n, indptr, indices, data, np.asfortranarray(rng.standard_normal((n, m))), "sell, skewed")
    indptr, indices, data = skewed_csr(rng, n, eighths=True)
    setup_fmt(dev, n, indptr, indices, data, SELL)
    check_precnd(dev, rng, n, indptr, indices, data, 2 if n > 5000 else 5)


# ------------------------------------------------------------------------------------------------------------------ 2. only / no long rows
@pytest.mark.parametrize("m", [1, 5, 13])
def test_sell_with_only_long_rows(dev, rng, m):
    n = 300
    indptr, indices, data = csr_from_lengths(rng, n, rng.integers(LONG_ROW + 1, n + 1, n))
    setup_fmt(dev, n, indptr, indices, data, SELL)
    info = dev.spmm_info()
    assert info["long_rows"] == n and info["stored"] == 0 and info["long_entries"] == int(indptr[-1])
    check_product(dev, n, indptr, indices, data, np.asfortranarray(rng.standard_normal((n, m))), "sell, tail only")


@pytest.mark.parametrize("m", [1, 5, 13])
def test_sell_without_long_rows(dev, rng, m):
    n = 1000
    indptr, indices, data = ragged_csr(rng, n, 33)
    setup_fmt(dev, n, indptr, indices, data, SELL)
    info = dev.spmm_info()
    assert info["long_rows"] == 0 and info["long_entries"] == 0 and info["slices"] == -(-n // SLICE)
    check_product(dev, n, indptr, indices, data, np.asfortranarray(rng.standard_normal((n, m))), "sell, no tail")


# ------------------------------------------------------------------------------------------------------------------ 3. same bits
@pytest.mark.parametrize("w_max", [5, 33, 70])
@pytest.mark.parametrize("n", [257, 5000])
def test_sell_returns_the_bits_of_ellpack(dev, rng, w_max, n):
    """rows that are not in the tail are accumulated in the same order, one fused multiply-add per entry from 0.0"""
    indptr, indices, data = ragged_csr(rng, n, w_max)
    x = np.asfortranarray(rng.standard_normal((n, 13)))
    setup_csr(dev, n, indptr, indices, data)
    assert dev.spmm_info()["format"] == "ell"
    plain = spmm_product(dev, n, 13, x)
    setup_fmt(dev, n, indptr, indices, data, SELL)
    assert dev.spmm_info()["format"] == "sell"
    assert np.array_equal(spmm_product(dev, n, 13, x), plain)
    setup_fmt(dev, n, indptr, indices, data, ELL)
    assert dev.spmm_info()["format"] == "ell"
    assert np.array_equal(spmm_product(dev, n, 13, x), plain)


# widths on both sides of every edge of the ELLPACK width ladder (4, 8, 16, 32) and the loop over any width beyond it; block widths
# below, at and above the 8 columns a slice entry is loaded for
SHORT_W_MAX = [1, 4, 5, 8, 9, 16, 17, 32, 33]
SHORT_M = [1, 8, 9, 13]


def chain_rows(indptr, indices, data, x, step):
    """every (row, column) as one sequential chain over the row's entries in stored order from 0.0: acc = step(value, x[col], acc)"""
    out = np.zeros((len(indptr) - 1, x.shape[1]))
    for i in range(len(indptr) - 1):
        p0, p1 = int(indptr[i]), int(indptr[i + 1])
        vals, cols = data[p0:p1].tolist(), indices[p0:p1]
        for c in range(x.shape[1]):
            acc = 0.0
            for v, xv in zip(vals, x[cols, c].tolist()):
                acc = step(v, xv, acc)
            out[i, c] = acc
    return out


@pytest.fixture(scope="module")
def short_rows():
    """n = 300 (two blocks of 256 rows; five slices, the last one partial), ragged rows of 0 .. w_max entries, 13 columns of x and the
    contract's chain of fused multiply-adds for all 13: computed once per matrix, left unchanged.  The test is sharp only where a
    separately rounded multiply and add gives other bits, which is asserted here for every matrix whose rows can tell the two apart:
    a chain of ONE entry rounds v x once either way, so w_max = 1 cannot (there the two are asserted equal instead)."""
    cases = {}
    for w_max in SHORT_W_MAX:
        rng = np.random.default_rng(5100 + w_max)
        indptr, indices, data = ragged_csr(rng, 300, w_max)
        x = np.asfortranarray(rng.standard_normal((300, 13)))
        fused = chain_rows(indptr, indices, data, x, fma)
        unfused = chain_rows(indptr, indices, data, x, lambda v, xv, acc: v * xv + acc)
        differ = int((fused != unfused).sum())
        print(f"w_max={w_max}: {differ} of {fused.size} elements tell a fused chain from a separately rounded one")
        assert differ > 0 if w_max > 1 else differ == 0, w_max
        for a in (indptr, indices, data, x, fused):
            a.flags.writeable = False
        cases[w_max] = (indptr, indices, data, x, fused)
    return cases


@pytest.mark.parametrize("m", SHORT_M)
@pytest.mark.parametrize("w_max", SHORT_W_MAX)
def test_short_rows_have_the_bits_of_the_contract(dev, short_rows, w_max, m):
    """per row and column the entries are accumulated in stored order, one fused multiply-add each, from 0.0 -- held to an exact
    emulation, in both formats, so that the two cannot change together unnoticed"""
    indptr, indices, data, x, fused = short_rows[w_max]
    n = 300
    for fmt, name in ((ELL, "ell"), (SELL, "sell")):
        setup_fmt(dev, n, indptr, indices, data, fmt)
        assert dev.spmm_info()["format"] == name
        got = spmm_product(dev, n, m, np.asfortranarray(x[:, :m]))
        print(f"{name} w_max={w_max} m={m}: {int((got != fused[:, :m]).sum())} of {got.size} elements differ from the emulation")
        assert np.array_equal(got, fused[:, :m]), (name, w_max, m)


def test_consecutive_sell_products_are_bit_identical(dev):
    n, m = 20000, 13
    rng = np.random.default_rng(7)
    indptr, indices, data = skewed_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    setup_fmt(dev, n, indptr, indices, data, SELL)
    assert np.array_equal(spmm_product(dev, n, m, x), spmm_product(dev, n, m, x))


# ------------------------------------------------------------------------------------------------------------------ 4. storage
@pytest.mark.parametrize("n", [4097, 20000])
@pytest.mark.parametrize("seed", [7, 8, 9])
def test_storage_is_proportional_to_the_nonzeros(dev, n, seed):
    """a condition, not a measurement: at most a quarter more entries than non-zeros, where ELLPACK would need n entries per row"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = skewed_csr(rng, n)
    nnz, lens = int(indptr[-1]), np.diff(indptr)
    for fmt in (SELL, AUTO):
        setup_fmt(dev, n, indptr, indices, data, fmt)
        info = dev.spmm_info()
        print(f"n={n} seed={seed}: {info}; (stored + long_entries) / nnz = {(info['stored'] + info['long_entries']) / nnz:.3f}")
        assert info["format"] == "sell"
        assert (info["slice_rows"], info["sort_window"], info["long_row_threshold"]) == (SLICE, WINDOW, LONG_ROW)
        assert info["n"] == n and info["nnz"] == nnz and info["slices"] == -(-n // SLICE)
        assert info["long_rows"] == int((lens > LONG_ROW).sum()) and info["long_entries"] == int(lens[lens > LONG_ROW].sum())
        assert info["stored"] + info["long_entries"] <= 1.25 * nnz
        assert info["device_bytes"] <= 16 * 1.25 * nnz + 16 * n + 8 * (info["slices"] + info["long_rows"] + 2)


def test_auto_keeps_ellpack_for_a_stencil(dev, rng):
    a = _laplacian_2d(96, 64)
    n = a.shape[0]
    dev.spmm_setup(a, fmt="auto")
    info = dev.spmm_info()
    assert info["format"] == "ell" and info["stored"] == 5 * n and info["nnz"] == a.nnz and info["device_bytes"] == 12 * 5 * n + 8 * n
    assert info["slices"] == info["long_rows"] == info["long_entries"] == info["slice_rows"] == 0
    x = np.asfortranarray(rng.standard_normal((n, 5)))
    auto = spmm_product(dev, n, 5, x)
    dev.spmm_setup(a)
    assert np.array_equal(spmm_product(dev, n, 5, x), auto)
    dev.spmm_setup(a, fmt="sell")
    assert dev.spmm_info()["format"] == "sell"
    assert np.array_equal(spmm_product(dev, n, 5, x), auto)
    with pytest.raises(ValueError):
        dev.spmm_setup(a, fmt="csr")


# ------------------------------------------------------------------------------------------------------------------ 5. second trip
def test_sell_and_its_preconditioner_take_a_second_stride_trip(dev, rng):
    """n = 700 001: 10 938 slices for at most 8 x 4 wavefronts per compute unit -- slices beyond the first trip of the grid-stride
    loop, a partial last slice, and three tail rows"""
    _assert_second_trip()
    n, m = N_TRIP, 2
    lens = rng.integers(0, 6, n)
    lens[rng.choice(n, 3, replace=False)] = 300
    try:
        indptr, indices, data = csr_from_lengths(rng, n, lens)
        setup_fmt(dev, n, indptr, indices, data, SELL)
        assert dev.spmm_info()["long_rows"] == 3
        x = np.asfortranarray(rng.standard_normal((n, m)))
        check_product(dev, n, indptr, indices, data, x, "sell, second trip")
        diag = csr_diagonal(indptr, indices, data)
        gx, gp = Guarded(dev, n, m, x), Guarded(dev, n, m)
        call_precnd(dev, "dla_spmm_precnd", n, m, 0.375, gx.ptr, gp.ptr)
        den = (diag + 0.375)[:, None]
        want = np.where(np.abs(den) > 1e-5, x / den, x)
        # one rounding of the stored diagonal (duplicates summed in another order than here), carried through the division
        assert_within(gp.body(), want.astype(LD), {"4 eps |want|": 4 * EPS * np.abs(want), "diag rounding": 4 * EPS * np.abs(want) * np.abs(diag[:, None] / den)},
                      "spmm_precnd (sell) at n = 700 001")
        gx.assert_unchanged()
        gx.free(); gp.free()
    finally:
        dev.trim()


# ------------------------------------------------------------------------------------------------------------------ 6. replacement
def test_either_format_replaces_the_other(dev, rng):
    """ELL(5000) -> SELL(100) -> ELL(257) -> SELL(20000) on one context: the blocks are shared and only grow, the kernels go by the
    operator set up last; a product with the stale n is refused; a refused setup leaves the previous operator's bits intact"""
    def product(n, mat, m):
        return check_product(dev, n, *mat, np.asfortranarray(np.random.default_rng(n).standard_normal((n, m))), "replacement")

    def refused_with_stale_n(n):
        gx, gy = Guarded(dev, n, 2, np.ones((n, 2))), Guarded(dev, n, 2)
        with pytest.raises(capi.DlaError, match="n differs from setup"):
            call_matvec(dev, "dla_spmm_matvec", n, 2, gx.ptr, gy.ptr)
        with pytest.raises(capi.DlaError, match="n differs from setup"):
            call_precnd(dev, "dla_spmm_precnd", n, 2, 1.0, gx.ptr, gy.ptr)
        assert np.all(gy.body() == SENT)
        gx.free(); gy.free()

    def bad_setups_leave(n, mat, m, before):
        idx, val = np.zeros(8, np.int32), np.ones(8)
        ok = np.array([0, 1, 2, 3, 3, 3, 3], np.int64)
        with pytest.raises(capi.DlaError, match="column index out of range"):
            setup_fmt(dev, 6, ok, np.array([0, 6, 1, 0, 0, 0, 0, 0], np.int32), val, SELL)
        assert np.array_equal(product(n, mat, m), before)
        with pytest.raises(capi.DlaError, match="unknown format"):
            setup_fmt(dev, 6, ok, idx, val, 3)
        assert np.array_equal(product(n, mat, m), before)

    m1 = ragged_csr(rng, 5000, 41)
    setup_csr(dev, 5000, *m1)
    product(5000, m1, 3)
    m2 = skewed_csr(rng, 100)
    setup_fmt(dev, 100, *m2, SELL)
    before = product(100, m2, 5)
    refused_with_stale_n(5000)
    bad_setups_leave(100, m2, 5, before)
    m3 = ragged_csr(rng, 257, 9)
    setup_fmt(dev, 257, *m3, ELL)
    before = product(257, m3, 2)
    refused_with_stale_n(100)
    bad_setups_leave(257, m3, 2, before)
    m4 = skewed_csr(rng, 20000)
    setup_fmt(dev, 20000, *m4, SELL)
    before = product(20000, m4, 9)
    refused_with_stale_n(257)
    bad_setups_leave(20000, m4, 9, before)


def test_info_before_any_setup_is_refused():
    """on a context of its own: the session's context has an operator from earlier tests"""
    lib = capi.load()
    h = C.c_void_p()
    assert lib.dla_create(C.byref(h), 0) == 0
    try:
        assert lib.dla_spmm_info(h, C.byref(capi.SpmmInfo())) == capi.ERR_ARG
    finally:
        lib.dla_destroy(h)


# ------------------------------------------------------------------------------------------------------------------ 7. a whole solve
def _arrow_power_law_matrix(n, half=6):
    """the matrix of test_solve_with_the_sparse_operator_on_the_device (diagonal i + 1, a band of 1 / (i + j) couplings) plus what
    makes it ragged: a power-law pattern P + P^T with entries 0.01 N(0, 1) and two arrow rows and columns that couple rows 0 and 1
    to everything with 0.1 / (i + j + 2)"""
    rng = np.random.default_rng(11)
    idx = np.arange(1.0, n + 1.0)
    band = sp.diags([1.0 / (idx[:-k] + idx[k:]) for k in range(1, half + 1)], list(range(1, half + 1)), shape=(n, n))
    lens = np.minimum(n, (3.0 * (1.0 + rng.pareto(1.2, n))).astype(np.int64))
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, rows.size)
    off = rows != cols
    p = sp.coo_matrix((0.01 * rng.standard_normal(int(off.sum())), (rows[off], cols[off])), shape=(n, n))
    i = np.arange(2, n)
    arrow = sp.coo_matrix((np.concatenate([0.1 / (i + 2.0), 0.1 / (i + 3.0)]), (np.repeat([0, 1], n - 2), np.concatenate([i, i]))), shape=(n, n))
    return (band + band.T + p + p.T + arrow + arrow.T + sp.diags(idx + 1.0)).tocsr()


@pytest.fixture(scope="module")
def solve_case():
    n, t = 20000, 6
    a = _arrow_power_law_matrix(n)
    diag = a.diagonal()

    # shift-invert at 0 with an inner solve by Jacobi-preconditioned CG to 1e-14: a sparse LU of this pattern fills the matrix
    def solve(b):
        x, bad = spl.cg(a, b, rtol=1e-14, atol=0.0, M=sp.diags(1.0 / diag), maxiter=1000)
        assert bad == 0
        return x
    want = np.sort(spl.eigsh(a, k=t, sigma=0.0, which="LM", return_eigenvectors=False, OPinv=spl.LinearOperator((n, n), matvec=solve, dtype=np.float64)))
    return a, diag, want


@pytest.mark.parametrize("solver", ["davidson", "lobpcg"])
def test_solve_with_the_sliced_operator_on_the_device(ctx, oracle, solve_case, solver):
    """the assertions of test_solve_with_the_sparse_operator_on_the_device on a matrix ELLPACK could not hold (two rows of n entries)"""
    a, diag, want = solve_case
    n, t, m = a.shape[0], 6, 11
    g = np.asfortranarray(np.random.default_rng(5).random((n, m)) - 0.5)
    g[200:] *= 1e-3
    ctx.spmm_setup(a, fmt="sell")
    info_op = ctx.spmm_info()
    w = int(np.diff(a.indptr).max())
    assert w == n and info_op["format"] == "sell" and info_op["long_rows"] >= 2
    assert info_op["device_bytes"] < 12 * w * n / 100, info_op
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    try:
        ev = ctx.panel(g)
        mv, pc = capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_precnd")
        if solver == "davidson":
            eig, _, ok, info = ctx.davidson_driver(n, t, m, 500, 1e-9, 20, 0.0, mv, pc, ev)
        else:
            eig, _, ok, info = ctx.lobpcg_driver(n, t, m, 500, 1e-9, 0.0, mv, pc, ev)
        vec = ev.download()
    finally:
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    assert ok, info

    c_dp, c_ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def h_mv(pn, pm, px, pax):
        k = pm[0]
        np.ctypeslib.as_array(pax, (k, n)).T[:, :] = a @ np.ctypeslib.as_array(px, (k, n)).T

    def h_pc(pn, pm, pf, px, ppx):
        k = pm[0]
        x = np.ctypeslib.as_array(px, (k, n)).T
        den = diag + pf[0]
        np.ctypeslib.as_array(ppx, (k, n)).T[:, :] = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)

    cmv = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp)(h_mv)
    cpc = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)(h_pc)
    amv, apc = C.cast(cmv, C.c_void_p).value, C.cast(cpc, C.c_void_p).value
    if solver == "davidson":
        eo, vo, oko, tr = oracle.davidson(n, t, m, 500, 1e-9, 20, 0.0, amv, apc, g)
    else:
        eo, vo, oko, tr = oracle.lobpcg(n, t, m, 500, 1e-9, 0.0, amv, apc, g)
    assert oko
    print(f"{solver}: iterations {info['iters']} (oracle {tr.iters}), max rel. eigenvalue difference {np.abs(eig[:t] / eo[:t] - 1).max():.2e}")
    assert np.allclose(eig[:t], eo[:t], rtol=1e-9, atol=0)
    assert abs(info["iters"] - tr.iters) <= max(2, tr.iters // 10), (info, tr.iters)
    assert np.allclose(eig[:t], want, rtol=1e-7, atol=0)
    x = vec[:, :t]
    assert np.abs(x.T @ x - np.eye(t)).max() < 1e-10
    assert np.linalg.norm(a @ x - x * eig[None, :t], axis=0).max() < 1e-6
