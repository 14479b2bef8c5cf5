"""GPU: the device-resident dense operator and metric (include/diaglib_amd.h, dla_dense_setup): the product kernel
dense_mfma_kernel on the stored copy, the combining kernel of a split contraction, the two diagonal preconditioners, the slots'
independence and refusals, and whole solves of the reference harness' dense problem (main.f90:311-317) in device mode against
the golden fixtures of the unmodified reference.

Outputs sit between sentinel columns and inputs between NaN columns (as in tests/test_dense_sweeps_gpu.py): nothing outside the
n x m result is written, nothing outside the n x m input is read."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SENTINEL = -7.25e77
SIZES = [1, 15, 16, 17, 63, 65, 130, 1000, 2049]
WIDTHS = [1, 8, 16, 17, 48, 49]
MUL = {0: "dla_dense_matvec", 1: "dla_dense_bvec"}


@pytest.fixture(autouse=True)
def _device_callbacks_and_empty_slots(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield
    ctx.dense_drop(False)
    ctx.dense_drop(True)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def setup_host(ctx, which, a, lda):
    """dla_dense_setup of a held in the leading n rows of an lda x n column-major array (the rest: NaN)"""
    n = a.shape[0]
    held = np.full((lda, n), np.nan, order="F")
    held[:n, :] = a
    ctx._chk(ctx.lib.dla_dense_setup(ctx.h, which, n, held.ctypes.data, lda))


def setup_device(ctx, which, a, lda):
    """dla_dense_setup_dev of the same array in device memory; the array is freed before anything is multiplied"""
    n = a.shape[0]
    held = np.full((lda, n), np.nan, order="F")
    held[:n, :] = a
    p = ctx.panel(held)
    ctx._chk(ctx.lib.dla_dense_setup_dev(ctx.h, which, n, p.ptr, lda))
    p.zero()
    ctx.sync()
    p.free()


def guarded(ctx, call, x, cols_out=None):
    """call(x_ptr, y_ptr) on an input between NaN columns and an output between sentinel columns; returns the n x m output"""
    n, m = x.shape
    xin = np.full((n, m + 2), np.nan, order="F")
    xin[:, 1:m + 1] = x
    px, py = ctx.panel(xin), ctx.panel(np.full((n, m + 2), SENTINEL, order="F"))
    ctx._chk(call(px.col(1, m).ptr, py.col(1, m).ptr))
    out, xafter = py.download(), px.download()
    assert np.all(out[:, 0] == SENTINEL) and np.all(out[:, m + 1] == SENTINEL), "the columns beside the result were written"
    assert np.array_equal(xafter[:, 1:m + 1], x) and np.all(np.isnan(xafter[:, [0, m + 1]])), "the input was changed"
    return out[:, 1:m + 1]


def product(ctx, which, x):
    n, m = x.shape
    return guarded(ctx, lambda xp, yp: ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(MUL[which]), n, m, xp, yp), x)


def precondition(ctx, name, fac, x):
    n, m = x.shape
    return guarded(ctx, lambda xp, yp: ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, fac, xp, yp), x)


def last_error(ctx):
    return ctx.lib.dla_last_error(ctx.h).decode()


# ------------------------------------------------------------------ 1. the exact product
@pytest.mark.parametrize("n", SIZES)
def test_integer_products_are_exact_in_both_slots_from_host_and_device_arrays(ctx, n):
    """entries in [-8, 8]: every order of summation is exact, so the result equals a @ x bit for bit"""
    rng = np.random.default_rng(2000 + n)
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)           # not symmetric
    xs = {m: rng.integers(-8, 9, (n, m)).astype(np.float64) for m in WIDTHS}
    for which, setup, lda in ((0, setup_host, n), (1, setup_device, n + 3), (0, setup_device, n), (1, setup_host, n + 3)):
        setup(ctx, which, a, lda)
        info = ctx.dense_info(bool(which))
        assert info["n"] == n and info["n_pad"] == -(-n // 16) * 16 and info["device_bytes"] == 8 * info["n_pad"] ** 2 + 8 * n
        for m in WIDTHS:
            got = product(ctx, which, xs[m])
            assert np.array_equal(got, a @ xs[m]), (n, m, which, setup.__name__, lda)


@pytest.mark.parametrize("n", SIZES)
def test_host_and_device_set_up_store_the_same_bits_and_products_repeat(ctx, n):
    rng = np.random.default_rng(3000 + n)
    a = rng.standard_normal((n, n))
    setup_host(ctx, 0, a, n + 3)
    setup_device(ctx, 1, a, n)
    for m in (1, 13, 37, 49):
        x = rng.standard_normal((n, m))
        first = product(ctx, 0, x)
        assert np.array_equal(first, product(ctx, 1, x)), (n, m)
        assert np.array_equal(first, product(ctx, 0, x)), (n, m)


def test_set_up_from_a_column_major_torch_view_and_refusal_of_other_tensors(ctx):
    import torch
    n, lda = 65, 70
    rng = np.random.default_rng(5)
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)
    buf = np.zeros((n, lda))
    buf[:, :n] = a.T                                       # buf[k, i] = a(i, k): a(lda, n) column-major
    t = torch.from_numpy(buf).cuda()
    ctx.dense_setup(t.T[:n, :])
    x = rng.integers(-8, 9, (n, 5)).astype(np.float64)
    assert np.array_equal(product(ctx, 0, x), a @ x)
    ctx.dense_setup(a, metric=True)                        # a NumPy array, C-ordered: made Fortran-ordered
    assert np.array_equal(product(ctx, 1, x), a @ x)
    for bad in (t[:, :n], t.T[:n, :].float(), torch.from_numpy(a), t.T[:n, :5]):
        with pytest.raises(ValueError, match="dense_setup"):
            ctx.dense_setup(bad)
    with pytest.raises(ValueError, match="dense_setup"):
        ctx.dense_setup(np.zeros((3, 4)))
    assert np.array_equal(product(ctx, 0, x), a @ x)


# ------------------------------------------------------------------ 2. the bound
_REFS = {}


def bound_case(n):
    """a non-symmetric standard-normal matrix, a block of 49 columns and their long-double product and magnitude product, once per n"""
    if n not in _REFS:
        rng = np.random.default_rng(4000 + n)
        a, x = rng.standard_normal((n, n)), rng.standard_normal((n, 49))
        al, xl = a.astype(LD), x.astype(LD)
        _REFS[n] = (a, x, al @ xl, np.abs(al) @ np.abs(xl), al.T @ xl)
        for v in _REFS[n]:
            v.setflags(write=False)
    return _REFS[n]


@pytest.mark.parametrize("m", [1, 13, 37, 49])
@pytest.mark.parametrize("n", [65, 1000, 2049])
def test_random_products_stay_within_the_contract_bound(ctx, n, m):
    """|got - ref| <= (n + 2) eps (|A| |x|)_i element-wise against the long-double product (the bound of the tail-row contract: it
    holds for any order of summation of n products).  The matrix is not symmetric: the transposed product breaks the bound."""
    a, x, ref, mag, ref_t = bound_case(n)
    setup_host(ctx, 0, a, n)
    got = product(ctx, 0, np.array(x[:, :m]))
    bound = (n + 2) * LD(EPS) * mag[:, :m]
    err = np.abs(got.astype(LD) - ref[:, :m])
    print(f"n={n} m={m}: max err / bound = {float((err / bound).max()):.3e}")
    assert np.all(err <= bound)
    assert not np.all(np.abs(ref_t[:, :m] - ref[:, :m]) <= bound), "the transposed product must fail the bound"


# ------------------------------------------------------------------ 3. one pass
@pytest.mark.parametrize("n,m", [(1000, 1), (1000, 13), (2049, 37), (2049, 48), (130, 17)])
def test_one_launch_of_the_product_kernel_per_block_of_at_most_48_columns(ctx, n, m):
    rng = np.random.default_rng(7)
    setup_host(ctx, 0, rng.standard_normal((n, n)), n)
    x = ctx.panel(rng.standard_normal((n, m)))
    y = ctx.panel(n, m)
    ctx.reset_stats()
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_dense_matvec"), n, m, x.ptr, y.ptr))
    ctx.sync()
    ks = {k: v for k, v in ctx.kernel_stats().items() if v["launches"]}
    name = f"dense_mfma_kernel<{-(-m // 16)}>"
    assert ks[name]["launches"] == 1 and set(ks) <= {name, "dense_combine_kernel"}, ks
    assert ks.get("dense_combine_kernel", {"launches": 0})["launches"] == (1 if ctx.dense_info()["k_chunks"] > 1 else 0), ks
    mv = ctx.stats()["matvec"]
    assert mv["alg_bytes"] == 8.0 * n * n + 16.0 * n * m and mv["flops"] == 2.0 * n * n * m, mv
    assert mv["launches"] == sum(v["launches"] for v in ks.values())
    assert ctx.dense_info()["workspace_bytes"] == (8 * ctx.dense_info()["k_chunks"] * n * m if ctx.dense_info()["k_chunks"] > 1 else 0)


# ------------------------------------------------------------------ 4. the preconditioners
def test_the_preconditioners_give_the_bits_of_the_numpy_expressions(ctx):
    n, m, fac = 130, 5, -3.75
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    a[7, 7] = -fac + 2.0e-6                                   # |a_ii + fac| below the guard on one row
    b[9, 9] = 0.5
    a[9, 9] = -fac * b[9, 9] - 3.0e-6                         # ... and |a_ii + fac b_ii| on another
    setup_host(ctx, 0, a, n + 3)
    setup_device(ctx, 1, b, n)
    x = rng.standard_normal((n, m))
    den = np.diag(a) + fac
    assert (np.abs(den) <= 1e-5).sum() == 1
    want = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)
    assert np.array_equal(precondition(ctx, "dla_dense_precnd", fac, x), want)
    den = np.diag(a) + fac * np.diag(b)
    assert (np.abs(den) <= 1e-5).sum() == 1
    want = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)
    assert np.array_equal(precondition(ctx, "dla_dense_precnd_pencil", fac, x), want)
    pre = ctx.stats()["precnd"]["launches"]
    precondition(ctx, "dla_dense_precnd", fac, x)
    assert ctx.stats()["precnd"]["launches"] == pre + 1
    # booked: one launch each under the kernel's name, with the bytes and flops the sparse preconditioners book for theirs
    px, py = ctx.panel(x), ctx.panel(n, m)
    for name, kernel, nbytes, flops in (("dla_dense_precnd", "diag_precnd_kernel", 8.0 * n * (2.0 * m + 1.0), 1.0 * n * m),
                                        ("dla_dense_precnd_pencil", "pencil_precnd_kernel", 16.0 * n * m + 16.0 * n, 2.0 * n * m)):
        ctx.reset_stats()
        ctx._chk(ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, fac, px.ptr, py.ptr))
        ctx.sync()
        ks = {k: (v["launches"], v["alg_bytes"], v["flops"]) for k, v in ctx.kernel_stats().items() if v["launches"]}
        assert ks == {kernel: (1, nbytes, flops)}, ks
        pc = ctx.stats()["precnd"]
        assert (pc["launches"], pc["alg_bytes"], pc["flops"]) == (1, nbytes, flops), pc
    px.free(); py.free()


# ------------------------------------------------------------------ 5. independence and refusals
def test_sparse_and_dense_slots_keep_their_bits_while_the_others_change(ctx):
    n, m = 130, 13
    rng = np.random.default_rng(9)
    i = np.arange(n, dtype=np.float64)
    s = sp.diags([0.1 * np.cos(i[:-1]), 2.0 + i / 50.0, 0.1 * np.cos(i[:-1])], [-1, 0, 1]).tocsr()
    a, b, other = rng.standard_normal((n, n)), rng.standard_normal((n, n)), rng.standard_normal((63, 63))
    x = rng.standard_normal((n, m))
    ctx.spmm_setup(s)
    setup_host(ctx, 0, a, n)
    setup_host(ctx, 1, b, n)

    def sparse(v):
        return guarded(ctx, lambda xp, yp: ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_spmm_matvec"), n, m, xp, yp), v)
    ys, ya, yb = sparse(x), product(ctx, 0, x), product(ctx, 1, x)
    assert np.abs(ys - s @ x).max() < 1e-12 and not np.array_equal(ya, yb)
    sparse_info = ctx.spmm_info()
    # the metric is replaced by a matrix of another size and dropped: A and the sparse operator keep their bits
    setup_device(ctx, 1, other, 63)
    assert np.array_equal(product(ctx, 0, x), ya) and np.array_equal(sparse(x), ys) and ctx.dense_info()["n"] == n
    ctx.dense_drop(True)
    with pytest.raises(capi.DlaError, match="dla_dense_info"):
        ctx.dense_info(True)
    assert np.array_equal(product(ctx, 0, x), ya) and np.array_equal(sparse(x), ys)
    # ... and the other way round; the sparse operator is replaced in between
    setup_host(ctx, 1, b, n + 3)
    ctx.dense_drop(False)
    ctx.spmm_setup(s * 2.0)
    assert np.array_equal(product(ctx, 1, x), yb)
    setup_device(ctx, 0, a, n)
    ctx.spmm_setup(s)
    assert np.array_equal(product(ctx, 0, x), ya) and np.array_equal(product(ctx, 1, x), yb) and np.array_equal(sparse(x), ys)
    assert ctx.spmm_info() == sparse_info
    ctx.dense_drop(False)
    ctx.dense_drop(False)                                      # a no-op where nothing is stored


def test_refused_set_ups_replace_nothing_and_callbacks_name_themselves(ctx):
    n, m = 65, 3
    rng = np.random.default_rng(10)
    a, b = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    x = rng.standard_normal((n, m))
    px, py = ctx.panel(x), ctx.panel(np.full((n + 1, m), SENTINEL, order="F"))

    def refused(call, *words):
        st = call()
        assert st == capi.ERR_ARG, st
        assert all(w in last_error(ctx) for w in words), last_error(ctx)
        assert np.all(py.download() == SENTINEL), "a refused call wrote"

    mv = lambda name, rows=n: ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), rows, m, px.ptr, py.ptr)
    pc = lambda name, rows=n: ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), rows, m, -1.5, px.ptr, py.ptr)
    # nothing is stored (whatever context the thread's callbacks are bound to)
    refused(lambda: mv("dla_dense_matvec"), "dla_dense_matvec", "operator")
    refused(lambda: mv("dla_dense_bvec"), "dla_dense_bvec", "metric")
    refused(lambda: pc("dla_dense_precnd"), "dla_dense_precnd", "operator")
    refused(lambda: pc("dla_dense_precnd_pencil"), "dla_dense_precnd_pencil", "operator")
    assert ctx.lib.dla_dense_info(ctx.h, 0, C.byref(capi.DenseInfo())) == capi.ERR_ARG and "dla_dense_info" in last_error(ctx)
    setup_host(ctx, 0, a, n)
    refused(lambda: pc("dla_dense_precnd_pencil"), "dla_dense_precnd_pencil", "metric")
    refused(lambda: mv("dla_dense_bvec"), "dla_dense_bvec", "metric")
    setup_device(ctx, 1, b, n)
    ya, yb = product(ctx, 0, x), product(ctx, 1, x)
    # refused set-ups, host and device entry: lda < n, a null pointer, which = 2, n <= 0
    held = np.asfortranarray(rng.standard_normal((n, n)))
    dev = ctx.panel(held)
    for entry, ptr in (("dla_dense_setup", held.ctypes.data), ("dla_dense_setup_dev", dev.ptr)):
        f = getattr(ctx.lib, entry)
        for which in (0, 1):
            refused(lambda: f(ctx.h, which, n, ptr, n - 1), entry + ":", "lda")
            refused(lambda: f(ctx.h, which, n, None, n), entry + ":", "null")
            refused(lambda: f(ctx.h, which, 0, ptr, n), entry + ":", "n must be positive")
        refused(lambda: f(ctx.h, 2, n, ptr, n), entry + ":", "which")
    assert ctx.lib.dla_dense_info(ctx.h, 2, C.byref(capi.DenseInfo())) == capi.ERR_ARG
    assert ctx.lib.dla_dense_drop(ctx.h, 2) == capi.ERR_ARG
    assert np.array_equal(product(ctx, 0, x), ya) and np.array_equal(product(ctx, 1, x), yb)
    # another n
    for name in ("dla_dense_matvec", "dla_dense_bvec"):
        refused(lambda: mv(name, n + 1), name, str(n + 1), str(n))
    for name in ("dla_dense_precnd", "dla_dense_precnd_pencil"):
        refused(lambda: pc(name, n + 1), name, str(n + 1), str(n))
    # the pencil form with a metric of another n
    setup_host(ctx, 1, rng.standard_normal((63, 63)), 63)
    refused(lambda: pc("dla_dense_precnd_pencil"), "dla_dense_precnd_pencil", "63", str(n))


# ------------------------------------------------------------------ 6. whole solves on the reference harness' problem
GOLDEN = ["dav_n1000_unit", "dav_n2000_unit", "dav_n2000_rand", "dav_n600_rand_dav10", "lob_n1000_unit", "lob_n2000_unit",
          "lob_n2000_rand", "lob_n800_shift", "gdav_n600_unit", "glob_n600_unit"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_fixtures.npz"), allow_pickle=False)


def harness_matrix(n):
    """a_ii = i + 1, a_ij = 1 / (i + j), 1-based (main.f90:311-317)"""
    idx = np.arange(1, n + 1.0)
    a = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a, idx + 1.0)
    return np.asfortranarray(a)


def guess(kind, n, m, seed):
    if kind == "unit":
        g = np.zeros((n, m), order="F")
        g[np.arange(m), np.arange(m)] = 1.0
        return g
    return np.asfortranarray(np.random.default_rng(seed).random((n, m)) - 0.5)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_reference_problem_solved_in_device_mode_matches_the_golden_results(ctx, oracle, gold, name):
    """Eigenvalues against the unmodified reference's at rtol = 1e-9 (the figure of tests/test_spmm_gpu.py for a device operator
    against the oracle); iterations within max(1, it_ref // 10) (the product sums in another order than the reference's dgemm, so
    equality is not asked); run-ahead on and off agree to 1e-10 -- both runs converged to the spec's residual tolerance (at most
    1e-6 relative), and an eigenvalue's error is quadratic in its residual."""
    spec = next(s for s in json.loads(str(gold["driver_specs"])) if s["name"] == name)
    n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
    a = harness_matrix(n)
    ctx.dense_setup(a)
    b = None
    if spec.get("gen"):
        b = oracle.metric_setup(n)
        ctx.dense_setup(b, metric=True)
    mv, pc, bv = (capi.fn_address(f) for f in ("dla_dense_matvec", "dla_dense_precnd", "dla_dense_bvec"))
    eigs = []
    for run_ahead in (1, 0):
        ctx.set_option(capi.OPT_RUN_AHEAD, run_ahead)
        g = guess(spec["guess"], n, m, spec["seed"])
        if spec["solver"] == "gen_davidson":
            eig, vec, ok, info = ctx.gen_david_driver(n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], spec["shift"], mv, pc, bv, g)
        elif spec["solver"] == "lobpcg":
            eig, vec, ok, info = ctx.lobpcg_driver(n, t, m, spec["max_iter"], spec["tol"], spec["shift"], mv, pc, g, bvec=bv if b is not None else None)
        else:
            eig, vec, ok, info = ctx.davidson_driver(n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], spec["shift"], mv, pc, g)
        assert ok and bool(gold[name + "_ok"]), (name, run_ahead, info)
        assert np.allclose(eig[:t], gold[name + "_eig"][:t], rtol=1e-9, atol=0), (name, run_ahead, eig[:t], gold[name + "_eig"][:t])
        it_ref = int(gold[name + "_tr_iters"])
        assert abs(info["iters"] - it_ref) <= max(1, it_ref // 10), (name, run_ahead, info, it_ref)
        x = vec[:, :t]
        gram = x.T @ (b @ x) if b is not None else x.T @ x
        assert np.abs(gram - np.eye(t)).max() < 1e-10, (name, run_ahead)
        eigs.append(eig[:t].copy())
    assert np.allclose(eigs[0], eigs[1], rtol=1e-10, atol=0), (name, eigs)
