"""GPU: a symmetric dense operator or metric stored as one triangle (include/diaglib_amd.h, dla_dense_setup_sym): the pack
kernel, dense_sym_mfma_kernel and dense_sym_combine_kernel against NumPy and a long-double reference, the triangle that must not
be read, what the slot remembers, its info, statistics, replacement and refusals, and whole solves of the reference harness'
problem with operator and metric stored symmetrically.

Outputs sit between sentinel columns and inputs between NaN columns, as in tests/test_dense_matvec_t_gpu.py: nothing outside the
n x m result is written, nothing outside the n x m input is read."""
import ctypes as C
import json

import numpy as np
import pytest

from diaglib_amd import capi
from test_dense_matvec_t_gpu import ncu_of, product_t
from test_dense_operator_gpu import (EPS, GOLDEN, LD, SENTINEL, gold, guess, harness_matrix, last_error, precondition,  # noqa: F401
                                     product, setup_device, setup_host)
from test_dense_sym_layout import planner_rule

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 63, 64, 65, 130, 255, 256, 257, 513, 1024]
WIDTHS = [1, 8, 16, 17, 37, 48, 49]
ENTRY = {False: "dla_dense_setup_sym", True: "dla_dense_setup_sym_dev"}


@pytest.fixture(autouse=True)
def _device_callbacks_and_empty_slots(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield
    ctx.dense_drop(False)
    ctx.dense_drop(True)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def held_triangle(a, lda, uplo, poison):
    """a in the leading n rows of an lda x n column-major array, rows n .. lda - 1 NaN; poison: the strict triangle that uplo does
    not reference is NaN as well"""
    n = a.shape[0]
    held = np.full((lda, n), np.nan, order="F")
    held[:n, :] = a
    if poison:
        held[:n, :][np.triu_indices(n, 1) if uplo == "L" else np.tril_indices(n, -1)] = np.nan
    return held


def setup_sym(ctx, which, a, lda, uplo, dev=False, poison=True):
    """dla_dense_setup_sym / _dev of triangle uplo of a; a device array is overwritten and freed before anything is multiplied"""
    n = a.shape[0]
    held = held_triangle(a, lda, uplo, poison)
    if not dev:
        ctx._chk(ctx.lib.dla_dense_setup_sym(ctx.h, which, n, held.ctypes.data, lda, uplo.encode()))
        return
    p = ctx.panel(held)
    ctx._chk(ctx.lib.dla_dense_setup_sym_dev(ctx.h, which, n, p.ptr, lda, uplo.encode()))
    p.zero()
    ctx.sync()
    p.free()


def symmetric_integers(rng, n):
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)
    return np.tril(a) + np.tril(a, -1).T


def test_the_shapes_cover_one_item_per_panel_and_several_chunks_in_a_panel(ctx):
    """from the planner's rule at this device's CU count, as tests/test_dense_sym_layout.py transcribes it (and holds against the
    planner itself on the CPU)"""
    ncu = ncu_of(ctx)
    plans = {(n, m): planner_rule(ncu, n, min(m, 48)) for n in SIZES for m in WIDTHS}
    assert any(p["panels"] > 1 and p["max_chunks"] == 1 for p in plans.values()), "no shape with one item per panel of several"
    assert any(p["max_chunks"] > 1 for p in plans.values()), "no shape with several chunks in a panel"
    assert planner_rule(ncu, 1024, 8)["max_chunks"] > 1 and planner_rule(ncu, 1024, 48)["max_chunks"] == 1
    assert planner_rule(ncu, 255, 8)["items"] == 1 and planner_rule(ncu, 257, 8)["panels"] == 2


# ------------------------------------------------------------------ 1. the exact product
@pytest.mark.parametrize("n", SIZES)
def test_integer_products_are_exact_in_both_slots_from_either_triangle_host_and_device(ctx, n):
    """entries in [-8, 8]: every order of summation is exact, so the result equals a @ x bit for bit"""
    rng = np.random.default_rng(8000 + n)
    a = symmetric_integers(rng, n)
    xs = {m: rng.integers(-8, 9, (n, m)).astype(np.float64) for m in WIDTHS}
    nt = -(-n // 16)
    for which, dev, uplo in ((0, False, "L"), (1, True, "U"), (0, True, "L"), (1, False, "U"), (0, False, "U"), (1, True, "L")):
        setup_sym(ctx, which, a, n + 3, uplo, dev)
        info = ctx.dense_info(bool(which))
        assert info["n"] == n and info["n_pad"] == nt * 16 and info["device_bytes"] == 8 * 128 * nt * (nt + 1) + 8 * n, info
        assert ctx.dense_sym_info(bool(which))["uplo"] == uplo
        for m in WIDTHS:
            got = product(ctx, which, xs[m])
            assert np.array_equal(got, a @ xs[m]), (n, m, which, dev, uplo)


@pytest.mark.parametrize("n", SIZES)
def test_the_unreferenced_triangle_is_never_read(ctx, n):
    """host and device set-up from an array whose unreferenced strict triangle is NaN: a NaN-free product with the bits of the
    product from the clean array"""
    rng = np.random.default_rng(8100 + n)
    a = rng.standard_normal((n, n))
    a = np.tril(a) + np.tril(a, -1).T
    x = rng.standard_normal((n, 13))
    for uplo in ("L", "U"):
        setup_sym(ctx, 0, a, n + 3, uplo, dev=False, poison=False)
        clean = product(ctx, 0, x)
        assert not np.isnan(clean).any()
        for dev in (False, True):
            setup_sym(ctx, 1, a, n + 3, uplo, dev, poison=True)
            assert np.array_equal(product(ctx, 1, x), clean), (n, uplo, dev)


# ------------------------------------------------------------------ 2. the bound, repeats, the two set-ups, the two triangles
_REFS = {}


def case(n):
    """an exactly symmetric standard-normal matrix, a block of 49 columns, their long-double product and |A| |x|: once per n, read-only"""
    if n not in _REFS:
        rng = np.random.default_rng(8200 + n)
        a, x = rng.standard_normal((n, n)), rng.standard_normal((n, 49))
        a = np.tril(a) + np.tril(a, -1).T
        al, xl = a.astype(LD), x.astype(LD)
        _REFS[n] = (a, x, al @ xl, np.abs(al) @ np.abs(xl))
        for v in _REFS[n]:
            v.setflags(write=False)
    return _REFS[n]


@pytest.mark.parametrize("n", SIZES)
def test_random_symmetric_products_stay_within_the_bound_and_repeat_bit_for_bit(ctx, n):
    """|got - ref| <= (n + 2) eps (|A| |x|)_i element-wise against the long-double product (the contract's bound: it holds for any
    order of summation); a second call, a device set-up and the other triangle return the same bits"""
    a, x, ref, mag = case(n)
    setup_sym(ctx, 0, a, n, "L", dev=False)
    setup_sym(ctx, 1, a, n + 3, "L", dev=True)
    first = {}
    for m in WIDTHS:
        xm = np.array(x[:, :m])
        got = first[m] = product(ctx, 0, xm)
        bound = (n + 2) * LD(EPS) * mag[:, :m]
        err = np.abs(got.astype(LD) - ref[:, :m])
        print(f"n={n} m={m}: max err / bound = {float((err / bound).max()):.3e}")
        assert np.all(err <= bound), (n, m)
        assert np.array_equal(product(ctx, 0, xm), got), (n, m)
        assert np.array_equal(product(ctx, 1, xm), got), (n, m, "device set-up")
    setup_sym(ctx, 1, a, n, "U", dev=False)
    for m in WIDTHS:
        assert np.array_equal(product(ctx, 1, np.array(x[:, :m])), first[m]), (n, m, "upper triangle")


@pytest.mark.parametrize("n", [17, 257, 1024])
def test_the_transposed_product_of_a_symmetric_slot_is_the_symmetric_product(ctx, n):
    a, x, _, _ = case(n)
    setup_sym(ctx, 0, a, n, "U")
    info = ctx.dense_info()
    for m in (1, 13, 49):
        xm = np.array(x[:, :m])
        assert np.array_equal(product_t(ctx, xm), product(ctx, 0, xm)), (n, m)
    assert ctx.dense_info()["n"] == info["n"] and ctx.dense_info()["device_bytes"] == info["device_bytes"]


def test_the_preconditioners_return_the_bits_they_return_on_full_copies(ctx):
    n, fac = 130, -3.75
    a, x, _, _ = case(n)
    b = np.array(case(65)[0])
    b = np.pad(b, ((0, 65), (0, 65))) + np.diag(np.linspace(2.0, 3.0, n))
    xm = np.array(x[:, :5])
    setup_host(ctx, 0, a, n)
    setup_host(ctx, 1, b, n)
    want = [precondition(ctx, name, fac, xm) for name in ("dla_dense_precnd", "dla_dense_precnd_pencil")]
    setup_sym(ctx, 0, a, n + 3, "L", dev=True)
    setup_sym(ctx, 1, b, n, "U")
    got = [precondition(ctx, name, fac, xm) for name in ("dla_dense_precnd", "dla_dense_precnd_pencil")]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    den = np.diag(a) + fac * np.diag(b)
    assert np.array_equal(got[1], np.where(np.abs(den)[:, None] > 1e-5, xm / den[:, None], xm))


# ------------------------------------------------------------------ 3. info and statistics
@pytest.mark.parametrize("n,m", [(1024, 1), (1024, 8), (257, 37), (130, 49), (1024, 48), (16, 8), (513, 100)])
def test_info_and_one_launch_per_pass_under_the_kernels_name(ctx, n, m):
    a, _, _, _ = case(n)
    x = np.random.default_rng(3).standard_normal((n, m))
    full = np.array(case(65)[0])
    setup_host(ctx, 1, full, 65)
    neighbour = ctx.dense_info(True)
    setup_sym(ctx, 0, a, n, "L")
    px, py = ctx.panel(x), ctx.panel(n, m)
    ctx.reset_stats()
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_dense_matvec"), n, m, px.ptr, py.ptr))
    ctx.sync()
    ks = {k: v for k, v in ctx.kernel_stats().items() if v["launches"]}
    passes = [min(48, m - c0) for c0 in range(0, m, 48)]
    want = {}
    for w in passes:
        e = want.setdefault(f"dense_sym_mfma_kernel<{-(-w // 16)}>", [0, 0.0, 0.0])
        e[0] += 1; e[1] += 4.0 * n * (n + 1) + 16.0 * n * w; e[2] += 2.0 * n * n * w
    combines = len(passes) if n > 16 else 0
    got = {k: [v["launches"], v["alg_bytes"], v["flops"]] for k, v in ks.items() if k != "dense_sym_combine_kernel"}
    assert got == want, (got, want)
    combine = ks.get("dense_sym_combine_kernel", {"launches": 0, "alg_bytes": 0.0})
    assert combine["launches"] == combines and combine["alg_bytes"] == 0.0
    mv = ctx.stats()["matvec"]
    assert mv["alg_bytes"] == 4.0 * n * (n + 1) * len(passes) + 16.0 * n * m and mv["flops"] == 2.0 * n * n * m
    assert mv["launches"] == len(passes) + combines
    # what the two infos answer: the first pass of this product, by the planner's rule
    nt = -(-n // 16)
    rule = planner_rule(ncu_of(ctx), n, passes[0])
    info, sym = ctx.dense_info(), ctx.dense_sym_info()
    assert info == {"n": n, "n_pad": 16 * nt, "row_tile": 64, "k_chunks": rule["max_chunks"], "device_bytes": 8 * 128 * nt * (nt + 1) + 8 * n,
                    "workspace_bytes": 8 * rule["ws_doubles"]}, info
    assert sym == {"uplo": "L", "panels": rule["panels"], "chunk_blocks": rule["chunk_blocks"], "max_partials": rule["max_partials"]}, sym
    assert ctx.dense_info(True) == neighbour, "the full neighbour's info changed"
    assert np.abs(py.download() - a @ x).max() <= 1e-10 * max(1.0, np.abs(a @ x).max())
    px.free(); py.free()


# ------------------------------------------------------------------ 4. replacement and refusals
def test_full_then_symmetric_then_full_each_product_right(ctx):
    n = 257
    rng = np.random.default_rng(11)
    sym = symmetric_integers(rng, n)
    full = rng.integers(-8, 9, (n, n)).astype(np.float64)          # not symmetric
    x = rng.integers(-8, 9, (n, 17)).astype(np.float64)
    for which in (0, 1):
        setup_host(ctx, which, full, n)
        assert np.array_equal(product(ctx, which, x), full @ x)
        with pytest.raises(capi.DlaError, match="dla_dense_sym_info"):
            ctx.dense_sym_info(bool(which))
        ctx.dense_setup(sym, metric=bool(which), sym="U")
        assert np.array_equal(product(ctx, which, x), sym @ x)
        assert ctx.dense_info(bool(which))["device_bytes"] == 8 * 128 * 17 * 18 + 8 * n
        setup_device(ctx, which, full, n + 3)
        assert np.array_equal(product(ctx, which, x), full @ x)
        assert ctx.dense_info(bool(which))["device_bytes"] == 8 * 272 * 272 + 8 * n
        if which == 0:
            assert np.array_equal(product_t(ctx, x), full.T @ x)
    with pytest.raises(ValueError, match="dense_setup"):
        ctx.dense_setup(sym, sym="X")


def test_refused_set_ups_replace_nothing_and_the_info_refuses_full_and_empty_slots(ctx):
    n, m = 65, 3
    a, x, _, _ = case(n)
    xm = np.array(x[:, :m])
    out = capi.DenseSymInfo()
    for which in (0, 1):
        assert ctx.lib.dla_dense_sym_info(ctx.h, which, C.byref(out)) == capi.ERR_ARG and "dla_dense_sym_info" in last_error(ctx)   # empty
    assert ctx.lib.dla_dense_sym_info(ctx.h, 2, C.byref(out)) == capi.ERR_ARG and "which" in last_error(ctx)
    setup_sym(ctx, 0, a, n, "L")
    setup_host(ctx, 1, a, n)
    assert ctx.lib.dla_dense_sym_info(ctx.h, 1, C.byref(out)) == capi.ERR_ARG and "dla_dense_sym_info" in last_error(ctx)           # full
    assert ctx.lib.dla_dense_sym_info(ctx.h, 0, None) == capi.ERR_ARG and "null" in last_error(ctx)
    ya, yb = product(ctx, 0, xm), product(ctx, 1, xm)
    infos = ctx.dense_info(), ctx.dense_info(True), ctx.dense_sym_info()
    held = np.asfortranarray(np.random.default_rng(12).standard_normal((n, n)))
    dev = ctx.panel(held)

    def refused(call, *words):
        st = call()
        assert st == capi.ERR_ARG, st
        assert all(w in last_error(ctx) for w in words), last_error(ctx)

    for is_dev, ptr in ((False, held.ctypes.data), (True, dev.ptr)):
        f, entry = getattr(ctx.lib, ENTRY[is_dev]), ENTRY[is_dev]
        for which in (0, 1):
            for bad in (b"X", b"0", b" "):
                refused(lambda: f(ctx.h, which, n, ptr, n, bad), entry + ":", "uplo")
            refused(lambda: f(ctx.h, which, n, None, n, b"L"), entry + ":", "null")
            refused(lambda: f(ctx.h, which, n, ptr, n - 1, b"U"), entry + ":", "lda")
            refused(lambda: f(ctx.h, which, 0, ptr, n, b"L"), entry + ":", "n must be positive")
        refused(lambda: f(ctx.h, 2, n, ptr, n, b"L"), entry + ":", "which")
    assert np.array_equal(product(ctx, 0, xm), ya) and np.array_equal(product(ctx, 1, xm), yb)
    assert (ctx.dense_info(), ctx.dense_info(True), ctx.dense_sym_info()) == infos
    # lower-case letters are accepted
    af = np.asfortranarray(a)
    ctx._chk(ctx.lib.dla_dense_setup_sym(ctx.h, 1, n, af.ctypes.data, n, b"u"))
    assert ctx.dense_sym_info(True)["uplo"] == "U" and np.array_equal(product(ctx, 1, xm), ya)
    dev.free()


# ------------------------------------------------------------------ 5. whole solves on the reference harness' problem
@pytest.mark.parametrize("name", GOLDEN)
def test_the_reference_problem_solved_with_symmetric_storage_matches_the_golden_results(ctx, oracle, gold, name):  # noqa: F811
    """the cases of tests/test_dense_operator_gpu.py with operator ('L') and metric ('U') stored as triangles: eigenvalues against
    the unmodified reference's at that test's rtol = 1e-9"""
    spec = next(s for s in json.loads(str(gold["driver_specs"])) if s["name"] == name)
    n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
    ctx.dense_setup(harness_matrix(n), sym="L")
    b = None
    if spec.get("gen"):
        b = oracle.metric_setup(n)
        ctx.dense_setup(b, metric=True, sym="U")
    mv, pc, bv = (capi.fn_address(f) for f in ("dla_dense_matvec", "dla_dense_precnd", "dla_dense_bvec"))
    g = guess(spec["guess"], n, m, spec["seed"])
    if spec["solver"] == "gen_davidson":
        eig, vec, ok, info = ctx.gen_david_driver(n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], spec["shift"], mv, pc, bv, g)
    elif spec["solver"] == "lobpcg":
        eig, vec, ok, info = ctx.lobpcg_driver(n, t, m, spec["max_iter"], spec["tol"], spec["shift"], mv, pc, g, bvec=bv if b is not None else None)
    else:
        eig, vec, ok, info = ctx.davidson_driver(n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], spec["shift"], mv, pc, g)
    assert ok and bool(gold[name + "_ok"]), (name, info)
    assert np.allclose(eig[:t], gold[name + "_eig"][:t], rtol=1e-9, atol=0), (name, eig[:t], gold[name + "_eig"][:t])
    assert ctx.dense_sym_info()["uplo"] == "L"
