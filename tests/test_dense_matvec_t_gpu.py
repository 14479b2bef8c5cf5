"""GPU: y = A^T x from the stored copy of the dense operator (include/diaglib_amd.h, dla_dense_matvec_t): the kernel
dense_t_mfma_kernel, the combining kernel of a split pass, the contract's bound, exactness, repeatability, what the call leaves
alone, its refusals and its statistics.

Outputs sit between sentinel columns and inputs between NaN columns, as in tests/test_dense_operator_gpu.py: x has leading
dimension n, so the rows of the allocation beyond a column's n are its neighbours -- nothing outside the n x m result is written,
nothing outside the n x m input is read."""
import numpy as np
import pytest

from diaglib_amd import capi
from test_dense_operator_gpu import EPS, LD, SENTINEL, guarded, last_error, product, setup_device, setup_host
from test_dense_t_plan import rule

pytestmark = pytest.mark.gpu
SIZES = [1, 15, 16, 17, 63, 64, 65, 130, 257, 1024]
WIDTHS = [1, 8, 16, 17, 37, 48, 49]
T = "dla_dense_matvec_t"


@pytest.fixture(autouse=True)
def _device_callbacks_and_empty_slots(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield
    ctx.dense_drop(False)
    ctx.dense_drop(True)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def product_t(ctx, x):
    n, m = x.shape
    return guarded(ctx, lambda xp, yp: ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(T), n, m, xp, yp), x)


def ncu_of(ctx):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_REFS = {}


def case(n):
    """a non-symmetric standard-normal matrix, a block of 49 columns, their long-double A^T x and |A|^T |x|: once per n, read-only"""
    if n not in _REFS:
        rng = np.random.default_rng(6000 + n)
        a, x = rng.standard_normal((n, n)), rng.standard_normal((n, 49))
        al, xl = a.astype(LD), x.astype(LD)
        _REFS[n] = (a, x, al.T @ xl, np.abs(al).T @ np.abs(xl), al @ xl)
        for v in _REFS[n]:
            v.setflags(write=False)
    return _REFS[n]


def chunks_of(ctx, n, m):
    """row_chunks of dense_t_plan at this device's CU count, by the planner's rule as tests/test_dense_t_plan.py transcribes it
    (and holds against the planner itself on the CPU)"""
    return rule(ncu_of(ctx), n, m)[0]


def test_the_shapes_cover_a_split_and_an_unsplit_plan(ctx):
    """1024 x {1, 8} split, the small and the wide shapes do not"""
    assert chunks_of(ctx, 1024, 1) > 1 and chunks_of(ctx, 1024, 8) > 1
    assert chunks_of(ctx, 130, 8) == 1 and chunks_of(ctx, 1024, 48) == 1 and chunks_of(ctx, 17, 1) == 1


@pytest.mark.parametrize("n", SIZES)
def test_integer_products_are_exact(ctx, n):
    """entries in [-8, 8]: every order of summation is exact, so the result equals a.T @ x bit for bit; host and device set-up"""
    rng = np.random.default_rng(7000 + n)
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)
    for setup, lda in ((setup_host, n + 3), (setup_device, n)):
        setup(ctx, 0, a, lda)
        for m in WIDTHS:
            x = rng.integers(-8, 9, (n, m)).astype(np.float64)
            assert np.array_equal(product_t(ctx, x), a.T @ x), (n, m, setup.__name__)


@pytest.mark.parametrize("n", SIZES)
def test_random_products_stay_within_the_bound_repeat_and_agree_with_the_metric_slot(ctx, n):
    """|got - ref| <= (n + 2) eps (|A|^T |x|)_i element-wise against the long-double product; a second call returns the same bits;
    dla_dense_bvec on a metric slot that holds the explicitly transposed array stays within twice the bound of it (each within
    one bound of the exact product); the forward product of the non-symmetric matrix breaks the bound."""
    a, x, ref, mag, ref_forward = case(n)
    setup_host(ctx, 0, a, n)
    setup_host(ctx, 1, np.ascontiguousarray(a.T), n)
    for m in WIDTHS:
        xm = np.array(x[:, :m])
        got = product_t(ctx, xm)
        bound = (n + 2) * LD(EPS) * mag[:, :m]
        err = np.abs(got.astype(LD) - ref[:, :m])
        print(f"n={n} m={m}: max err / bound = {float((err / bound).max()):.3e}")
        assert np.all(err <= bound), (n, m)
        assert np.array_equal(product_t(ctx, xm), got), (n, m)
        other = product(ctx, 1, xm)
        assert np.all(np.abs(got.astype(LD) - other.astype(LD)) <= 2 * bound), (n, m)
        if n > 1:
            assert not np.all(np.abs(ref_forward[:, :m] - ref[:, :m]) <= bound), "the forward product must fail the bound"


def test_the_call_leaves_the_slot_as_it_was(ctx):
    n = 257
    a, x, _, _, _ = case(n)
    setup_host(ctx, 0, a, n)
    forward = product(ctx, 0, np.array(x[:, :13]))
    info = ctx.dense_info()
    for m in (1, 37, 49):
        product_t(ctx, np.array(x[:, :m]))
        assert ctx.dense_info() == info
    assert np.array_equal(product(ctx, 0, np.array(x[:, :13])), forward)
    assert info["device_bytes"] == 8 * info["n_pad"] ** 2 + 8 * n
    # the convenience of the Python layer
    px, py = ctx.panel(np.array(x[:, :5])), ctx.panel(n, 5)
    ctx.dense_matvec_t(px, py)
    assert np.array_equal(py.download(), product_t(ctx, np.array(x[:, :5])))
    px.free(); py.free()


def test_refusals_name_the_entry_and_write_nothing(ctx):
    n, m = 65, 3
    a, x, _, _, _ = case(n)
    px, py = ctx.panel(np.array(x[:, :m])), ctx.panel(np.full((n + 1, m), SENTINEL, order="F"))

    def refused(rows, *words):
        st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(T), rows, m, px.ptr, py.ptr)
        assert st == capi.ERR_ARG, st
        assert all(w in last_error(ctx) for w in words), last_error(ctx)
        assert np.all(py.download() == SENTINEL), "a refused call wrote"

    refused(n, T, "operator")                                   # nothing stored
    setup_host(ctx, 1, a, n)
    refused(n, T, "operator")                                   # a metric is not the operator
    setup_host(ctx, 0, a, n)
    refused(n + 1, T, str(n + 1), str(n))                       # another n
    assert np.array_equal(product_t(ctx, np.array(x[:, :m])), product_t(ctx, np.array(x[:, :m])))
    ctx.dense_drop(False)
    refused(n, T, "operator")
    px.free(); py.free()


@pytest.mark.parametrize("n,m", [(1024, 1), (1024, 8), (257, 37), (130, 49), (1024, 48)])
def test_statistics_one_launch_per_pass_under_the_kernels_name(ctx, n, m):
    a, x, _, _, _ = case(n)
    setup_host(ctx, 0, a, n)
    px, py = ctx.panel(np.array(x[:, :m])), ctx.panel(n, m)
    ctx.reset_stats()
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(T), n, m, px.ptr, py.ptr))
    ctx.sync()
    ks = {k: v for k, v in ctx.kernel_stats().items() if v["launches"]}
    passes = [min(48, m - c0) for c0 in range(0, m, 48)]
    want = {}
    for w in passes:
        e = want.setdefault(f"dense_t_mfma_kernel<{-(-w // 16)}>", [0, 0.0, 0.0])
        e[0] += 1; e[1] += 8.0 * n * n + 16.0 * n * w; e[2] += 2.0 * n * n * w
    combines = sum(1 for w in passes if chunks_of(ctx, n, w) > 1)
    got = {k: [v["launches"], v["alg_bytes"], v["flops"]] for k, v in ks.items() if k != "dense_combine_kernel"}
    assert got == want, (got, want)
    assert ks.get("dense_combine_kernel", {"launches": 0})["launches"] == combines
    mv = ctx.stats()["matvec"]
    assert mv["alg_bytes"] == 8.0 * n * n * len(passes) + 16.0 * n * m and mv["flops"] == 2.0 * n * n * m
    assert mv["launches"] == len(passes) + combines
    px.free(); py.free()
