"""GPU: y = A^T x from the one stored copy of the sparse operator (include/diaglib_amd.h, dla_spmm_transpose_prepare and
dla_spmm_matvec_t): the kernels ell_spmm_t_kernel<W>, sell_spmm_t_kernel<8>, csr_long_segments_t_kernel<4> with
long_rows_combine_kernel, and the index they walk, which the device builds from A's stored blocks.

References: A^T x and |A|^T |x| in long double straight from the triplets (bound (len_j + 2) eps |A|^T |x|, len_j the column's
length), and -- for the order contract -- dla_spmm_bvec on a metric slot that holds the stably transposed CSR arrays in the index's
format, whose bits the transposed product must return.  Outputs sit between sentinel columns, inputs between columns of NaN,
and come back unchanged.  Shapes: n around one slice of 64 and one block of 256, m around SELL_MC = 8 and LONG_MC = 4, every
pairing of A's storage (ELLPACK, sliced, sliced with a tail) with the index's."""
import ctypes as C

import numpy as np
import pytest

from diaglib_amd import capi
from spmm_cases import LONG_ROW, SLICE, WINDOW, csr_from_lengths
from spmm_slots import fresh_context, info, last_error, product, precnd, refresh, refresh_status, same_bits, setup, setup_status
from test_operators_gpu import EPS, LD, Guarded, assert_within, call_matvec, csr_rows, ragged_csr, setup_csr_one_shard

pytestmark = pytest.mark.gpu
T = "dla_spmm_matvec_t"
SEG = 4096
WIDTHS = (1, 4, 5, 8, 9, 13)


@pytest.fixture(scope="module")
def c():
    """a context of its own: the thread's sparse callbacks act on it from its first set-up of A"""
    with fresh_context() as ctx:
        yield ctx


def product_t(ctx, x):
    """dla_spmm_matvec_t on x: the output between sentinel columns, the input between columns of NaN -- a gather that leaves the n x m
    block of x poisons the result -- and unchanged afterwards"""
    n, m = x.shape
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    gx.host[:, 0] = gx.host[:, -1] = np.nan
    gx.whole.upload(gx.host)
    call_matvec(ctx, T, n, m, gx.ptr, gy.ptr)
    got = gy.body().copy()
    assert np.array_equal(gx.whole.download(), gx.host, equal_nan=True), "the input block (or its guard columns) was modified"
    gx.free(); gy.free()
    return got


# ------------------------------------------------------------------------------------------------------------------ matrices
def banded_csr(rng, n, eighths=False):
    """non-symmetric band |i - j| in {0, 1, 2, 17}, columns ascending: the pattern of examples/fortran_sparse_nonsym_caller"""
    rows, cols = [], []
    for i in range(n):
        js = sorted({j for j in (i - 17, i - 2, i - 1, i, i + 1, i + 2, i + 17) if 0 <= j < n})
        rows += [i] * len(js); cols += js
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    data = rng.integers(-40, 41, len(cols)) / 8.0 if eighths else rng.standard_normal(len(cols))
    return indptr, np.array(cols, np.int32), np.ascontiguousarray(data, dtype=np.float64)


def dense_column_csr(rng, n, dense_row=False):
    """rows of 1 .. 4 entries that all hold column 3: more than SEG entries in one column at n = 5000 (two segments of the index's
    tail) under rows that fit ELLPACK; dense_row: row n // 3 holds every column once as well, shuffled (A's own tail)"""
    lens = rng.integers(1, 5, n)
    if dense_row:
        lens[n // 3] = n
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    indices[indptr[:-1] + (rng.random(n) * np.minimum(lens, 4)).astype(np.int64)] = 3
    if dense_row:
        indices[indptr[n // 3]:indptr[n // 3 + 1]] = rng.permutation(n).astype(np.int32)
    return indptr, indices, data


def dense_row_csr(rng, n):
    lens = rng.integers(0, 4, n)
    lens[n // 3] = n
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    indices[indptr[n // 3]:indptr[n // 3 + 1]] = rng.permutation(n).astype(np.int32)
    return indptr, indices, data


def matrix(kind, n, seed=0):
    rng = np.random.default_rng(97 * n + seed)
    if kind == "ragged":
        return ragged_csr(rng, n, min(n, 9))
    if kind == "banded":
        return banded_csr(rng, n)
    return {"dense_column": dense_column_csr, "dense_row": dense_row_csr,
            "cross": lambda r, k: dense_column_csr(r, k, dense_row=True)}[kind](rng, n)


def stable_transpose(n, indptr, indices, data):
    """the CSR arrays of A^T with the entries of every column in the order of the caller's arrays"""
    order = np.argsort(indices, kind="stable")
    tptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n), out=tptr[1:])
    return tptr, np.ascontiguousarray(csr_rows(indptr)[order], dtype=np.int32), np.ascontiguousarray(data[order])


def transposed_reference(indptr, indices, data, x):
    rows = csr_rows(indptr)
    ref, mag = np.zeros(x.shape, LD), np.zeros(x.shape, LD)
    np.add.at(ref, indices, data.astype(LD)[:, None] * x.astype(LD)[rows])
    np.add.at(mag, indices, np.abs(data).astype(LD)[:, None] * np.abs(x).astype(LD)[rows])
    return ref, mag


def bound(n, indices, mag):
    return {"(len_j + 2) eps |A|^T|x|": (np.bincount(indices, minlength=n)[:, None] + 2) * EPS * mag, "tiny": LD(1e-300)}


def layout_of(lens):
    """what dla::sell_layout makes of these row lengths, in the fields of dla_spmm_info (the rules of include/diaglib_amd.h)"""
    n = len(lens)
    tail = lens > LONG_ROW
    asked = np.where(tail, 0, lens)
    stored = 0
    for w0 in range(0, n, WINDOW):
        a = np.sort(asked[w0:w0 + WINDOW])[::-1]
        stored += sum(int(a[s:s + SLICE].max()) for s in range(0, len(a), SLICE)) * SLICE
    segs = [-(-int(v) // SEG) for v in lens[tail]]
    return dict(stored=stored, slices=-(-n // SLICE), long_rows=int(tail.sum()), long_entries=int(lens[tail].sum()),
                long_segments=sum(segs), multi_segments=sum(s for s in segs if s > 1), multi_rows=sum(1 for s in segs if s > 1))


# ------------------------------------------------------------------------------------------------------------------ products
SMALL = [(kind, n, fa, ft) for kind in ("ragged", "banded") for n in (1, 63, 64, 65, 257, 1000) for fa in ("ell", "sell") for ft in ("ell", "sell")]
# n = 5000: a column of two segments under ELLPACK rows; a dense row, whose values the index finds in A's tail; both at once
LARGE = [("dense_column", 5000, "ell", "sell"), ("dense_column", 5000, "sell", "sell"), ("dense_row", 5000, "sell", "ell"),
         ("dense_row", 5000, "sell", "sell"), ("cross", 5000, "sell", "sell")]


@pytest.mark.parametrize("kind,n,fa,ft", SMALL + LARGE)
def test_random_data_bound_order_contract_repeats_and_both_setups(c, kind, n, fa, ft):
    indptr, indices, data = matrix(kind, n)
    setup(c, "A", n, indptr, indices, data, fa)
    c.spmm_transpose_prepare(ft)
    ti = c.spmm_transpose_info()
    assert ti["format"] == ft and ti["nnz"] == len(indices) and info(c, "A")["format"] == fa
    if kind in ("dense_column", "cross"):
        assert ti["long_segments"] == 2 and ti["multi_segments"] == 2
    if kind in ("dense_row", "cross"):
        assert info(c, "A")["long_rows"] == 1
    setup(c, "B", n, *stable_transpose(n, indptr, indices, data), ft)
    rng = np.random.default_rng(n)
    got = {}
    for m in WIDTHS:
        x = np.asfortranarray(rng.standard_normal((n, m)))
        y = got[m] = product_t(c, x)
        ref, mag = transposed_reference(indptr, indices, data, x)
        assert_within(y, ref, bound(n, indices, mag), f"{kind} n={n} {fa}/{ft} m={m}")
        assert same_bits(y, product_t(c, x)), "a repeated product differs"
        assert same_bits(y, product(c, "B", x)), "not the bits of dla_spmm_bvec on the stably transposed arrays"
        if m == 5 and n > 1:
            # the test can see a wrong kernel: the forward product of this non-symmetric matrix misses the bound
            fwd = product(c, "A", x)
            assert np.any(np.abs(fwd.astype(LD) - ref) > sum(bound(n, indices, mag).values()))
    # the same bits from a device set-up of A
    setup(c, "A", n, indptr, indices, data, fa, "device")
    with pytest.raises(RuntimeError):
        c.spmm_transpose_info()                     # (an accepted set-up has dropped the index)
    c.spmm_transpose_prepare(ft)
    rng = np.random.default_rng(n)
    for m in WIDTHS:
        assert same_bits(got[m], product_t(c, np.asfortranarray(rng.standard_normal((n, m))))), "host and device set-ups of A differ"


@pytest.mark.parametrize("kind,n,fa,ft", [s for s in SMALL if s[1] in (65, 1000)] + LARGE)
def test_integer_data_is_exact(c, kind, n, fa, ft):
    indptr, indices, _ = matrix(kind, n)
    rng = np.random.default_rng(5)
    data = rng.integers(-8, 9, len(indices)).astype(np.float64)
    setup(c, "A", n, indptr, indices, data, fa)
    c.spmm_transpose_prepare(ft)
    for m in (4, 9):
        x = np.asfortranarray(rng.integers(-8, 9, (n, m)).astype(np.float64))
        want = np.zeros((n, m))
        np.add.at(want, indices, data[:, None] * x[csr_rows(indptr)])
        assert np.array_equal(product_t(c, x), want)


def test_an_empty_column_gives_plus_zero(c):
    n = 130
    indptr, indices, data = matrix("ragged", n)
    indices = np.where(indices == 77, 78, indices).astype(np.int32)
    for fa, ft in (("ell", "ell"), ("sell", "sell")):
        setup(c, "A", n, indptr, indices, data, fa)
        c.spmm_transpose_prepare(ft)
        y = product_t(c, np.asfortranarray(np.random.default_rng(1).standard_normal((n, 5))))
        assert np.all(y[77] == 0.0) and not np.any(np.signbit(y[77]))


# ------------------------------------------------------------------------------------------------------------------ info
# (an ELLPACK index of a dense column at n = 5000 would be 25e6 entries: ELLPACK is asked for at the small shapes)
@pytest.mark.parametrize("kind,n,ft", [(k, n, ft) for k, n in (("ragged", 257), ("banded", 1000)) for ft in ("ell", "sell", "auto")] +
                         [(k, 5000, ft) for k in ("dense_column", "cross") for ft in ("sell", "auto")])
def test_info_field_by_field(c, kind, n, ft):
    indptr, indices, data = matrix(kind, n)
    setup(c, "A", n, indptr, indices, data, "auto")
    c.spmm_transpose_prepare(ft)
    got = c.spmm_transpose_info()
    lens = np.bincount(indices, minlength=n)
    nnz = len(indices)
    fmt = ft if ft != "auto" else ("ell" if int(lens.max()) * n <= 1.25 * nnz else "sell")
    if fmt == "ell":
        want = dict(format="ell", n=n, nnz=nnz, stored=int(lens.max()) * n, device_bytes=8 * int(lens.max()) * n, slice_rows=0, sort_window=0,
                    long_row_threshold=0, slices=0, long_rows=0, long_entries=0, long_segment_entries=0, long_segments=0, multi_segments=0)
    else:
        lay = layout_of(lens)
        multi_rows = lay.pop("multi_rows")
        want = dict(lay, format="sell", n=n, nnz=nnz, slice_rows=SLICE, sort_window=WINDOW, long_row_threshold=LONG_ROW, long_segment_entries=SEG)
        want["device_bytes"] = (8 * (lay["stored"] + lay["long_entries"]) + 4 * n + 8 * (lay["slices"] + 1) + 4 * lay["long_rows"] +
                                16 * lay["long_segments"] + 8 + 8 * multi_rows + 4)
    assert got == want


# ------------------------------------------------------------------------------------------------------------------ neighbours
def test_prepare_and_products_leave_the_operator_alone(c):
    n = 257
    indptr, indices, data = matrix("ragged", n)
    x = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 5)))
    for fa in ("ell", "sell"):
        setup(c, "A", n, indptr, indices, data, fa)
        before = (info(c, "A"), product(c, "A", x), precnd(c, "dla_spmm_precnd", x))
        for ft in ("ell", "sell"):
            c.spmm_transpose_prepare(ft)
            product_t(c, x)
            after = (info(c, "A"), product(c, "A", x), precnd(c, "dla_spmm_precnd", x))
            assert before[0] == after[0] and same_bits(before[1], after[1]) and same_bits(before[2], after[2])


@pytest.mark.parametrize("kind,n,fa,ft", [("ragged", 257, "ell", "sell"), ("banded", 1000, "sell", "ell"), ("cross", 5000, "sell", "sell")])
def test_a_refresh_of_the_values_is_a_refresh_of_the_transpose(c, kind, n, fa, ft):
    indptr, indices, data = matrix(kind, n)
    new = np.random.default_rng(3).standard_normal(len(data))
    x = np.asfortranarray(np.random.default_rng(4).standard_normal((n, 9)))
    setup(c, "A", n, indptr, indices, new, fa)
    c.spmm_transpose_prepare(ft)
    fresh = product_t(c, x)
    setup(c, "A", n, indptr, indices, data, fa)
    c.spmm_transpose_prepare(ft)
    old = product_t(c, x)
    assert not same_bits(old, fresh)
    # a refused refresh (another pattern) changes nothing
    other = indices.copy()
    other[0] = (other[0] + 1) % n
    assert refresh_status(c, "A", n, indptr, other, new) == capi.ERR_ARG
    assert same_bits(product_t(c, x), old)
    refresh(c, "A", n, indptr, indices, new)
    assert same_bits(product_t(c, x), fresh), "the product after a refresh is not that of a fresh set-up and prepare"


def test_lifecycle(c):
    n = 257
    indptr, indices, data = matrix("ragged", n)
    x = np.asfortranarray(np.random.default_rng(6).standard_normal((n, 4)))
    setup(c, "A", n, indptr, indices, data, "ell")
    c.spmm_transpose_prepare("ell")
    assert c.spmm_transpose_info()["format"] == "ell"
    y = product_t(c, x)
    # a refused set-up keeps the index and its bits
    bad = indices.copy()
    bad[5] = n
    for where in ("host", "device"):
        assert setup_status(c, "A", n, indptr, bad, data, "sell", where) == capi.ERR_ARG
        assert c.spmm_transpose_info()["format"] == "ell" and same_bits(product_t(c, x), y)
    # a second prepare in another format replaces it; a refused one (unknown format) does not
    c.spmm_transpose_prepare("sell")
    assert c.spmm_transpose_info()["format"] == "sell" and same_bits(product_t(c, x), y)     # (no tail: the same order of summation)
    assert c.lib.dla_spmm_transpose_prepare(c.h, 7) == capi.ERR_ARG
    assert c.spmm_transpose_info()["format"] == "sell" and same_bits(product_t(c, x), y)
    # a set-up of another slot leaves it; an accepted set-up of A through any entry drops it
    setup(c, "B", n, indptr, indices, data, "ell")
    assert same_bits(product_t(c, x), y)
    c.spmm_drop_metric()                                       # (the sharded set-up is refused beside a metric)
    for again in (lambda: setup(c, "A", n, indptr, indices, data, "sell"), lambda: setup(c, "A", n, indptr, indices, data, None),
                  lambda: setup(c, "A", n, indptr, indices, data, "ell", "device"), lambda: setup_csr_one_shard(c, n, indptr, indices, data)):
        c.spmm_transpose_prepare("auto")
        c.spmm_transpose_info()
        again()
        out = capi.SpmmInfo()
        assert c.lib.dla_spmm_transpose_info(c.h, C.byref(out)) == capi.ERR_ARG
        assert "no transposed index" in last_error(c)
        setup(c, "A", n, indptr, indices, data, "ell")          # (whole again behind the shard)
    # drop: idempotent, and the operator stays
    c.spmm_transpose_prepare("auto")
    fwd = product(c, "A", x)
    c.spmm_drop_transpose()
    c.spmm_drop_transpose()
    assert c.lib.dla_spmm_transpose_info(c.h, C.byref(capi.SpmmInfo())) == capi.ERR_ARG and same_bits(product(c, "A", x), fwd)


# ------------------------------------------------------------------------------------------------------------------ refusals
def refused_product(ctx, n, m=2):
    gx, gy = Guarded(ctx, n, m, np.ones((n, m))), Guarded(ctx, n, m)
    st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(T), n, m, gx.ptr, gy.ptr)
    msg = last_error(ctx)
    assert np.all(gy.body() == 7.0), "a refused product has written"
    gx.free(); gy.free()
    return st, msg


def test_refusals():
    n = 64
    indptr, indices, data = matrix("banded", n)
    with fresh_context() as ctx:
        # nothing stored (a refused set-up binds the thread's callbacks to this context)
        assert ctx.lib.dla_spmm_setup_csr(ctx.h, 0, 0, 0, 0) == capi.ERR_ARG
        assert ctx.lib.dla_spmm_transpose_prepare(ctx.h, capi.SPMM_FORMATS["auto"]) == capi.ERR_ARG
        assert last_error(ctx) == "spmm_transpose_prepare: no operator has been set up"
        st, msg = refused_product(ctx, n)
        assert st != 0 and "dla_spmm_matvec_t" in msg and "no operator has been set up" in msg
        assert ctx.lib.dla_spmm_drop_transpose(ctx.h) == 0
        # an operator, no index
        setup(ctx, "A", n, indptr, indices, data, "ell")
        st, msg = refused_product(ctx, n)
        assert st != 0 and "dla_spmm_matvec_t before dla_spmm_transpose_prepare" in msg
        assert ctx.lib.dla_spmm_transpose_info(ctx.h, C.byref(capi.SpmmInfo())) == capi.ERR_ARG
        assert "spmm_transpose_info: no transposed index" in last_error(ctx)
        for bad in (3, -1):
            assert ctx.lib.dla_spmm_transpose_prepare(ctx.h, bad) == capi.ERR_ARG
            assert last_error(ctx) == "spmm_transpose_prepare: unknown format"
        # another n
        ctx.spmm_transpose_prepare("auto")
        st, msg = refused_product(ctx, n + 1)
        assert st != 0 and "dla_spmm_matvec_t" in msg and "n differs from setup" in msg
        # a row-sharded operator
        setup_csr_one_shard(ctx, n, indptr, indices, data)
        assert ctx.lib.dla_spmm_transpose_prepare(ctx.h, capi.SPMM_FORMATS["auto"]) == capi.ERR_ARG
        assert "spmm_transpose_prepare: the operator of this context is row-sharded" in last_error(ctx)
        st, msg = refused_product(ctx, n)
        assert st != 0 and "dla_spmm_matvec_t before dla_spmm_transpose_prepare" in msg


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("kind,n,ft,names", [("ragged", 257, "ell", None), ("banded", 1000, "ell", ["ell_spmm_t_kernel<8>"]),
                                             ("ragged", 257, "sell", ["sell_spmm_t_kernel<8>"]),
                                             ("cross", 5000, "sell", ["sell_spmm_t_kernel<8>", "csr_long_segments_t_kernel<4>", "long_rows_combine_kernel"])])
def test_statistics(c, kind, n, ft, names):
    indptr, indices, data = matrix(kind, n)
    setup(c, "A", n, indptr, indices, data, "auto")
    c.spmm_transpose_prepare(ft)
    ti = c.spmm_transpose_info()
    m, nnz = 5, len(indices)
    if ft == "ell":
        w = ti["stored"] // n
        ladder = [f"ell_spmm_t_kernel<{next(k for k in (4, 8, 16, 32) if w <= k)}>"]         # (the narrowest instance that holds w pairs)
        assert names in (None, ladder), w
        names = ladder
    gx, gy = Guarded(c, n, m, np.ones((n, m))), Guarded(c, n, m)
    c.sync()
    c.reset_stats()
    c._chk(c.lib.dla_call_matvec(c.h, capi.fn_address(T), n, m, gx.ptr, gy.ptr))
    c.sync()
    s, ks = c.stats()["matvec"], c.kernel_stats()
    gx.free(); gy.free()
    entries = ti["stored"] + ti["long_entries"]
    extra = 4 * n + 16 * ti["multi_segments"] * m if ft == "sell" else 0
    assert s["launches"] == len(names)
    assert s["alg_bytes"] == 8 * entries + 8 * nnz + 16 * n * m + extra and s["flops"] == 2 * nnz * m
    for name in names:
        assert ks[name]["launches"] == 1, (name, ks.get(name))
    assert (ks[names[0]]["alg_bytes"], ks[names[0]]["flops"]) == (s["alg_bytes"], s["flops"])
