"""GPU: the device-resident operators and preconditioners, kernel by kernel -- ell_spmm_kernel<4|8|16|32|general>, diag_precnd_kernel,
synth_apply_kernel (six kinds), synth_precnd_kernel<1|2>, synth_lrprec_kernel, random_fill_kernel, axpy / sumsq and the CSR -> ELLPACK
conversion of dla_spmm_setup_csr.  These are what every device-mode solve multiplies by; the solver tests only see them through
solves that converge or residuals formed with the same operator.

Conventions
  * references are computed in np.longdouble from the operator's DEFINITION (raw CSR triplets, the table above synth_apply_kernel),
    so only the kernel's own rounding is measured;
  * every output block sits between two sentinel columns of 7.0 and is itself prefilled with 7.0: the sentinels must survive, every
    entry of the block must have been written, the inputs must come back unchanged;
  * shapes straddle one block of 256 rows, the ELLPACK width buckets (4, 8, 16, 32, general) and -- once per kernel -- the
    launch cap of 8 blocks of 256 threads per compute unit, beyond which the grid-stride loops take a second trip.

The generators and checkers are plain functions of (ctx, rng, shape): tools/fuzz_operators.py sweeps them over random shapes."""
import ctypes as C

import numpy as np
import pytest

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SENT = 7.0
ROW0_FAR = 5_000_001                      # a shard in the middle of n_global = 1e7 rows: i mod 7, sqrt(i) and i + 1 all differ from row0 = 0
N_GLOBAL_FAR = 10 ** 7
# one grid-stride trip covers 8 blocks x 256 threads = 2048 rows per compute unit: 524 288 on the 256 CUs of an MI355X.  700 001 rows
# (odd: scalar paths) need a second trip on up to 341 CUs (341 * 2048 = 698 368); synth_precnd_kernel<2> handles two rows per thread,
# so its second trip needs twice that, 1 400 002 (even).
N_TRIP, N_TRIP2 = 700_001, 1_400_002


@pytest.fixture()
def dev(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def _assert_second_trip(rows_per_thread=1, n=N_TRIP):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n > 8 * 256 * cus * rows_per_thread, (n, cus)


# ------------------------------------------------------------------------------------------------------------------ plumbing
class Guarded:
    """An n x m device block between two sentinel columns.  `fill` = the block's content (an input), None = prefilled with the
    sentinel (an output).  offset = 8 places the whole panel 8 bytes past a 16-byte aligned allocation."""

    def __init__(self, ctx, n, m, fill=None, offset=0):
        self.ctx, self.n, self.m, self.raw = ctx, n, m, None
        self.host = np.full((n, m + 2), SENT, order="F")
        if fill is not None:
            self.host[:, 1:m + 1] = fill
        if offset:
            raw = C.c_void_p()
            ctx._chk(ctx.lib.dla_alloc(ctx.h, 8 * n * (m + 2) + 16, C.byref(raw)))
            self.raw = raw.value
            assert self.raw % 16 == 0, self.raw
            self.whole = capi.DevPanel(ctx, n, m + 2, ptr=self.raw + offset, owner=False)
        else:
            self.whole = capi.DevPanel(ctx, n, m + 2)
            assert self.whole.ptr % 16 == 0, self.whole.ptr
        self.whole.upload(self.host)
        self.ptr = self.whole.ptr + 8 * n            # (odd n: the block itself is then 8-byte aligned only)

    def body(self):
        """the block, after checking that both sentinel columns survived"""
        got = self.whole.download()
        assert np.all(got[:, 0] == SENT) and np.all(got[:, -1] == SENT), "a sentinel column next to the output block was overwritten"
        return got[:, 1:-1]

    def assert_unchanged(self):
        assert np.array_equal(self.whole.download(), self.host), "an input block (or its sentinel columns) was modified"

    def free(self):
        self.whole.free()
        if self.raw:
            self.ctx.lib.dla_free(self.ctx.h, self.raw)
            self.raw = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def call_matvec(ctx, name, n, m, x_ptr, y_ptr):
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, x_ptr, y_ptr))


def call_precnd(ctx, name, n, m, fac, x_ptr, y_ptr):
    ctx._chk(ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, float(fac), x_ptr, y_ptr))


def assert_within(got, ref, terms, what):
    """|got - ref| <= sum(terms) elementwise; on failure the largest violation, where it is and what each term of the bound is there"""
    bound = sum(terms.values())
    err = np.abs(got.astype(LD) - ref)
    assert np.all(np.isfinite(got)), what + ": non-finite output"
    ratio = err / bound
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[at] <= 1.0, (f"{what}: |got - ref| = {float(err[at]):.3e} at {at} is {float(ratio[at]):.2f} x the bound; terms there: "
                              + ", ".join(f"{k} = {float(np.broadcast_to(v, err.shape)[at]):.3e}" for k, v in terms.items()))
    return float(ratio[at])


# ------------------------------------------------------------------------------------------------------------------ ELLPACK product
def ragged_csr(rng, n, w_max, eighths=False):
    """Raw CSR arrays (indptr int64, indices int32, data float64) of an n x n matrix that is nothing like a band:
    row lengths 0 .. w_max with at least one row of w_max entries and (n >= 3) at least one empty row; columns uniform over [0, n):
    unsorted, long-range, non-symmetric; about 10 % of the entries repeat a column of their row; about 5 % explicit zeros; about a
    third of the rows without a diagonal entry, a quarter of the others with two.  eighths: values are multiples of 1/8, |v| <= 5,
    so that duplicate entries sum exactly in any order."""
    lens = rng.integers(0, w_max + 1, n)
    if n >= 3:
        full, empty = rng.choice(n, 2, replace=False)
        lens[full], lens[empty] = w_max, 0
    else:
        lens[rng.integers(n)] = w_max
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(nnz, dtype=np.int64) - indptr[rows]
    cols = rng.integers(0, n, nnz)
    dup = (pos >= 1) & (rng.random(nnz) < 0.1)
    cols[dup] = cols[indptr[rows[dup]] + (rng.random(int(dup.sum())) * pos[dup]).astype(np.int64)]
    with_diag = rng.random(n) < 2.0 / 3.0
    if n > 1:
        hit = (cols == rows) & ~with_diag[rows]
        cols[hit] = (cols[hit] + 1) % n
    r1 = np.flatnonzero(with_diag & (lens >= 1))
    cols[indptr[r1] + (rng.random(r1.size) * lens[r1]).astype(np.int64)] = r1
    r2 = r1[(lens[r1] >= 2) & (rng.random(r1.size) < 0.25)]
    cols[indptr[r2] + (rng.random(r2.size) * lens[r2]).astype(np.int64)] = r2
    data = rng.integers(-40, 41, nnz) / 8.0 if eighths else rng.standard_normal(nnz)
    data[rng.random(nnz) < 0.05] = 0.0
    return indptr, np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(data, dtype=np.float64)


def csr_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def csr_product_reference(indptr, indices, data, x):
    """A x and |A| |x| straight from the triplets (scipy would sort the columns and sum the duplicates of a non-canonical
    csr_matrix in place -- and hand the engine a cleaned matrix)"""
    rows = csr_rows(indptr)
    ref = np.zeros(x.shape, LD)
    mag = np.zeros(x.shape, LD)
    np.add.at(ref, rows, data.astype(LD)[:, None] * x.astype(LD)[indices])
    np.add.at(mag, rows, np.abs(data).astype(LD)[:, None] * np.abs(x).astype(LD)[indices])
    return ref, mag


def csr_diagonal(indptr, indices, data):
    """the sum of all (i, i) entries, 0 where a row has none"""
    rows = csr_rows(indptr)
    d = np.zeros(len(indptr) - 1)
    on = indices == rows
    np.add.at(d, rows[on], data[on])
    return d


def setup_csr(ctx, n, indptr, indices, data):
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
    ctx._chk(ctx.lib.dla_spmm_setup_csr(ctx.h, n, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data))


def setup_csr_one_shard(ctx, n, indptr, indices, data):
    gi = np.ascontiguousarray(indices, dtype=np.int64)
    ctx._chk(ctx.lib.dla_spmm_setup_csr_sharded(ctx.h, n, 0, n, indptr.ctypes.data, gi.ctypes.data, data.ctypes.data))


def spmm_product(ctx, n, m, x):
    """dla_spmm_matvec on x between sentinels; sentinels, inputs checked"""
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    call_matvec(ctx, "dla_spmm_matvec", n, m, gx.ptr, gy.ptr)
    got = gy.body().copy()
    gx.assert_unchanged()
    gx.free(); gy.free()
    return got


def check_spmm(ctx, rng, n, w_max, m, sharded=False):
    """set up a ragged matrix and check one product: the dot-product bound of w_max fused terms ((w_max + 2) eps |A| |x|: padding
    lanes contribute exact zeros), exact zeros on empty rows"""
    indptr, indices, data = ragged_csr(rng, n, w_max)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    (setup_csr_one_shard if sharded else setup_csr)(ctx, n, indptr, indices, data)
    got = spmm_product(ctx, n, m, x)
    ref, mag = csr_product_reference(indptr, indices, data, x)
    assert_within(got, ref, {"(w+2) eps |A||x|": (w_max + 2) * EPS * mag, "tiny": LD(1e-300)}, f"spmm n={n} w_max={w_max} m={m}")
    empty = np.diff(indptr) == 0
    assert np.all(got[empty] == 0.0), "an empty row must give exactly 0.0"
    return indptr, indices, data, x, got


# every w_max with an n below, at and above one block of 256 rows, plus one of the remaining sizes; the four block widths in turn
_W = [1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 70]
_M = [1, 5, 13, 37]
SPMM_CASES = [(w, n, _M[(k + t) % 4]) for k, w in enumerate(_W) for t, n in enumerate([255, 256, 257, [1, 2, 1000][k % 3]])]


@pytest.mark.parametrize("w_max,n,m", SPMM_CASES)
def test_spmm_on_ragged_unsorted_matrices(dev, rng, w_max, n, m):
    """all five width buckets at their boundaries (w == W: no padding lane; w == W + 1: the next bucket), short and empty rows,
    duplicates, explicit zeros, missing diagonals, unsorted long-range columns"""
    check_spmm(dev, rng, n, w_max, m)


def test_spmm_and_its_preconditioner_take_a_second_stride_trip(dev, rng):
    """n = 700 001, w_max = 5, m = 2: rows beyond the first 2048 x CUs are computed in the second trip of the grid-stride loop"""
    _assert_second_trip()
    n, m = N_TRIP, 2
    try:
        indptr, indices, data, x, _ = check_spmm(dev, rng, n, 5, m)
        diag = csr_diagonal(indptr, indices, data)
        gx, gp = Guarded(dev, n, m, x), Guarded(dev, n, m)
        call_precnd(dev, "dla_spmm_precnd", n, m, 0.375, gx.ptr, gp.ptr)
        den = (diag + 0.375)[:, None]
        want = np.where(np.abs(den) > 1e-5, x / den, x)
        # one rounding of the ELLPACK diagonal (duplicates summed in another order than here), carried through the division
        assert_within(gp.body(), want.astype(LD), {"4 eps |want|": 4 * EPS * np.abs(want), "diag rounding": 4 * EPS * np.abs(want) * np.abs(diag[:, None] / den)},
                      "spmm_precnd at n = 700 001")
        gx.assert_unchanged()
        gx.free(); gp.free()
    finally:
        dev.trim()


def test_spmm_setup_again_with_a_smaller_matrix(dev, rng):
    """The device arrays only grow: after n = 5000, w = 41 a setup with n = 100, w = 3 leaves the larger blocks in place and the
    kernels must go by the new n and w.  A call with the old n is then refused, and the context goes on working."""
    check_spmm(dev, rng, 5000, 41, 3)
    check_spmm(dev, rng, 100, 3, 5)
    gx, gy = Guarded(dev, 5000, 2, np.ones((5000, 2))), Guarded(dev, 5000, 2)
    with pytest.raises(capi.DlaError, match="n differs from setup"):
        call_matvec(dev, "dla_spmm_matvec", 5000, 2, gx.ptr, gy.ptr)
    with pytest.raises(capi.DlaError, match="n differs from setup"):
        call_precnd(dev, "dla_spmm_precnd", 5000, 2, 1.0, gx.ptr, gy.ptr)
    assert np.all(gy.body() == SENT)                          # nothing was written
    x = np.asfortranarray(rng.standard_normal((100, 5)))
    assert np.all(np.isfinite(spmm_product(dev, 100, 5, x)))  # the n = 100 operator is still there
    check_spmm(dev, rng, 257, 9, 2)


@pytest.mark.parametrize("w_max,n,m", [(5, 257, 5), (17, 1000, 13), (70, 256, 1)])
def test_one_shard_equals_the_unsharded_setup_bit_for_bit(dev, rng, w_max, n, m):
    """include/diaglib_amd.h: 'with one rank it equals dla_spmm_setup_csr' -- the halo kernel with halo = 0 on a ragged matrix"""
    indptr, indices, data, x, plain = check_spmm(dev, rng, n, w_max, m)
    diag = csr_diagonal(indptr, indices, data)
    setup_csr_one_shard(dev, n, indptr, indices, data)
    assert np.array_equal(spmm_product(dev, n, m, x), plain)
    gx, gp = Guarded(dev, n, m, x), Guarded(dev, n, m)
    call_precnd(dev, "dla_spmm_precnd", n, m, 0.375, gx.ptr, gp.ptr)
    den = (diag + 0.375)[:, None]
    want = np.where(np.abs(den) > 1e-5, x / den, x)
    assert_within(gp.body(), want.astype(LD), {"4 eps |want|": 4 * EPS * np.abs(want), "diag rounding": 4 * EPS * np.abs(want) * np.abs(diag[:, None] / den)},
                  "spmm_precnd after the one-shard setup")


def _bad_setups(n):
    """(what, indptr, indices, message) of CSR arrays the setups must refuse"""
    idx = np.zeros(8, np.int32)
    return [("descending row pointers", np.array([0, 3, 2, 5] + [5] * (n - 3), np.int64), idx, "row pointers not ascending"),
            ("column index n", np.array([0, 1, 2, 3] + [3] * (n - 3), np.int64), np.array([0, n, 1, 0, 0, 0, 0, 0], np.int32), "column index out of range"),
            ("column index -1", np.array([0, 1, 2, 3] + [3] * (n - 3), np.int64), np.array([0, 1, -1, 0, 0, 0, 0, 0], np.int32), "column index out of range"),
            ("no entries at all", np.zeros(n + 1, np.int64), idx, "empty")]


@pytest.mark.parametrize("sharded", [False, True])
def test_setup_refuses_malformed_csr_and_the_context_survives(dev, rng, sharded):
    """descending row pointers (the unsharded setup used to take such a row for an empty one), a column outside [0, n), a matrix
    without entries: an error from both setups, in the same words, and the operator set up before is still usable"""
    n = 6
    indptr, indices, data, x, before = check_spmm(dev, rng, 300, 9, 3)
    val = np.ones(8)
    for what, rp, ci, msg in _bad_setups(n):
        with pytest.raises(capi.DlaError, match=msg):
            (setup_csr_one_shard if sharded else setup_csr)(dev, n, rp, ci, val)
        assert np.array_equal(spmm_product(dev, 300, 3, x), before), what      # a refused setup replaces nothing
    check_spmm(dev, rng, n, 2, 2, sharded=sharded)


# ------------------------------------------------------------------------------------------------------------------ diagonal preconditioner
def check_spmm_precnd(ctx, rng, n, w_max, m):
    """dla_spmm_precnd on a matrix whose values are multiples of 1/8 (the expected diagonal is exact): the guard |d + fac| <= 1e-5
    passes x through bit for bit, 2^-16 outside it divides; rows without a diagonal entry have d = 0"""
    indptr, indices, data = ragged_csr(rng, n, w_max, eighths=True)
    diag = csr_diagonal(indptr, indices, data)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    setup_csr(ctx, n, indptr, indices, data)
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
        assert_within(got, want.astype(LD), {"4 eps |want|": 4 * EPS * np.abs(want), "tiny": LD(1e-300)}, f"spmm_precnd n={n} w_max={w_max} fac={fac!r}")
        if delta is not None:
            assert diag[j] + fac == delta                                # (exact: multiples of 1/8 and a power of two)
            if abs(delta) <= 2.0 ** -17:
                assert np.array_equal(got[j], x[j]), ("inside the guard: x passes through", delta)
            else:
                assert np.array_equal(got[j], x[j] / delta), ("outside the guard: x / delta", delta)
        else:
            assert np.array_equal(got[~has_diag], x[~has_diag] / fac if fac else x[~has_diag]), ("rows without a diagonal entry", fac)
        gp.free()
    gx.assert_unchanged()
    gx.free()


@pytest.mark.parametrize("n,w_max,m", [(1, 3, 1), (2, 4, 5), (255, 5, 13), (256, 9, 3), (257, 17, 2), (1000, 33, 7)])
def test_spmm_precnd_diagonal_and_guard(dev, rng, n, w_max, m):
    check_spmm_precnd(dev, rng, n, w_max, m)


# ------------------------------------------------------------------------------------------------------------------ built-in operator
def synth_precnd_want(diag, fac, x):
    den = (diag + fac)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(np.abs(den) > 1e-5, x / den, x)
        amp = np.where(np.abs(den) > 1e-5, np.abs(diag[:, None] / den), 0.0)
    # 4 eps: the division (the suite's constant for this kernel family); second term: the oracle's diagonal may differ from the
    # device's by one rounding, d (1 + eps) + fac moves the quotient by eps |d| / |den|
    terms = {"4 eps |want|": 4 * EPS * np.abs(want), "diag rounding": 4 * EPS * amp * np.abs(want), "tiny": LD(1e-300)}
    return want, terms


def check_synth_precnd(ctx, oracle, rng, n, m, row0=0, n_global=None, fac=-0.75, x_offset=0, px_offset=0, guard_row=None):
    """dla_synth_precnd against x / (diag + fac) with the oracle's diagonal; guard_row = j: fac = -diag[j], row j passes through
    exactly while its neighbour in the same 16-byte pair is divided"""
    n_global = n if n_global is None else n_global
    ctx.synth_setup(n_global, row0, n); oracle.synth_setup(n_global, row0, n)
    diag = oracle.synth_diag()
    x = np.asfortranarray(rng.standard_normal((n, m)))
    if guard_row is not None:
        fac = -diag[guard_row]
    gx, gp = Guarded(ctx, n, m, x, offset=x_offset), Guarded(ctx, n, m, offset=px_offset)
    call_precnd(ctx, "dla_synth_precnd", n, m, fac, gx.ptr, gp.ptr)
    got = gp.body()
    want, terms = synth_precnd_want(diag, fac, x)
    if guard_row is not None:
        j = guard_row
        assert np.array_equal(got[j], x[j]), ("row inside the guard: x passes through bit for bit", j)
        if (j ^ 1) < n:
            assert abs(diag[j ^ 1] + fac) > 1e-3 and not np.array_equal(got[j ^ 1], x[j ^ 1]), ("the other lane of the pair is divided", j ^ 1)
        got, want = np.delete(got, j, 0), np.delete(want, j, 0)
        terms = {k: (np.delete(np.broadcast_to(v, x.shape), j, 0)) for k, v in terms.items()}
    if got.size:
        assert_within(got, want.astype(LD), terms, f"synth_precnd n={n} m={m} row0={row0} fac={fac!r} offsets=({x_offset},{px_offset})")
    gx.assert_unchanged()
    gx.free(); gp.free()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 1001])
@pytest.mark.parametrize("m", [1, 8, 13])
def test_synth_precnd(dev, oracle, rng, n, m):
    """even n: two rows per thread (16-byte accesses); odd n: one"""
    check_synth_precnd(dev, oracle, rng, n, m)


@pytest.mark.parametrize("which", ["x", "px"])
def test_synth_precnd_on_a_block_that_is_not_16_byte_aligned(dev, oracle, rng, which):
    """even n, but x (or px) starts 8 bytes into a 16-byte aligned allocation: the two-row kernel must not be chosen"""
    check_synth_precnd(dev, oracle, rng, 1000, 5, x_offset=8 if which == "x" else 0, px_offset=8 if which == "px" else 0)


@pytest.mark.parametrize("j", [400, 401, 0, 999])
def test_synth_precnd_guard_is_taken_per_row(dev, oracle, rng, j):
    """fac = -diag[j], n even and aligned: rows j and j ^ 1 share one 16-byte pair; only row j is inside the guard"""
    check_synth_precnd(dev, oracle, rng, 1000, 3, guard_row=j)


@pytest.mark.parametrize("n", [256, 257, 1000, 1001])
def test_synth_precnd_on_a_shard(dev, oracle, rng, n):
    check_synth_precnd(dev, oracle, rng, n, 4, row0=ROW0_FAR, n_global=N_GLOBAL_FAR)
    check_synth_precnd(dev, oracle, rng, n, 4, row0=ROW0_FAR, n_global=N_GLOBAL_FAR, guard_row=n // 2 + 1)


@pytest.mark.parametrize("n,rows_per_thread", [(N_TRIP2, 2), (N_TRIP, 1)])
def test_synth_precnd_takes_a_second_stride_trip(dev, oracle, rng, n, rows_per_thread):
    _assert_second_trip(rows_per_thread, n)
    try:
        check_synth_precnd(dev, oracle, rng, n, 2, guard_row=n - 2)       # (a guarded row in the second trip)
    finally:
        dev.trim()


def test_synth_precnd_refuses_another_n(dev, oracle, rng):
    dev.synth_setup(1000, 0, 1000)
    gx, gp = Guarded(dev, 998, 2, np.ones((998, 2))), Guarded(dev, 998, 2)
    with pytest.raises(capi.DlaError, match="n differs from setup"):
        call_precnd(dev, "dla_synth_precnd", 998, 2, 1.0, gx.ptr, gp.ptr)
    assert np.all(gp.body() == SENT)
    check_synth_precnd(dev, oracle, rng, 1000, 2)


# ---- synth_apply: y = d(i) x + W C W^T x, restated from the table above synth_apply_kernel (i = 1-based global row)
SIGMA, TAU = 0.5, 0.05
_J = np.array([[0.0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1], [0, 0, -1, 0]])
SYNTH_KINDS = {   # entry point: (offset of the diagonal d = i + offset, or None for d = s(i);  the 4 x 4 coupling C)
    "dla_synth_matvec": (1.0, SIGMA * np.eye(4)),
    "dla_synth_apbmul": (5.0, SIGMA * np.eye(4)),
    "dla_synth_ambmul": (2.0, (0.2 * SIGMA) * np.eye(4)),
    "dla_synth_spdmul": (None, TAU * _J),
    "dla_synth_smdmul": (None, -TAU * _J),
    "dla_synth_metric": (None, 0.1 * np.eye(4)),
}


def synth_s(gi):
    return LD(1) + LD(0.5) / (LD(1) + (gi % 7).astype(LD))


def synth_apply_reference(name, w, x, row0):
    """(ref, bound terms) of one sample operator in longdouble, matrix-free"""
    off, cpl = SYNTH_KINDS[name]
    gi = np.arange(w.shape[0], dtype=np.int64) + row0 + 1
    d = (gi.astype(LD) + LD(off)) if off is not None else synth_s(gi)
    wl, xl, cl = w.astype(LD), x.astype(LD), cpl.astype(LD)
    ref = d[:, None] * xl + wl @ (cl @ (wl.T @ xl))
    mag = np.abs(wl) @ (np.abs(cl) @ (np.abs(wl).T @ np.abs(xl)))
    return ref, {"64 eps |d||x|": 64 * EPS * np.abs(d)[:, None] * np.abs(xl), "64 eps |W||C||W|^T|x|": 64 * EPS * mag, "tiny": LD(1e-300)}


def check_synth_apply(ctx, oracle, rng, n, m, row0=0, n_global=None, names=tuple(SYNTH_KINDS)):
    n_global = n if n_global is None else n_global
    ctx.synth_setup(n_global, row0, n); oracle.synth_setup(n_global, row0, n)
    w = oracle.synth_w()
    x = np.asfortranarray(rng.standard_normal((n, m)))
    gx = Guarded(ctx, n, m, x)
    for name in names:
        gy = Guarded(ctx, n, m)
        call_matvec(ctx, name, n, m, gx.ptr, gy.ptr)
        ref, terms = synth_apply_reference(name, w, x, row0)
        assert_within(gy.body(), ref, terms, f"{name} n={n} m={m} row0={row0}")
        gy.free()
    gx.assert_unchanged()
    gx.free()


@pytest.mark.parametrize("n", [1, 255, 257, 1000, 1001])
@pytest.mark.parametrize("m", [1, 7, 37, 64])
def test_synth_apply_all_kinds(dev, oracle, rng, n, m):
    check_synth_apply(dev, oracle, rng, n, m)


@pytest.mark.parametrize("n", [1, 255, 257, 1000, 1001])
@pytest.mark.parametrize("m", [1, 7, 37, 64])
def test_synth_apply_all_kinds_on_a_shard(dev, oracle, rng, n, m):
    """row0 = 5 000 001: d = i + c, s(i mod 7) and W(i) all go by the GLOBAL row"""
    check_synth_apply(dev, oracle, rng, n, m, row0=ROW0_FAR, n_global=N_GLOBAL_FAR)


def test_synth_apply_refuses_more_than_64_columns(dev, oracle, rng):
    n = 300
    dev.synth_setup(n, 0, n)
    gx, gy = Guarded(dev, n, 65, np.ones((n, 65))), Guarded(dev, n, 65)
    for name in SYNTH_KINDS:
        with pytest.raises(capi.DlaError, match="m > 64"):
            call_matvec(dev, name, n, 65, gx.ptr, gy.ptr)
    assert np.all(gy.body() == SENT)
    check_synth_apply(dev, oracle, rng, n, 64)


def test_synth_apply_takes_a_second_stride_trip(dev, oracle, rng):
    """n = 700 001, m = 2, kinds A and S + D: the operator against its definition (not against itself) beyond one trip"""
    _assert_second_trip()
    try:
        check_synth_apply(dev, oracle, rng, N_TRIP, 2, names=("dla_synth_matvec", "dla_synth_spdmul"))
    finally:
        dev.trim()


# ---- lrprec_1 / lrprec_2 on the diagonals of the sample operators
def check_synth_lrprec(ctx, oracle, rng, n, m, row0=0, n_global=None):
    n_global = n if n_global is None else n_global
    ctx.synth_setup(n_global, row0, n); oracle.synth_setup(n_global, row0, n)
    w = oracle.synth_w().astype(LD)
    gi = np.arange(n, dtype=np.int64) + row0 + 1
    wsq = (w * w).sum(1)
    aa = (LD(0.5) * ((gi.astype(LD) + 5 + LD(SIGMA) * wsq) + (gi.astype(LD) + 2 + LD(0.2 * SIGMA) * wsq)))[:, None]
    s = synth_s(gi)[:, None]
    xp, xm = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
    gxp, gxm = Guarded(ctx, n, m, xp), Guarded(ctx, n, m, xm)
    xpl, xml = xp.astype(LD), xm.astype(LD)
    for variant, fac in [(1, 0.37), (2, 2.5)]:
        f = LD(fac)
        if variant == 1:
            den = aa * aa - f * f * s * s
            inv, ca, cs = -1 / den, aa, f * s
        else:
            den = f * f * aa * aa - s * s
            inv, ca, cs = 1 / den, f * aa, s
        assert np.all(den > 1.0)                 # aa >= 4.5, s <= 1.5: no denominator comes near zero for these fac
        gyp, gym = Guarded(ctx, n, m), Guarded(ctx, n, m)
        ctx._chk(ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(f"dla_synth_lrprec{variant}"), n, m, fac, gxp.ptr, gxm.ptr, gyp.ptr, gym.ptr))
        for got, a, b, nm in [(gyp.body(), xpl, xml, "yp"), (gym.body(), xml, xpl, "ym")]:
            ref = inv * (ca * a + cs * b)
            assert_within(got, ref, {"32 eps |den| |aa||x1|": 32 * EPS * np.abs(inv) * np.abs(ca) * np.abs(a),
                                     "32 eps |den| |fac s||x2|": 32 * EPS * np.abs(inv) * np.abs(cs) * np.abs(b), "tiny": LD(1e-300)},
                          f"lrprec{variant} {nm} n={n} m={m} row0={row0}")
        gyp.free(); gym.free()
    gxp.assert_unchanged(); gxm.assert_unchanged()
    gxp.free(); gxm.free()


@pytest.mark.parametrize("n,m", [(1, 1), (255, 7), (257, 3), (1000, 5), (1001, 2)])
@pytest.mark.parametrize("row0", [0, ROW0_FAR])
def test_synth_lrprec(dev, oracle, rng, n, m, row0):
    check_synth_lrprec(dev, oracle, rng, n, m, row0=row0, n_global=N_GLOBAL_FAR if row0 else None)


def test_synth_lrprec_takes_a_second_stride_trip(dev, oracle, rng):
    _assert_second_trip()
    try:
        check_synth_lrprec(dev, oracle, rng, N_TRIP, 2)
        gx = Guarded(dev, 10, 1, np.ones((10, 1)))
        with pytest.raises(capi.DlaError, match="n differs from setup"):
            dev._chk(dev.lib.dla_call_lrprec(dev.h, capi.fn_address("dla_synth_lrprec1"), 10, 1, 0.37, gx.ptr, gx.ptr, gx.ptr, gx.ptr))
    finally:
        dev.trim()


# ------------------------------------------------------------------------------------------------------------------ generator
def check_random_fill(ctx, n, m, row0=0, seed=2, support_rows=0):
    """dla_fill_guess (seed, offset -0.5, support_rows) and dla_random_fill (seed 7, offset 0, no support) over the whole panel,
    bit for bit, against the oracle's restatement of the generator.  Both entry points pass the context's row0 down
    (host_logic.cpp), so both are rows row0 + 1 .. row0 + n of the global stream."""
    from oracle.pyoracle import Oracle
    if row0:
        ctx.set_shard(row0 + n + 1000, row0)
    try:
        g = Guarded(ctx, n, m)
        ctx._chk(ctx.lib.dla_fill_guess(ctx.h, n, m, g.ptr, seed, support_rows))
        want = Oracle.guess_u01(seed, n, m, row0=row0, offset=-0.5)
        if support_rows > 0:
            want[np.arange(n) + row0 >= support_rows] = 0.0
        assert np.array_equal(g.body(), want), dict(n=n, m=m, row0=row0, seed=seed, support_rows=support_rows)
        g.free()
        g = Guarded(ctx, n, m)
        ctx._chk(ctx.lib.dla_random_fill(ctx.h, n, m, g.ptr))
        got = g.body()
        assert np.array_equal(got, Oracle.guess_u01(7, n, m, row0=row0, offset=0.0)), dict(n=n, m=m, row0=row0)
        assert 0.0 <= got.min() and got.max() < 1.0
        g.free()
    finally:
        if row0:
            ctx.set_shard(-1, 0)


@pytest.mark.parametrize("n,m", [(1, 1), (257, 64), (3001, 7), (100_003, 7)])
@pytest.mark.parametrize("row0", [0, 12_345, 5 * 10 ** 9])
def test_random_fill_whole_panel(ctx, n, m, row0):
    """(100 003 x 7 = 700 021 entries: the second stride trip; row0 = 5e9: the row counter is 64 bits wide)"""
    if n * m > N_TRIP:
        _assert_second_trip(1, n * m)
    check_random_fill(ctx, n, m, row0=row0)


@pytest.mark.parametrize("row0", [0, 12_345, 5 * 10 ** 9])
def test_fill_guess_support_rows(ctx, row0):
    n, m = 3001, 7
    for support in (row0 + 1500, row0 + 1, row0, row0 + n, row0 + n + 10, row0 - 5):
        if support > 0:
            check_random_fill(ctx, n, m, row0=row0, seed=3, support_rows=support)


# ------------------------------------------------------------------------------------------------------------------ axpy / nrm2
def check_axpy_nrm2(ctx, rng, n, m, alpha):
    """on the n x m block behind one sentinel column (odd n: the block is 8-byte aligned only)"""
    x, y = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m, y)
    ctx._chk(ctx.lib.dla_axpy(ctx.h, n * m, float(alpha), gx.ptr, gy.ptr))
    ref = y.astype(LD) + LD(alpha) * x.astype(LD)
    got = gy.body()
    assert_within(got, ref, {"2 eps |y|": 2 * EPS * np.abs(y), "2 eps |alpha x|": 2 * EPS * np.abs(alpha * x), "tiny": LD(1e-300)}, f"axpy len={n * m} alpha={alpha}")
    if alpha == 0.0:
        assert np.array_equal(got, y)
    out = C.c_double(-1.0)
    ctx._chk(ctx.lib.dla_nrm2(ctx.h, n * m, gx.ptr, C.byref(out)))
    want = np.sqrt((x.astype(LD) ** 2).sum())
    assert abs(LD(out.value) - want) <= 64 * EPS * want, (out.value, float(want), n, m)
    gx.assert_unchanged()
    gx.free(); gy.free()


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (255, 1), (257, 1), (257, 3), (N_TRIP2, 1)])
@pytest.mark.parametrize("alpha", [0.37, 0.0])
def test_axpy_nrm2(ctx, rng, n, m, alpha):
    """(257 x 3 behind column 0 of an odd-n panel: a column view that is 8-byte aligned only; 1 400 002: second stride trip)"""
    try:
        check_axpy_nrm2(ctx, rng, n, m, alpha)
    finally:
        if n >= N_TRIP:
            ctx.trim()
