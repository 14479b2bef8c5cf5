"""GPU: the CSR tail of the sliced sparse operator, split over wavefronts -- csr_long_segments_kernel and long_rows_combine_kernel
behind dla_spmm_matvec / dla_spmm_bvec, the three segment fields of dla_spmm_info, the workspace of partial sums and its booking.

The contract is the one in include/diaglib_amd.h: a tail row is cut into segments of SEG = long_segment_entries entries, one
wavefront forms the partial of a segment (64 strided chains of fused multiply-adds from 0.0, then a butterfly), a row of one
segment is that partial, a longer row is ((part_0 + part_1) + part_2) + ...  The sharp test holds the device to an emulation of
exactly that in exact rational arithmetic, bit for bit.  SEG is read from dla_spmm_info, never written here: tuning it moves the
sizes of this file with it.  The matrix has n = 3 SEG + 70 rows: rows of LONG_ROW + 1, SEG - 1, SEG, SEG + 1, 2 SEG, 2 SEG + 63,
3 SEG + 1 and n entries on distinct rows, everything else 0 .. 5 entries (conventions of tests/test_spmm_formats_gpu.py)."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from diaglib_amd import capi
from spmm_cases import LONG_ROW, csr_from_lengths, fma
from spmm_slots import fresh_context, product, setup
from test_operators_gpu import EPS, LD, Guarded, assert_within, call_matvec, csr_product_reference, spmm_product

pytestmark = pytest.mark.gpu
ELL, SELL = capi.SPMM_ELL, capi.SPMM_SELL
M_ALL = [1, 4, 5, 13]                     # below, at and above the 4 right-hand sides a tail entry is loaded for, and the headline width


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


def emulate_row(vals, xs, seg):
    """one tail row (its values and the gathered entries of one column of x, in the caller's order) by the contract"""
    parts = []
    for s0 in range(0, len(vals), seg):
        acc = [0.0] * 64
        for q, (v, xv) in enumerate(zip(vals[s0:s0 + seg], xs[s0:s0 + seg])):
            acc[q & 63] = fma(v, xv, acc[q & 63])
        for off in (32, 16, 8, 4, 2, 1):
            acc = [acc[lane] + acc[lane ^ off] for lane in range(64)]
        parts.append(acc[0])
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def edge_lengths(seg):
    return [LONG_ROW + 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 63, 3 * seg + 1]


def segment_counts(lens, seg):
    per_row = -(-lens[lens > LONG_ROW] // seg)
    return int(per_row.sum()), int(per_row[per_row > 1].sum())


def edge_matrix(rng, seg, extra_dense=0):
    """n = 3 SEG + 70; the rows of edge_lengths, 1 + extra_dense rows of n entries, the rest 0 .. 5 entries; standard-normal values"""
    n = 3 * seg + 70
    lens = rng.integers(0, 6, n)
    special = edge_lengths(seg) + [n] * (1 + extra_dense)
    rows = rng.choice(n, len(special), replace=False)
    lens[rows] = special
    return n, rows[:7], csr_from_lengths(rng, n, lens)


@pytest.fixture(scope="module")
def case(ctx):
    """the matrix, 13 columns of x, the long-double reference and the emulation of the seven edge rows: computed once, left unchanged"""
    ctx.spmm_setup(sp.identity(2, format="csr"), fmt="sell")
    seg = ctx.spmm_info()["long_segment_entries"]
    rng = np.random.default_rng(2024)
    n, rows, (indptr, indices, data) = edge_matrix(rng, seg)
    x = np.asfortranarray(rng.standard_normal((n, 13)))
    ref, mag = csr_product_reference(indptr, indices, data, x)
    emu = np.empty((len(rows), 13))
    for i, r in enumerate(rows):
        p0, p1 = int(indptr[r]), int(indptr[r + 1])
        vals = data[p0:p1].tolist()
        for c in range(13):
            emu[i, c] = emulate_row(vals, x[indices[p0:p1], c].tolist(), seg)
    for a in (indptr, indices, data, x, emu):
        a.flags.writeable = False
    lens = np.diff(indptr)
    segments, multi = segment_counts(lens, seg)
    return {"seg": seg, "n": n, "rows": rows, "mat": (indptr, indices, data), "x": x, "ref": ref, "mag": mag, "emu": emu,
            "long_rows": int((lens > LONG_ROW).sum()), "segments": segments, "multi": multi}


def columns(case, m):
    return np.asfortranarray(case["x"][:, :m])


# ------------------------------------------------------------------------------------------------------------------ 1. info
def test_info_reports_the_segments(dev, case):
    n, seg, lens = case["n"], case["seg"], np.diff(case["mat"][0])
    setup_fmt(dev, n, *case["mat"], SELL)
    info = dev.spmm_info()
    assert info["long_segment_entries"] == seg and seg > 0 and seg % 64 == 0
    assert (info["long_segments"], info["multi_segments"]) == segment_counts(lens, seg) == (case["segments"], case["multi"])
    # (at SEG = 4096: eight tail rows of 1 + 1 + 1 + 2 + 2 + 3 + 4 + 4 segments, 15 of them in rows of more than one)
    assert info["long_rows"] == case["long_rows"] and info["long_segments"] > info["multi_segments"] >= 2 + 2 + 3 + 4 + 4
    setup_metric(dev, n, *case["mat"], SELL)
    assert dev.spmm_metric_info() == info
    indptr, indices, data = csr_from_lengths(np.random.default_rng(1), 300, np.full(300, 3))
    setup_fmt(dev, 300, indptr, indices, data, ELL)
    info = dev.spmm_info()
    assert info["format"] == "ell" and info["long_segment_entries"] == info["long_segments"] == info["multi_segments"] == 0


# ------------------------------------------------------------------------------------------------------------------ 2. the contract's bits
def test_the_emulation_rounds_once(case):
    """the fused multiply-add of the emulation against its definition, on entries of the matrix itself and on cancelling operands"""
    data, x = case["mat"][2], case["x"]
    acc = 0.0
    for v, xv in zip(data[:2000].tolist(), x[:2000, 0].tolist()):
        want = float(Fraction(v) * Fraction(xv) + Fraction(acc))
        assert fma(v, xv, acc) == want
        acc = want
    for a, b, c in [(1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0), (3.0, 1.0 / 3.0, -1.0), (2.0 ** -600, 2.0 ** -600, 1.0), (0.1, 10.0, -1.0)]:
        assert fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("m", M_ALL)
def test_tail_rows_have_the_bits_of_the_contract(dev, case, m):
    """rows of one segment (LONG_ROW + 1, SEG - 1, SEG) pin the bits the tail had before it was split; the rows of two, three and
    four segments have those of the sum in segment order"""
    n = case["n"]
    setup_fmt(dev, n, *case["mat"], SELL)
    got = spmm_product(dev, n, m, columns(case, m))[case["rows"]]
    want = case["emu"][:, :m]
    for i, length in enumerate(edge_lengths(case["seg"])):
        print(f"m={m} row of {length} entries: {'same bits' if np.array_equal(got[i], want[i]) else f'differs, got {got[i]!r} want {want[i]!r}'}")
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ 3. every row, bounded
@pytest.mark.parametrize("m", M_ALL)
def test_every_row_is_written_and_within_the_bound(dev, case, m):
    n, lens = case["n"], np.diff(case["mat"][0])
    setup_fmt(dev, n, *case["mat"], SELL)
    gx, gy = Guarded(dev, n, m, columns(case, m)), Guarded(dev, n, m, np.full((n, m), np.nan))
    call_matvec(dev, "dla_spmm_matvec", n, m, gx.ptr, gy.ptr)
    got = gy.body().copy()
    gx.assert_unchanged()
    gx.free(); gy.free()
    assert not np.isnan(got).any(), f"rows nobody wrote: {np.flatnonzero(np.isnan(got).any(axis=1))[:10]}"
    ratio = assert_within(got, case["ref"][:, :m], {"(len+2) eps |A||x|": (lens[:, None] + 2) * EPS * case["mag"][:, :m], "tiny": LD(1e-300)},
                          f"split tail n={n} m={m}")
    print(f"n={n} m={m}: worst |got - ref| / bound = {ratio:.3f}")
    assert np.all(got[lens == 0] == 0.0), "an empty row must give exactly 0.0"


# ------------------------------------------------------------------------------------------------------------------ 4. rows outside the tail
def test_rows_outside_the_tail_keep_the_bits_of_ellpack(dev, case):
    """the same matrix with its long rows cut to LONG_ROW entries fits ELLPACK; the rows that were short all along are the same
    rows in both, and come out with the same bits from the sliced format beside a tail and from plain ELLPACK"""
    n, m = case["n"], 13
    indptr, indices, data = case["mat"]
    lens = np.diff(indptr)
    keep = (np.arange(len(indices)) - np.repeat(indptr[:-1], lens)) < LONG_ROW
    cut = np.zeros(n + 1, np.int64)
    np.cumsum(np.minimum(lens, LONG_ROW), out=cut[1:])
    setup_fmt(dev, n, cut, np.ascontiguousarray(indices[keep]), np.ascontiguousarray(data[keep]), ELL)
    assert dev.spmm_info()["format"] == "ell"
    plain = spmm_product(dev, n, m, columns(case, m))
    setup_fmt(dev, n, indptr, indices, data, SELL)
    assert dev.spmm_info()["long_rows"] == case["long_rows"]
    sliced = spmm_product(dev, n, m, columns(case, m))
    short = lens <= LONG_ROW
    assert short.sum() == n - case["long_rows"] and np.array_equal(sliced[short], plain[short])


# ------------------------------------------------------------------------------------------------------------------ 5. determinism, workspace
def test_products_are_deterministic_while_the_workspace_grows_and_operators_change(dev, case):
    """m = 1, 13, 1, 37 on one operator (the workspace of multi_segments x m partial sums grows twice and is reused in between), then
    an operator with more segments, then one with fewer: every product twice, bit-identical, and equal to what a context that
    never held anything else gives (there the widest block comes first, so its workspace never grows)"""
    seg, n = case["seg"], case["n"]
    rng = np.random.default_rng(77)
    n2, _, more = edge_matrix(rng, seg, extra_dense=3)
    n3 = seg + 200
    lens3 = rng.integers(0, 6, n3)
    lens3[5] = n3
    ops = [(n, case["mat"], [1, 13, 1, 37]), (n2, more, [5, 13]), (n3, csr_from_lengths(rng, n3, lens3), [13, 2])]
    xs = {nn: np.asfortranarray(np.random.default_rng(nn).standard_normal((nn, 37))) for nn in (n, n3)}
    results, multi = [], []
    for nn, mat, ms in ops:
        setup_fmt(dev, nn, *mat, SELL)
        multi.append(dev.spmm_info()["multi_segments"])
        for m in ms:
            x = np.asfortranarray(xs[nn][:, :m])
            first, second = spmm_product(dev, nn, m, x), spmm_product(dev, nn, m, x)
            assert np.array_equal(first, second), (nn, m)
            results.append(first)
    assert multi[1] > multi[0] > multi[2] == -(-n3 // seg), multi
    assert np.array_equal(results[0], results[2]), "m = 1 before and after the workspace grew"
    at = 0
    for nn, mat, ms in ops:
        with fresh_context() as c:
            setup_fmt(c, nn, *mat, SELL)
            got = {m: spmm_product(c, nn, m, np.asfortranarray(xs[nn][:, :m])) for m in sorted(set(ms), reverse=True)}
        for m in ms:
            assert np.array_equal(results[at], got[m]), ("a fresh context gives other bits", nn, m)
            at += 1


# ------------------------------------------------------------------------------------------------------------------ 6. the metric slot
def test_bvec_returns_the_operator_bits_on_rows_of_many_segments(dev, case):
    n = case["n"]
    setup_fmt(dev, n, *case["mat"], SELL)
    ax = {m: product(dev, "dla_spmm_matvec", columns(case, m)) for m in (5, 13)}
    setup_metric(dev, n, *case["mat"], SELL)
    assert dev.spmm_metric_info()["multi_segments"] == case["multi"]
    for m in (13, 5):
        assert np.array_equal(product(dev, "dla_spmm_bvec", columns(case, m)), ax[m])
        assert np.array_equal(product(dev, "dla_spmm_matvec", columns(case, m)), ax[m])
    dev.spmm_drop_metric()
    for m in (5, 13):
        assert np.array_equal(product(dev, "dla_spmm_matvec", columns(case, m)), ax[m])
    assert np.array_equal(ax[13][case["rows"]], case["emu"])


# ------------------------------------------------------------------------------------------------------------------ 7. booking
def booked_bytes(ctx, n, m, x):
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    ctx.sync()
    ctx.reset_stats()
    call_matvec(ctx, "dla_spmm_matvec", n, m, gx.ptr, gy.ptr)
    ctx.sync()
    s = ctx.stats()["matvec"]
    gx.free(); gy.free()
    assert s["launches"] == 1, s
    return s["alg_bytes"], s["flops"]


@pytest.mark.parametrize("m", [1, 13])
def test_a_product_books_the_partial_sums_once_written_once_read(dev, case, m):
    n = case["n"]
    setup_fmt(dev, n, *case["mat"], SELL)
    info = dev.spmm_info()
    present = 12.0 * (info["stored"] + info["long_entries"]) + 4.0 * n + 16.0 * n * m
    assert booked_bytes(dev, n, m, columns(case, m)) == (present + 16.0 * info["multi_segments"] * m, 2.0 * info["nnz"] * m)
    # tail rows of one segment only: nothing but the present formula
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 6, n)
    lens[rng.choice(n, 3, replace=False)] = [LONG_ROW + 1, case["seg"] - 1, case["seg"]]
    mat = csr_from_lengths(rng, n, lens)
    setup_fmt(dev, n, *mat, SELL)
    info = dev.spmm_info()
    assert info["long_segments"] == info["long_rows"] == 3 and info["multi_segments"] == 0
    assert booked_bytes(dev, n, m, columns(case, m)) == (12.0 * (info["stored"] + info["long_entries"]) + 4.0 * n + 16.0 * n * m, 2.0 * info["nnz"] * m)


# ------------------------------------------------------------------------------------------------------------------ 8. one small solve
def test_davidson_on_an_arrowhead_matrix(ctx, case):
    """diagonal 1 .. n plus one dense symmetric row and column of 1e-3, n = SEG + 200: the dense row has two segments"""
    n, t, m = case["seg"] + 200, 4, 8
    i = np.arange(1, n)
    arrow = sp.coo_matrix((np.full(n - 1, 1e-3), (np.zeros(n - 1, np.int64), i)), shape=(n, n))
    a = (sp.diags(np.arange(1.0, n + 1.0)) + arrow + arrow.T).tocsr()
    want = np.sort(spl.eigsh(a.tocsc(), k=t, sigma=0.0, which="LM", return_eigenvectors=False))
    g = np.asfortranarray(np.random.default_rng(5).random((n, m)) - 0.5)
    g[200:] *= 1e-3
    ctx.spmm_setup(a, fmt="sell")
    info_op = ctx.spmm_info()
    assert info_op["format"] == "sell" and info_op["long_rows"] == 1 and info_op["multi_segments"] == 2
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    try:
        ev = ctx.panel(g)
        eig, _, ok, info = ctx.davidson_driver(n, t, m, 500, 1e-9, 20, 0.0, capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_precnd"), ev)
        vec = ev.download()
    finally:
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    assert ok, info
    print(f"davidson: iterations {info['iters']}, max rel. eigenvalue difference to eigsh {np.abs(eig[:t] / want - 1).max():.2e}")
    assert np.allclose(eig[:t], want, rtol=1e-9, atol=0)
    x = vec[:, :t]
    assert np.abs(x.T @ x - np.eye(t)).max() < 1e-10
    assert np.linalg.norm(a @ x - x * eig[None, :t], axis=0).max() < 1e-6
