"""CPU: the transposed index of the sparse operator (dla::spmm_transpose_build and what it calls in diaglib_amd/csrc/dla_internal.h;
the contract: include/diaglib_amd.h, dla_spmm_transpose_prepare).

tests/spmm_transpose_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_sell_layout.py does): it lays A out and builds the index with the product's own host code, forms A^T x by walking the
index the way the three kernels do and writes what it saw.  Here that product is held to the raw triplets (exact on integers, the
bound (len_j + 2) eps |A|^T |x| against long double), to the order contract (the bits of the forward walk over the explicitly
transposed arrays in the index's format) and the index to its structure."""
import os
import subprocess

import numpy as np
import pytest

import hostsim
from spmm_cases import LONG_ROW, SLICE, csr_from_lengths
from test_operators_gpu import EPS, LD, assert_within, csr_rows, ragged_csr

SRC = os.path.join(hostsim.ROOT, "tests", "spmm_transpose_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"), os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "spmm_transpose_driver")
ERR_ARG = 3
ELL, SELL, AUTO = 0, 1, 2
SEG = 4096
HEAD = ("n", "m", "nnz", "a_fmt", "a_stored", "a_total", "t_fmt", "t_w", "t_stored", "t_slices", "t_long_rows", "t_long_entries",
        "t_long_segments", "t_multi_segments", "entries")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("spmm_t")

    def run(n, indptr, indices, data, x, fmt_a, fmt_t):
        m = x.shape[1]
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        with open(fin, "wb") as f:
            np.array([n, m, len(indices), fmt_a, fmt_t], np.int64).tofile(f)
            np.ascontiguousarray(indptr, np.int64).tofile(f)
            np.ascontiguousarray(indices, np.int32).tofile(f)
            np.ascontiguousarray(data, np.float64).tofile(f)
            np.asfortranarray(x, np.float64).T.tofile(f)
        p = subprocess.run([EXE, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        raw = open(fout, "rb").read()
        status = int(np.frombuffer(raw, np.int64, 1)[0])
        if status:
            return {"status": status, "message": p.stdout}
        at = 8

        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a
        out = dict(zip(HEAD, (int(v) for v in take(np.int64, len(HEAD)))), status=0)
        assert (out["n"], out["m"]) == (n, m)
        out["y"], out["z"] = take(np.float64, n * m).reshape(m, n).T, take(np.float64, n * m).reshape(m, n).T
        out["writes"] = take(np.int32, n)
        out["row"], out["pos"] = take(np.int32, out["entries"]), take(np.int32, out["entries"])
        out["a_val"], out["colptr"] = take(np.float64, out["a_total"]), take(np.int64, n + 1)
        if out["t_fmt"] == SELL:
            out["perm"], out["slice_ptr"] = take(np.int32, n), take(np.int64, out["t_slices"] + 1)
            out["long_row"], out["long_ptr"] = take(np.int32, out["t_long_rows"]), take(np.int64, out["t_long_rows"] + 1)
            out["seg_ptr"], out["seg_part"] = take(np.int64, out["t_long_segments"] + 1), take(np.int32, out["t_long_segments"])
            out["ref_slice_ptr"], out["ref_perm"] = take(np.int64, out["t_slices"] + 1), take(np.int32, n)
        assert at == len(raw)
        return out
    return run


def transposed_reference(indptr, indices, data, x):
    """A^T x and |A|^T |x| straight from the triplets, in long double"""
    rows = csr_rows(indptr)
    ref, mag = np.zeros(x.shape, LD), np.zeros(x.shape, LD)
    np.add.at(ref, indices, data.astype(LD)[:, None] * x.astype(LD)[rows])
    np.add.at(mag, indices, np.abs(data).astype(LD)[:, None] * np.abs(x).astype(LD)[rows])
    return ref, mag


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_index(out, n, indptr, indices, data, x, fmt_t):
    nnz = int(indptr[-1] - indptr[0])
    col_len = np.bincount(indices, minlength=n)
    rows = csr_rows(indptr)
    # ---- the product: the bound, the order contract, one writer per element
    ref, mag = transposed_reference(indptr, indices, data, x)
    assert_within(out["y"], ref, {"(len_j + 2) eps |A|^T|x|": (col_len[:, None] + 2) * EPS * mag, "tiny": LD(1e-300)}, f"index walk n={n}")
    assert same_bits(out["y"], out["z"]), "the index walk and the forward walk over the transposed arrays differ in bits"
    assert np.all(out["y"][col_len == 0] == 0.0) and not np.any(np.signbit(out["y"][col_len == 0]))
    assert np.array_equal(out["writes"], np.ones(n, np.int32)), "every element of the result has exactly one writer"
    # ---- the layout is that of the column lengths
    assert out["nnz"] == nnz and np.array_equal(np.diff(out["colptr"]), col_len) and out["colptr"][0] == 0
    want_fmt = fmt_t if fmt_t != AUTO else (ELL if col_len.max() * n <= 1.25 * nnz else SELL)
    assert out["t_fmt"] == want_fmt
    row, pos = out["row"], out["pos"]
    real = pos >= 0
    if out["t_fmt"] == ELL:
        assert out["t_w"] == col_len.max() and out["entries"] == out["t_w"] * n
        q, j = np.divmod(np.arange(out["entries"]), n)
        assert np.array_equal(real, q < col_len[j]), "padding follows a column's entries and is marked by position -1"
        owner = j
    else:
        assert np.array_equal(out["slice_ptr"], out["ref_slice_ptr"]) and np.array_equal(out["perm"], out["ref_perm"])
        is_long = col_len > LONG_ROW
        assert np.array_equal(np.sort(out["long_row"]), np.flatnonzero(is_long))
        assert np.array_equal(np.diff(out["long_ptr"]), col_len[out["long_row"]])
        assert out["t_long_entries"] == int(col_len[is_long].sum()) and out["entries"] == out["t_stored"] + out["t_long_entries"]
        assert out["t_long_segments"] == int(sum(-(-int(c) // SEG) for c in col_len[is_long]))
        assert out["t_multi_segments"] == int(sum(-(-int(c) // SEG) for c in col_len[is_long] if c > SEG))
        owner = np.zeros(out["entries"], np.int64)
        perm = out["perm"]
        for s in range(out["t_slices"]):
            b0, b1 = int(out["slice_ptr"][s]), int(out["slice_ptr"][s + 1])
            lanes = np.arange(b1 - b0) % SLICE
            slot = s * SLICE + lanes
            pj = np.where(slot < n, perm[np.minimum(slot, n - 1)], 0)
            j = np.where(pj < 0, ~pj, pj)
            asked = np.where((slot < n) & (pj >= 0), col_len[j], 0)
            assert np.array_equal(real[b0:b1], np.arange(b1 - b0) // SLICE < asked)
            owner[b0:b1] = j
        for r, j in enumerate(out["long_row"]):
            owner[out["t_stored"] + out["long_ptr"][r]:out["t_stored"] + out["long_ptr"][r + 1]] = j
        assert np.all(real[out["t_stored"]:]), "a tail holds no padding"
    # ---- every real entry of A is referenced exactly once, through the position of its value; padding points nowhere
    assert int(real.sum()) == nnz
    assert np.array_equal(np.sort(pos[real]), np.sort(stored_positions(out, n, indptr)))
    assert np.all(pos[~real] == -1) and np.all((row >= 0) & (row < n))
    got = sorted(zip(owner[real].tolist(), row[real].tolist(), out["a_val"][pos[real]].view(np.uint64).tolist()))
    want = sorted(zip(indices.tolist(), rows.tolist(), data.view(np.uint64).tolist()))
    assert got == want, "the index does not hold the triplets of A"
    return out


def stored_positions(out, n, indptr):
    """where A's layout keeps every entry, from the promises of include/diaglib_amd.h alone: ELLPACK q n + i; a sliced A is checked
    through its values (the test above) and through the tail lying behind `stored`"""
    lens = np.diff(indptr)
    if out["a_fmt"] == ELL:
        rows = csr_rows(indptr)
        q = np.arange(len(rows)) - (indptr[rows] - indptr[0])
        return q * n + rows
    in_tail = np.repeat(lens > LONG_ROW, lens)
    pos = out["pos"][out["pos"] >= 0]
    assert int((pos >= out["a_stored"]).sum()) == int(in_tail.sum()), "positions of A's tail entries lie behind `stored`"
    return pos


def dense_column_csr(rng, n, eighths=False):
    """short rows (1 .. 4 entries) that all hold column 3 as well: A is ELLPACK, its transpose needs a tail"""
    lens = rng.integers(1, 5, n)
    indptr, indices, data = csr_from_lengths(rng, n, lens, eighths)
    indices[indptr[:-1] + (rng.random(n) * lens).astype(np.int64)] = 3 % n
    return indptr, indices, data


def dense_row_csr(rng, n, eighths=False):
    """short rows and one row that holds every column once, in a shuffled order: its entries live in A's tail"""
    lens = rng.integers(0, 4, n)
    lens[n // 3] = n
    indptr, indices, data = csr_from_lengths(rng, n, lens, eighths)
    indices[indptr[n // 3]:indptr[n // 3 + 1]] = rng.permutation(n).astype(np.int32)
    return indptr, indices, data


def with_empty_column(indptr, indices, data, n, j):
    indices = indices.copy()
    indices[indices == j] = (j + 1) % n
    return indptr, indices, data


PAIRS = [(fa, ft) for fa in (ELL, SELL) for ft in (ELL, SELL)]


@pytest.mark.parametrize("fmt_a,fmt_t", PAIRS)
@pytest.mark.parametrize("n,w_max", [(1, 1), (63, 5), (64, 9), (65, 33), (257, 5), (1000, 17)])
def test_ragged_unsorted_matrix_with_duplicates(driver, n, w_max, fmt_a, fmt_t):
    rng = np.random.default_rng(1000 * n + w_max)
    indptr, indices, data = ragged_csr(rng, n, min(w_max, n))
    x = np.asfortranarray(rng.standard_normal((n, 3)))
    check_index(driver(n, indptr, indices, data, x, fmt_a, fmt_t), n, indptr, indices, data, x, fmt_t)


@pytest.mark.parametrize("fmt_a,fmt_t", PAIRS + [(AUTO, AUTO)])
def test_integer_data_is_exact(driver, fmt_a, fmt_t):
    n = 300
    rng = np.random.default_rng(7)
    indptr, indices, _ = ragged_csr(rng, n, 12)
    data = rng.integers(-8, 9, len(indices)).astype(np.float64)
    x = np.asfortranarray(rng.integers(-8, 9, (n, 2)).astype(np.float64))
    out = check_index(driver(n, indptr, indices, data, x, fmt_a, fmt_t), n, indptr, indices, data, x, fmt_t)
    want = np.zeros((n, 2))
    np.add.at(want, indices, data[:, None] * x[csr_rows(indptr)])
    assert np.array_equal(out["y"], want)


@pytest.mark.parametrize("fmt_a,fmt_t", PAIRS)
def test_an_empty_column_gives_plus_zero(driver, fmt_a, fmt_t):
    n = 130
    rng = np.random.default_rng(11)
    indptr, indices, data = with_empty_column(*ragged_csr(rng, n, 6), n, 77)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = check_index(driver(n, indptr, indices, data, x, fmt_a, fmt_t), n, indptr, indices, data, x, fmt_t)
    assert np.all(out["y"][77] == 0.0) and not np.any(np.signbit(out["y"][77]))


@pytest.mark.parametrize("fmt_t", [SELL, AUTO])
def test_one_dense_column_under_short_rows_gets_a_tail_although_a_is_ellpack(driver, fmt_t):
    n = 700
    rng = np.random.default_rng(12)
    indptr, indices, data = dense_column_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = check_index(driver(n, indptr, indices, data, x, ELL, fmt_t), n, indptr, indices, data, x, fmt_t)
    assert out["a_fmt"] == ELL and out["t_fmt"] == SELL
    assert list(out["long_row"]) == [3] and out["t_long_entries"] >= n and out["t_long_segments"] == 1


@pytest.mark.parametrize("fmt_t", [ELL, SELL, AUTO])
def test_one_dense_row_has_positions_behind_stored(driver, fmt_t):
    n = 700
    rng = np.random.default_rng(13)
    indptr, indices, data = dense_row_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = check_index(driver(n, indptr, indices, data, x, SELL, fmt_t), n, indptr, indices, data, x, fmt_t)
    assert out["a_fmt"] == SELL and out["a_total"] - out["a_stored"] == n
    assert int((out["pos"] >= out["a_stored"]).sum()) == n


def test_a_column_of_two_segments(driver):
    """n = 5000 with a column of more than 4096 entries: two segments, combined in order"""
    n = 5000
    rng = np.random.default_rng(14)
    indptr, indices, data = dense_column_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, 5)))
    out = check_index(driver(n, indptr, indices, data, x, AUTO, AUTO), n, indptr, indices, data, x, AUTO)
    assert out["t_fmt"] == SELL and out["t_long_segments"] == 2 and out["t_multi_segments"] == 2
    assert np.array_equal(out["seg_part"], [0, 1]) and np.array_equal(np.diff(out["seg_ptr"]), [SEG, out["t_long_entries"] - SEG])


def test_refusals(driver):
    n = 6
    rp, ci, va, x = np.array([0, 1, 2, 3, 3, 3, 3], np.int64), np.zeros(3, np.int32), np.ones(3), np.ones((n, 1), order="F")
    for fmt_t in (3, -1):
        out = driver(n, rp, ci, va, x, ELL, fmt_t)
        assert out["status"] == ERR_ARG and "spmm_transpose_prepare: unknown format" in out["message"], out
    for fmt_t in (ELL, SELL, AUTO):
        assert driver(n, rp, ci, va, x, ELL, fmt_t)["status"] == 0
