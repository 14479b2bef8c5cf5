"""CPU: the sliced-ELLPACK layout of the sparse operator (dla::sell_build and the setup checks in diaglib_amd/csrc/dla_internal.h).

tests/sell_layout_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_owned_buffers.py does): it checks and builds the layout with the product's own code, multiplies by walking the
structure the way the two kernels do and writes what it saw.  Here the product is compared with the raw triplets, and the
structure with what include/diaglib_amd.h promises: a permutation inside windows, widths that follow the sorted rows, a tail
that starts one entry above the threshold, storage that follows the non-zeros."""
import os
import subprocess

import numpy as np
import pytest

import hostsim
from spmm_cases import LONG_ROW, SLICE, WINDOW, csr_from_lengths, skewed_csr
from test_operators_gpu import EPS, LD, assert_within, csr_diagonal, csr_product_reference, ragged_csr

SRC = os.path.join(hostsim.ROOT, "tests", "sell_layout_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"), os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "sell_layout_driver")
ERR_ARG = 3
ELL, SELL, AUTO = 0, 1, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("sell")

    def run(n, indptr, indices, data, x, fmt=SELL):
        m = x.shape[1]
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        with open(fin, "wb") as f:
            np.array([n, m, len(indices), fmt], np.int64).tofile(f)
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
        names = ("n", "m", "slices", "stored", "long_entries", "long_rows", "nnz", "C", "sigma", "long_row_threshold", "auto")
        out = dict(zip(names, (int(v) for v in take(np.int64, 11))), status=0)
        assert (out["n"], out["m"]) == (n, m)
        out["ax"] = take(np.float64, n * m).reshape(m, n).T
        out["diag"], out["writes"], out["perm"] = take(np.float64, n), take(np.int32, n), take(np.int32, n)
        out["slice_ptr"] = take(np.int64, out["slices"] + 1)
        out["long_row"], out["long_ptr"] = take(np.int32, out["long_rows"]), take(np.int64, out["long_rows"] + 1)
        assert at == len(raw)
        return out
    return run


def check_layout(out, n, indptr, indices, data, x):
    lens = np.diff(indptr)
    assert (out["C"], out["sigma"], out["long_row_threshold"]) == (SLICE, WINDOW, LONG_ROW)
    # ---- the product and the diagonal, from the triplets
    ref, mag = csr_product_reference(indptr, indices, data, x)
    assert_within(out["ax"], ref, {"(len + 2) eps |A||x|": (lens[:, None] + 2) * EPS * mag, "tiny": LD(1e-300)}, f"layout walk n={n}")
    assert np.all(out["ax"][lens == 0] == 0.0)
    d = csr_diagonal(indptr, indices, data)
    assert_within(out["diag"][:, None], d.astype(LD)[:, None], {"len eps |d|": (lens[:, None] + 2) * EPS * csr_diagonal(indptr, indices, np.abs(data))[:, None],
                                                               "tiny": LD(1e-300)}, f"diag n={n}")
    assert np.array_equal(out["writes"], np.ones(n, np.int32)), "every row is produced exactly once"
    # ---- perm: a permutation that keeps every row inside its window; tail rows are marked
    perm = out["perm"]
    rows = np.where(perm < 0, ~perm, perm)
    assert np.array_equal(np.sort(rows), np.arange(n))
    assert np.array_equal(rows // WINDOW, np.arange(n) // WINDOW), "a row left its sorting window"
    is_long = lens > LONG_ROW
    assert np.array_equal(perm < 0, is_long[rows])
    assert np.array_equal(np.sort(out["long_row"]), np.flatnonzero(is_long)) and out["long_rows"] == int(is_long.sum())
    assert np.array_equal(np.diff(out["long_ptr"]), lens[out["long_row"]]) and out["long_entries"] == int(lens[is_long].sum())
    # ---- widths: every slice as wide as its longest row that is not in the tail, non-increasing inside a window
    asked = np.where(is_long, 0, lens)[rows]
    assert out["slices"] == -(-n // SLICE)
    width = np.diff(out["slice_ptr"]) // SLICE
    assert np.array_equal(np.diff(out["slice_ptr"]) % SLICE, np.zeros(out["slices"], np.int64))
    want = np.array([asked[s * SLICE:(s + 1) * SLICE].max() for s in range(out["slices"])])
    assert np.array_equal(width, want)
    for w0 in range(0, n, WINDOW):
        a = asked[w0:w0 + WINDOW]
        assert np.all(np.diff(a) <= 0), "rows are not sorted by descending length inside a window"
        assert np.all(np.diff(width[w0 // SLICE:(w0 + WINDOW) // SLICE]) <= 0)
        # stable: equal lengths keep the caller's order
        r = rows[w0:w0 + WINDOW]
        assert np.all((np.diff(a) < 0) | (np.diff(r) > 0))
    assert out["stored"] == int(out["slice_ptr"][-1]) == int(width.sum()) * SLICE
    assert out["nnz"] == int(indptr[-1] - indptr[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4095, 4096, 4097, 20000])
def test_skewed_matrix_walks_to_the_product_of_the_triplets(driver, n):
    rng = np.random.default_rng(100 + n)
    indptr, indices, data = skewed_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, 3)))
    out = driver(n, indptr, indices, data, x)
    check_layout(out, n, indptr, indices, data, x)
    if n > LONG_ROW + 1:
        assert out["long_rows"] >= 2              # the dense row and the row of LONG_ROW + 1 entries


@pytest.mark.parametrize("n,w_max", [(257, 5), (1000, 33), (5000, 70)])
def test_ragged_matrix_without_long_rows(driver, n, w_max):
    rng = np.random.default_rng(n)
    indptr, indices, data = ragged_csr(rng, n, w_max)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = driver(n, indptr, indices, data, x)
    check_layout(out, n, indptr, indices, data, x)
    assert out["long_rows"] == 0 and out["long_entries"] == 0


def test_only_long_rows(driver):
    n = 300
    rng = np.random.default_rng(5)
    indptr, indices, data = csr_from_lengths(rng, n, rng.integers(LONG_ROW + 1, n + 1, n))
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = driver(n, indptr, indices, data, x)
    check_layout(out, n, indptr, indices, data, x)
    assert out["long_rows"] == n and out["stored"] == 0


def test_threshold_row_is_in_a_slice_and_one_more_is_in_the_tail(driver):
    n = 400
    rng = np.random.default_rng(6)
    lens = np.full(n, 2)
    lens[17], lens[300] = LONG_ROW, LONG_ROW + 1
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    x = np.asfortranarray(rng.standard_normal((n, 1)))
    out = driver(n, indptr, indices, data, x)
    check_layout(out, n, indptr, indices, data, x)
    assert list(out["long_row"]) == [300]
    assert out["perm"][0] == 17                                  # the longest row that stays sorts first
    assert int(np.diff(out["slice_ptr"])[0]) == LONG_ROW * SLICE
    assert out["perm"][n - 1] == ~300                            # the tail row asks nothing of its slice: it sorts last
    assert out["stored"] == (LONG_ROW + 2 * (out["slices"] - 1)) * SLICE


@pytest.mark.parametrize("n", [4097, 20000])
@pytest.mark.parametrize("seed", [7, 8, 9])
def test_storage_follows_the_nonzeros(driver, n, seed):
    """the condition tests/test_spmm_formats_gpu.py asks of dla_spmm_info, on the builder alone"""
    rng = np.random.default_rng(seed)
    indptr, indices, data = skewed_csr(rng, n)
    out = driver(n, indptr, indices, data, np.zeros((n, 1), order="F"), fmt=AUTO)
    nnz = int(indptr[-1])
    ratio = (out["stored"] + out["long_entries"]) / nnz
    print(f"n={n} seed={seed}: (stored + long_entries) / nnz = {ratio:.3f}; ELLPACK would need {n * n / nnz:.0f} x nnz")
    assert ratio <= 1.25
    assert out["auto"] == SELL


def test_auto_keeps_ellpack_for_a_stencil(driver):
    import scipy.sparse as sp
    g = 40
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(g, g))
    a = (sp.kron(sp.identity(g), t) + sp.kron(t, sp.identity(g))).tocsr()
    n = g * g
    out = driver(n, a.indptr, a.indices, a.data, np.ones((n, 1), order="F"), fmt=AUTO)
    assert out["auto"] == ELL


def test_setup_refusals(driver):
    n = 6
    idx, val, x = np.zeros(8, np.int32), np.ones(8), np.ones((n, 1), order="F")
    ok = np.array([0, 1, 2, 3, 3, 3, 3], np.int64)
    bad = [("descending row pointers", np.array([0, 3, 2, 5, 5, 5, 5], np.int64), idx, SELL, "row pointers not ascending"),
           ("column index n", ok, np.array([0, n, 1, 0, 0, 0, 0, 0], np.int32), SELL, "column index out of range"),
           ("column index -1", ok, np.array([0, 1, -1, 0, 0, 0, 0, 0], np.int32), SELL, "column index out of range"),
           ("no entries at all", np.zeros(n + 1, np.int64), idx, SELL, "empty"),
           ("unknown format", ok, idx, 3, "unknown format"), ("unknown format", ok, idx, -1, "unknown format")]
    for what, rp, ci, fmt, msg in bad:
        out = driver(n, rp, ci, val, x, fmt=fmt)
        assert out["status"] == ERR_ARG and msg in out["message"], (what, out)
    for fmt in (ELL, SELL, AUTO):
        assert driver(n, ok, idx, val, x, fmt=fmt)["status"] == 0
