"""Test helper: the skewed matrices of the storage-format tests (tests/test_sell_layout.py, tests/test_spmm_formats_gpu.py) and of
tools/tune_spmm_format.py -- power-law row lengths with one dense row, the kind of matrix plain ELLPACK cannot hold."""
import numpy as np

# diaglib_amd/csrc/dla_internal.h: SELL_C, SELL_SIGMA, SELL_LONG_ROW (the CPU test checks them against what the builder reports)
SLICE, WINDOW, LONG_ROW = 64, 4096, 256


def skewed_lengths(rng, n):
    """row lengths min(n, int(3 (1 + pareto(1.2)))), then -- on distinct rows, as far as n allows -- exactly one row of length n,
    one empty row, one row of LONG_ROW and one of LONG_ROW + 1 entries (the last slice row and the first tail row)"""
    lens = np.minimum(n, (3.0 * (1.0 + rng.pareto(1.2, n))).astype(np.int64))
    if n > 1:
        lens = np.minimum(lens, n - 1)                     # (exactly one row of length n)
    special = [n, 0] + [w for w in (LONG_ROW, LONG_ROW + 1) if w < n]
    rows = rng.choice(n, min(n, len(special)), replace=False)
    for r, w in zip(rows, special):
        lens[r] = w
    return lens


def csr_from_lengths(rng, n, lens, eighths=False):
    """raw CSR arrays (indptr int64, indices int32, data float64): uniform unsorted columns (duplicates as they fall), about 5 %
    explicit zeros, standard-normal values (eighths: multiples of 1/8, |v| <= 5, so that any order of summation is exact)"""
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    cols = rng.integers(0, n, nnz).astype(np.int32)
    data = rng.integers(-40, 41, nnz) / 8.0 if eighths else rng.standard_normal(nnz)
    data[rng.random(nnz) < 0.05] = 0.0
    return indptr, np.ascontiguousarray(cols), np.ascontiguousarray(data, dtype=np.float64)


def skewed_csr(rng, n, eighths=False):
    return csr_from_lengths(rng, n, skewed_lengths(rng, n), eighths)


def fma(a, b, c):
    """a b + c rounded once: float(Fraction(a) * Fraction(b) + Fraction(c)) without the gcd -- the three as exact ratios over powers
    of two, and int / int rounds correctly (test_the_emulation_rounds_once of
    tests/test_spmm_long_rows_gpu.py compares the two)"""
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    d = da * db
    if dc > d:
        return (na * nb * (dc // d) + nc) / dc
    return (na * nb + nc * (d // dc)) / d
