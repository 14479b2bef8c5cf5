"""GPU: nonsym_driver in device mode on a SPARSE non-symmetric matrix stored once -- dla_spmm_matvec, dla_spmm_matvec_t (the
transposed product through the index of the same stored values) and dla_spmm_precnd as the three callbacks.

The matrix is that of examples/fortran_sparse_nonsym_caller: A = D S D^-1 with S symmetric and banded (s_ii = i + 1, s_ij = 1/(i + j)
for |i - j| in {1, 2, 17}, 1-based) and D = diag(exp(t_i)), t_i = 0.01 sin(1.3 i), so the eigenvalues are those of S and the
eigenvector matrix D Q has condition number at most e^0.02 (Bauer-Fike: eigenvalues within e^0.02 sqrt(n) tol for an rms residual
below tol, the argument of tests/test_fortran_nonsym_caller_gpu.py)."""
import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
N, N_TARG, N_MAX, MAX_DAV, TOL, MAX_ITER = 300, 4, 8, 10, 1e-9, 200


def example_matrix(n):
    """(A as csr, S dense)"""
    i = np.arange(1, n + 1)
    s = np.zeros((n, n))
    for off in (1, 2, 17):
        r = np.arange(n - off)
        s[r, r + off] = s[r + off, r] = 1.0 / (i[r] + i[r + off])
    np.fill_diagonal(s, i + 1.0)
    t = 0.01 * np.sin(1.3 * i)
    a = np.exp(t[:, None] - t[None, :]) * s
    return sp.csr_matrix(a), s


@pytest.fixture(scope="module")
def mats():
    a, s = example_matrix(N)
    return a, s, np.linalg.eigvalsh(s)[:N_TARG]


@pytest.fixture(autouse=True)
def _device_callbacks(ctx):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield
    ctx.spmm_drop_transpose()
    ctx.dense_drop(False)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.set_option(capi.OPT_EVEC_ON_DEVICE, 0)


def solve(ctx, names, side):
    g = np.zeros((N, N_MAX), order="F")
    g[np.arange(N_MAX), np.arange(N_MAX)] = 1.0
    mv, mvl, pc = (capi.fn_address(f) for f in names)
    eig, r, l, ok, info = ctx.nonsym_driver(N, N_TARG, N_MAX, MAX_ITER, TOL, MAX_DAV, 0.0, mv, mvl, pc, g.copy(order="F"), g.copy(order="F"), side)
    return eig, r, l, ok, info


SPARSE = ("dla_spmm_matvec", "dla_spmm_matvec_t", "dla_spmm_precnd")
DENSE = ("dla_dense_matvec", "dla_dense_matvec_t", "dla_dense_precnd")


@pytest.mark.parametrize("side", ["r", "l", "c"])
def test_sparse_callbacks_find_the_spectrum_of_s(ctx, mats, side):
    a, s, want = mats
    ctx.spmm_setup(a, "auto")
    ctx.spmm_transpose_prepare("auto")
    eig, r, l, ok, info = solve(ctx, SPARSE, side)
    assert ok and 0 < info["iters"] < MAX_ITER, info
    assert np.abs(eig[:N_TARG] - want).max() <= np.exp(0.02) * np.sqrt(N) * TOL, (eig[:N_TARG], want)
    if side == "c":
        assert np.abs(l.T @ r - np.eye(N_MAX)).max() <= N * np.finfo(float).eps
    # the same solve on the same matrix stored densely: the same algorithm on another order of summation, at most one block apart
    ctx.dense_setup(np.asfortranarray(a.toarray()))
    eig_d, _, _, ok_d, info_d = solve(ctx, DENSE, side)
    assert ok_d and abs(info["matvec_cols"] - info_d["matvec_cols"]) <= 8, (info, info_d)
    assert np.abs(eig_d[:N_TARG] - want).max() <= np.exp(0.02) * np.sqrt(N) * TOL
