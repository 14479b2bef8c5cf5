"""CPU: dla_geev, the small general eigensolver behind nonsym_driver (diaglib_amd/csrc/smalldense.cpp; replaces dgeev('v','v') of
reference diaglib.f90:2499), against numpy / scipy (LAPACK) on the same matrices.

Residuals are assembled in complex arithmetic from dgeev's packed columns and held to 8 x LAPACK's own residual plus
n eps ||A||_F (other shifts, no balancing).  Measured ratios, this solver's residual over LAPACK's, right / left, the largest over the
sizes: random 1.03 / 1.20 from n = 3 on (2.21 / 0.99 at n = 2, where both residuals are one or two ulps), symmetric 1.64 / 1.41, companion
1.11 / 1.11 (2.83 / 0.50 at n = 2), rotations 1.07 / 1.07, the reduced matrices of a Davidson run 0.85 / 0.80.
"""
import numpy as np
import pytest
import scipy.linalg as sl

import nonsym_cases as nc
from diaglib_amd import capi

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 3, 5, 16, 40, 117]


def _matrix(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "random":
        return rng.standard_normal((n, n))
    if kind == "symmetric":
        s = rng.standard_normal((n, n))
        return s + s.T
    if kind == "companion":
        c = np.zeros((n, n))
        c[0, :] = rng.standard_normal(n)
        c[np.arange(1, n), np.arange(n - 1)] = 1.0
        return c
    assert kind == "rotations"          # 2 x 2 rotations by distinct angles: every eigenvalue complex (odd n: one 1 x 1 block more)
    r = np.zeros((n, n))
    for k in range(n // 2):
        th = 0.3 + 0.7 * k
        r[2 * k:2 * k + 2, 2 * k:2 * k + 2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    if n % 2:
        r[n - 1, n - 1] = 2.0
    return r


def _davidson_reduced():
    """V^T A V of every iteration of a plain block Davidson run (numpy) on the first non-symmetric test matrix"""
    n, n_targ, n_max, _, _, _, t = nc.CASES[2]
    a, _ = nc.matrix(n, t, *nc.factors(n))
    prec = nc.mprec(np.diag(a).copy())
    v = nc.guess(n, n_max)
    out = []
    for _ in range(8):
        h = v.T @ a @ v
        out.append(h)
        w, y = np.linalg.eig(h)
        keep = np.argsort(w.real)[:n_max]
        x = v @ y[:, keep].real
        res = a @ x - x * w[keep].real
        new = np.column_stack([prec(-w[keep[j]].real, res[:, j:j + 1]) for j in range(n_max)])
        new -= v @ (v.T @ new)
        new -= v @ (v.T @ new)
        v = np.column_stack([v, np.linalg.qr(new)[0]])
    return out


def _unpack(wi, v):
    """dgeev's packed eigenvector columns as a complex matrix"""
    n = len(wi)
    z = np.zeros((n, n), dtype=complex)
    j = 0
    while j < n:
        if wi[j] != 0.0:
            z[:, j] = v[:, j] + 1j * v[:, j + 1]
            z[:, j + 1] = v[:, j] - 1j * v[:, j + 1]
            j += 2
        else:
            z[:, j] = v[:, j]
            j += 1
    return z


def _check(a, label):
    n = a.shape[0]
    wr, wi, vl, vr = capi.geev(a)
    lam = wr + 1j * wi
    right, left = _unpack(wi, vr), _unpack(wi, vl)
    w_ref, l_ref, r_ref = sl.eig(a, left=True, right=True)
    w_np, r_np = np.linalg.eig(a)
    fro = np.linalg.norm(a)
    res_r = np.linalg.norm(a @ right - right * lam)
    res_l = np.linalg.norm(a.T @ left - left * lam.conj())
    ref_r = np.linalg.norm(a @ r_np - r_np * w_np)
    ref_l = np.linalg.norm(a.T @ l_ref - l_ref * w_ref.conj())
    print(f"{label} n={n}: right {res_r:.2e} (LAPACK {ref_r:.2e}), left {res_l:.2e} (LAPACK {ref_l:.2e})")
    assert res_r <= 8 * ref_r + n * EPS * fro
    assert res_l <= 8 * ref_l + n * EPS * fro
    # eigenvalues as multisets: each within 100 n eps ||A||_2 / |u^H v| of its partner, u, v LAPACK's unit vectors of that partner
    cond = np.abs(np.sum(l_ref.conj() * r_ref, axis=0))
    two = np.linalg.norm(a, 2)
    free = list(range(n))
    for x in lam:
        k = min(free, key=lambda q: abs(w_ref[q] - x))
        free.remove(k)
        assert abs(w_ref[k] - x) <= 100 * n * EPS * two / cond[k] + 1e-300, (x, w_ref[k], cond[k])
    # dgeev's conventions
    j = 0
    while j < n:
        if wi[j] != 0.0:
            assert wi[j] > 0.0 and wi[j + 1] == -wi[j] and wr[j + 1] == wr[j]
            j += 2
        else:
            j += 1
    for z in (right, left):
        assert np.abs(np.linalg.norm(z, axis=0) - 1.0).max() <= 8 * EPS
        big = z[np.argmax(np.abs(z), axis=0), np.arange(n)]
        assert np.all(big.imag == 0.0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["random", "symmetric", "companion", "rotations"])
def test_geev_against_lapack(kind, n):
    a = _matrix(kind, n)
    _check(a, kind)
    if kind == "rotations" and n >= 2:
        assert np.count_nonzero(capi.geev(a)[1]) == 2 * (n // 2)
    if kind == "symmetric":
        assert not np.any(capi.geev(a)[1])


def test_geev_on_the_reduced_matrices_of_a_davidson_run():
    for h in _davidson_reduced():
        _check(h, "davidson-reduced")


def test_geev_destroys_its_input_only_and_repeats_bit_for_bit():
    a = _matrix("random", 40)
    keep = a.copy()
    first = capi.geev(a)
    assert np.array_equal(a, keep)            # (the wrapper works on a copy)
    for x, y in zip(first, capi.geev(a)):
        assert np.array_equal(x, y)
    # a leading dimension larger than n, sentinels around the outputs
    L = capi.load()
    n, ld = 5, 9
    big = np.full((ld, n), np.nan, order="F")
    big[:n] = keep[:n, :n]
    wr, wi = np.zeros(n), np.zeros(n)
    vl, vr = np.full((ld, n), 7.0, order="F"), np.full((ld, n), 7.0, order="F")
    dp = capi._dp
    assert L.dla_geev(n, dp(big), ld, dp(wr), dp(wi), dp(vl), ld, dp(vr), ld) == 0
    assert np.all(vl[n:] == 7.0) and np.all(vr[n:] == 7.0) and np.all(np.isnan(big[n:]))
    ref = capi.geev(keep[:n, :n])
    assert np.array_equal(wr, ref[0]) and np.array_equal(vr[:n], ref[3]) and np.array_equal(vl[:n], ref[2])
    assert L.dla_geev(n, dp(big), n - 1, dp(wr), dp(wi), dp(vl), ld, dp(vr), ld) == -1
