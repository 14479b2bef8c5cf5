"""CPU: the reference the GPU tests hold the diagonally scaled Chebyshev preconditioner against (tests/cheb_jacobi_ref.py; the
contract: include/diaglib_amd.h, dla_spmm_precnd_cheb_jacobi).

1. Plain float64 stays inside the bound 2 E_d on banded(777, 3).
2. The bound has teeth: one rho_k off by a relative 1e-6 falls outside, for every k.
3. The reference is the Chebyshev polynomial of the scaled operator: on a diagonal matrix D^-1 M = I, so the residual of
   p(D^-1 M) D^-1 is T_d((theta - 1) / delta) / T_d(sigma) in every row, whatever the diagonal.
4. What the scaled form is for: the oracle's Davidson and LOBPCG on diffusion(32, 1e3) converge with it in fewer iterations than
   with the plain polynomial, and do not converge within 150 with the diagonal preconditioner (measured: 46 / 41 against 90 / 83)."""
import numpy as np
import pytest

import cheb_jacobi_ref as ref
import cheb_ref

LD = np.longdouble
F = 0.02


def _banded_case():
    a = cheb_ref.banded(777, 3)
    x = np.asfortranarray(np.random.default_rng(11).standard_normal((777, 3)))
    return a, cheb_ref.raw(a), x


def test_diffusion_matrix():
    a = ref.diffusion(4, 100.0)
    d = a.toarray()
    assert np.array_equal(d, d.T) and a.shape == (16, 16)
    kap = lambda i, j: 100.0 ** (0.5 + 0.5 * np.sin(1.3 * i) * np.cos(0.9 * j))
    w = lambda p, q: 2.0 * kap(*p) * kap(*q) / (kap(*p) + kap(*q))
    assert d[1 * 4 + 2, 2 * 4 + 2] == -w((1, 2), (2, 2)) and d[1 * 4 + 2, 1 * 4 + 3] == -w((1, 2), (1, 3)) and d[0, 5] == 0.0
    # an interior row sums to zero up to rounding, a corner row keeps two Dirichlet terms
    assert abs(d[5].sum()) <= 1e-12 * d[5, 5] and abs(d[0].sum() - 2.0 * kap(0, 0)) <= 1e-12 * d[0, 0]
    assert np.linalg.eigvalsh(d)[0] > 0.0
    assert (np.diff(ref.diffusion(32, 1e3).indptr) == 5).sum() == 30 * 30


@pytest.mark.parametrize("fac,d", [(0.0, 8), (0.5, 8), (-1.25, 3)])
def test_plain_float64_stays_inside_the_bound(fac, d):
    a, csr, x = _banded_case()
    hi = float(ref.upper(*csr, fac)[0])
    z, e = ref.reference(*csr, x, hi, fac, d, F)
    teeth = cheb_ref.assert_bound_has_teeth(z, e)
    got = ref.float64(a, x, hi, fac, d, F)
    share = float((np.abs(got.astype(LD) - z) / (2 * e)).max())
    print("fac %+.2f, d = %d: float64 uses %.3f of the tolerance (2 E_d / |z_d| = %.1e)" % (fac, d, share, teeth))
    assert share <= 1.0, (fac, share)


def test_the_bound_has_teeth():
    """one rho_k off by a relative 1e-6 must not pass"""
    a, csr, x = _banded_case()
    hi = float(ref.upper(*csr, 0.0)[0])
    z, e = ref.reference(*csr, x, hi, 0.0, 8, F)
    cheb_ref.assert_bound_has_teeth(z, e)
    for k in range(1, 8):
        got = ref.float64(a, x, hi, 0.0, 8, F, rho_off=(k, 1e-6))
        assert np.any(np.abs(got.astype(LD) - z) > 2 * e), k


def test_upper_bounds_the_scaled_spectrum():
    a, csr, _ = _banded_case()
    for fac in (0.0, 0.5, -1.25, -3.0):
        hi, slack = ref.upper(*csr, fac)
        m = a.toarray() + fac * np.eye(777)
        s, den = ref.scaling(np.diag(m).copy(), 0.0)
        assert hi >= np.abs(np.linalg.eigvals(m / den[:, None])).max()
        assert 0 < slack < 1e-13 * hi


@pytest.mark.parametrize("hi", [1.0, 1.3, 2.0])
@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_reference_is_the_chebyshev_polynomial_of_the_scaled_operator(d, hi):
    """hi = 1 is the bound itself (the scaled spectrum sits on the interval's upper end); a larger hi puts it inside"""
    n, fac = 200, 0.25
    lam = np.linspace(0.5, 800.0, n)
    indptr, indices = np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32)
    assert ref.upper(n, indptr, indices, lam, fac)[0] == LD(1)
    q, _ = ref.reference(n, indptr, indices, lam, np.ones((n, 1)), hi, fac, d, F)
    res = 1 - (lam.astype(LD) + LD(fac)) * q[:, 0]
    theta, delta, _ = cheb_ref.scalars(LD(hi), LD(F) * LD(hi), 1)
    t = lambda v: np.cos(d * np.arccos(v)) if abs(v) <= 1 else np.cosh(d * np.arccosh(v))
    want = t(max((theta - 1) / delta, LD(-1))) / t(theta / delta)
    assert np.abs(res - want).max() <= 1e-12 * max(abs(want), LD(1e-3)), (float(res[0]), float(want))
    if hi == 1.0:
        assert abs(abs(want) * t(theta / delta) - 1) <= 1e-12


def test_iteration_counts_from_the_oracle(oracle):
    scaled, plain, diag = (ref.oracle_counts(oracle, w) for w in ("scaled", "plain", "diag"))
    want = np.linalg.eigvalsh(ref.diffusion(ref.ORDER, ref.CONTRAST).toarray())[:ref.SOLVE["n_targ"]]
    print("oracle iterations, scaled:", {k: v[1] for k, v in scaled.items()}, "plain:", {k: (v[0], v[1]) for k, v in plain.items()},
          "diagonal:", {k: (v[0], v[1]) for k, v in diag.items()})
    for driver in ("davidson", "lobpcg"):
        ok, iters, eig = scaled[driver]
        assert ok and iters <= ref.SOLVE["max_iter"], (driver, ok, iters)
        assert np.abs(eig - want).max() <= 1e-7 * want.max(), (driver, eig, want)
        assert iters < plain[driver][1], (driver, iters, plain[driver])
        assert not diag[driver][0], (driver, diag[driver])
