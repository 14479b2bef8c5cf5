"""CPU: the reference the GPU tests hold the Chebyshev preconditioner on the scaled pencil against (tests/cheb_pencil_ref.py; the
contract: include/diaglib_amd.h, dla_spmm_precnd_cheb_pencil).

1. On every case the GPU file uses the teeth cap holds and plain float64 stays inside the bound 2 E_d.
2. The bound rejects two seeded errors: fac applied to B with the wrong sign, and B replaced by the identity.
3. The two test metrics are what their descriptions say (symmetric, positive definite, the stated row sums), the guard case hits
   den0 == 0.0 exactly, and fac = -3 leaves 51 rows with den0 < 0.
4. With B the identity the reference is that of the scaled form, and upper() bounds the scaled pencil's spectrum.
5. What the pencil form is for: the oracle's gen_davidson and lobpcg_gen on (diffusion(32, 1e3), mass(32)) converge with it, and do
   not converge within 150 iterations with x / (a_ii + fac b_ii) (measured: 47 / 36)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cheb_jacobi_ref
import cheb_pencil_ref as ref
import cheb_ref

LD = np.longdouble
F = ref.F


def _share(got, z, e):
    return float((np.abs(got.astype(LD) - z) / (2 * e)).max())


def _check(a, b, csr_a, csr_b, x, fac, d, seeded):
    hi = float(ref.upper(csr_a, csr_b, fac)[0])
    z, e = ref.reference(csr_a, csr_b, x, hi, fac, d, F)
    teeth = cheb_ref.assert_bound_has_teeth(z, e)
    share = _share(ref.float64(a, b, x, hi, fac, d, F), z, e)
    print("d = %d, m = %d, fac = %+.3f: float64 uses %.3f of the tolerance (2 E_d / |z_d| = %.1e)" % (d, x.shape[1], fac, share, teeth))
    assert share <= 1.0, share
    if seeded and d > 1 and fac != 0.0:
        n = a.shape[0]
        wrong_sign = _share(ref.float64(a, b, x, hi, fac, d, F, fac_b=-fac), z, e)
        identity = _share(ref.float64(a, sp.identity(n, format="csr"), x, hi, fac, d, F), z, e)
        print("   seeded errors: wrong sign %.1e, B = I %.1e times the tolerance" % (wrong_sign, identity))
        # (measured: 1e8 .. 3e9 times the tolerance on the banded cases; what is asserted is that both fall outside, by a wide margin)
        assert wrong_sign > 1e3 and identity > 1e3, (wrong_sign, identity)
    return teeth


@pytest.mark.parametrize("hba,hbb,m,d,fac", ref.BAND_CASES)
def test_band_cases_have_teeth_and_float64_stays_inside(hba, hbb, m, d, fac):
    a, b = ref.band_pair(hba, hbb)
    # (B = I as a seeded error is the scaling's error too, which a row at the guard turns into a division by nearly nothing)
    teeth = _check(a, b, cheb_ref.raw(a), cheb_ref.raw(b), ref.panel(ref.N, m), fac, d, seeded=fac != ref.GUARD_FAC)
    assert teeth <= (7.3e-10 if d == 8 else 5e-13) * 1.05, teeth


@pytest.mark.parametrize("m,d,fac", ref.BIG_RUNS)
@pytest.mark.parametrize("pair", ref.BIG_PAIRS)
def test_sliced_cases_have_teeth_and_float64_stays_inside(pair, m, d, fac):
    csr_a, csr_b = ref.big_matrix(pair[0]), ref.big_matrix(pair[1])
    teeth = _check(ref.as_scipy(csr_a), ref.as_scipy(csr_b), csr_a, csr_b, ref.panel(5000, m), fac, d, seeded=False)
    assert teeth <= 1.3e-11 * 1.05, teeth


def test_diffusion_mass_case_has_teeth():
    a, b = ref.diffusion(ref.ORDER, ref.CONTRAST), ref.mass(ref.ORDER)
    _check(a, b, cheb_ref.raw(a), cheb_ref.raw(b), ref.panel(a.shape[0], 5), -0.3, 8, seeded=True)


def test_the_metrics():
    for hb in (1, 3, 17):
        b = ref.metric_band(ref.N, hb).toarray()
        assert np.array_equal(b, b.T)
        assert (np.abs(b).sum(1) - np.diag(b)).max() < 0.69 and np.diag(b).min() >= 1.0
        assert b[5, 5] == 1.0 + 0.25 * np.sin(0.003 * 5) ** 2 and b[5, 6] == 0.1 * np.cos(0.01 * 5 + 1)
        if hb >= 3:
            assert b[5, 8] == (0.1 / 3) * np.cos(0.01 * 5 + 3)
    m, d = ref.mass(ref.ORDER), ref.diffusion(ref.ORDER, ref.CONTRAST)
    assert np.array_equal(m.indptr, d.indptr) and np.array_equal(m.indices, d.indices)
    mm = m.toarray()
    rho = lambda i, j: 1.0 + 0.5 * np.sin(0.7 * i) * np.cos(1.1 * j)
    assert np.array_equal(mm, mm.T) and mm[32 + 2, 32 + 2] == rho(1, 2)
    assert mm[1 * 32 + 2, 2 * 32 + 2] == 2.0 * rho(1, 2) * rho(2, 2) / (rho(1, 2) + rho(2, 2)) / 10.0
    assert np.all(mm.sum(1) - np.diag(mm) <= 0.8 * np.diag(mm))
    assert np.linalg.eigvalsh(mm)[0] > 0.0


def test_the_guard_and_the_negative_rows():
    a, b = ref.band_pair(6, 2)
    den0 = ref.scaling(a.diagonal(), b.diagonal(), ref.GUARD_FAC)[0]
    assert den0[77] == 0.0 and (np.abs(den0) <= ref.GUARD).sum() == 1
    for hba, hbb in ((3, 6), (17, 1)):
        a, b = ref.band_pair(hba, hbb)
        assert (ref.scaling(a.diagonal(), b.diagonal(), -3.0)[0] < 0).sum() == 51


def test_identity_metric_is_the_scaled_form():
    a = cheb_ref.banded(ref.N, 3)
    csr_a, csr_i = cheb_ref.raw(a), cheb_ref.raw(sp.identity(ref.N, format="csr"))
    x = ref.panel(ref.N, 3)
    for fac, d in ((0.5, 8), (-1.25, 3)):
        hi = ref.upper(csr_a, csr_i, fac)[0]
        assert hi == cheb_jacobi_ref.upper(*csr_a, fac)[0]
        z, e = ref.reference(csr_a, csr_i, x, float(hi), fac, d, F)
        zj, ej = cheb_jacobi_ref.reference(*csr_a, x, float(hi), fac, d, F)
        assert np.abs(z - zj).max() <= 1e-17 * np.abs(zj).max() and np.all(e >= ej)


def test_upper_bounds_the_scaled_spectrum():
    for hba, hbb, fac in ((3, 6, 0.5), (6, 2, -1.25), (17, 17, -3.0), (3, 17, 0.0)):
        a, b = ref.band_pair(hba, hbb)
        hi, slack = ref.upper(cheb_ref.raw(a), cheb_ref.raw(b), fac)
        m = a.toarray() + fac * b.toarray()
        den = ref.scaling(np.diag(m).copy(), np.zeros(ref.N), 0.0)[2]
        assert hi >= np.abs(np.linalg.eigvals(m / den[:, None])).max()
        assert 0 < slack < 1e-13 * hi


def test_iteration_counts_from_the_oracle(oracle):
    import scipy.linalg
    pencil, diag = (ref.oracle_counts(oracle, w) for w in ("pencil", "diag"))
    t = ref.SOLVE["n_targ"]
    want = scipy.linalg.eigh(ref.diffusion(ref.ORDER, ref.CONTRAST).toarray(), ref.mass(ref.ORDER).toarray(), eigvals_only=True)[:t]
    print("oracle iterations, pencil:", {k: v[1] for k, v in pencil.items()}, "diagonal:", {k: (v[0], v[1]) for k, v in diag.items()})
    for driver, measured in (("davidson", 47), ("lobpcg", 36)):
        ok, iters, eig = pencil[driver]
        assert ok and iters <= ref.SOLVE["max_iter"], (driver, ok, iters)
        assert np.abs(eig - want).max() <= 1e-7 * want.max(), (driver, eig, want)
        assert abs(iters - measured) <= max(1, measured // 5), (driver, iters)
        assert not diag[driver][0], (driver, diag[driver])
