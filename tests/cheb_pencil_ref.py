"""Test helper: the reference of the Chebyshev preconditioner on the scaled pencil A + fac B (include/diaglib_amd.h,
dla_spmm_precnd_cheb_pencil) and its bound.  Scalars, banded matrices and the teeth condition are those of tests/cheb_ref.py; the
per-row sums and the diffusion matrix those of tests/cheb_jacobi_ref.py.

metric_band()  a banded positive definite metric: diagonal 1 + 0.25 sin^2(0.003 i), off-diagonals k = 1 .. hb of (0.1 / k) cos(0.01 i + k),
               mirrored.  The off-diagonal row sums stay below 0.69 for hb <= 17, the diagonal is at least 1.
mass()         the five-point pattern of diffusion(order, .): diagonal rho(i, j) = 1 + 0.5 sin(0.7 i) cos(1.1 j), each edge carries
               + (harmonic mean of its two rho) / 10; a harmonic mean of rho and its neighbour is below 2 rho, so the off-diagonal
               row sums are at most 0.8 rho: positive definite.
scaling()      (den0, s, den) of the contract in float64 or long double; in float64 den0 = a_ii + fac * b_ii has the contract's bits
               (numpy rounds the product and the sum each on its own).
upper()        (hi, slack): hi = max_i (s_i + offA_i + |fac| offB_i) / den_i in long double, and what a float64 evaluation may differ
               by: (lenA_i + lenB_i + 5) u (sum |a_p| + |fac| sum |b_p|) / den_i to first order -- the additions of the two off sums
               and of the stored diagonals, the product and the sum of den0, s + offA, the fused multiply-add and the division --
               which also covers diagonals that are cancelling sums.  slack is the maximum of that over the rows.
reference()    the recurrence of the contract in long double (y = x o r, z_1 = y / theta, z_{k+1} = z_k + a (z_k - z_{k-1})
               + b (y - r o (A z_k + fac B z_k))) and beside it the first-order running bound of a float64 evaluation, u = 2^-53:
                 E_0 = 0,  E_y = 2 u |y|,  E_1 = 3 u |z_1|,
                 E_{k+1} = (1 + a) E_k + a E_{k-1} + b (E_y + r (|A| E_k + |fac| |B| E_k))
                           + u (lenA_i + lenB_i + 12) (|z_k| + a (|z_k| + |z_{k-1}|) + b (|y| + r (|A||z_k| + |fac||B||z_k|)))
               The tolerance on px is 2 E_d element by element, and a case counts only while cheb_ref.assert_bound_has_teeth holds.
float64()      the same recurrence in plain float64 numpy; fac_b: what B is multiplied by in the product (a seeded error uses -fac).
oracle_counts()  the oracle's gen_davidson and lobpcg_gen on (diffusion(32, 1e3), mass(32)) with numpy callbacks, once per kind."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import cheb_jacobi_ref
import cheb_ref
import spmm_cases

LD = np.longdouble
U = cheb_ref.U
GUARD = 1e-5
ORDER, CONTRAST = 32, 1e3
SOLVE = dict(cheb_ref.SOLVE, max_iter=150)
N, F = 777, 0.02

diffusion = cheb_jacobi_ref.diffusion


def metric_band(n, hb):
    i = np.arange(n, dtype=np.float64)
    diags, offs = [1.0 + 0.25 * np.sin(0.003 * i) ** 2], [0]
    for k in range(1, hb + 1):
        v = (0.1 / k) * np.cos(0.01 * i[:n - k] + k)
        diags += [v, v]; offs += [k, -k]
    return sp.diags(diags, offs, shape=(n, n), format="csr")


def mass(order):
    i, j = np.meshgrid(np.arange(order), np.arange(order), indexing="ij")
    rho = 1.0 + 0.5 * np.sin(0.7 * i) * np.cos(1.1 * j)
    idx = i * order + j
    n = order * order
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [rho.ravel()]
    for di, dj in ((1, 0), (0, 1)):
        r1, r2 = rho[:order - di, :order - dj], rho[di:, dj:]
        w = (2.0 * r1 * r2 / (r1 + r2)).ravel() / 10.0
        p, q = idx[:order - di, :order - dj].ravel(), idx[di:, dj:].ravel()
        rows += [p, q]; cols += [q, p]; vals += [w, w]
    b = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    b.sort_indices()
    return b


GUARD_FAC = -(float(cheb_ref.banded(N, 6).diagonal()[77]) / float(metric_band(N, 2).diagonal()[77]))


def scaling(diag_a, diag_b, fac):
    """(den0, s, den) of the contract in the type of the diagonals"""
    den0 = diag_a + fac * diag_b
    s = np.abs(den0)
    return den0, s, np.where(s > GUARD, s, np.ones_like(s))


def upper(csr_a, csr_b, fac):
    """(hi, slack) in long double"""
    da, offa, tota, lna = cheb_jacobi_ref.rows(*csr_a)
    db, offb, totb, lnb = cheb_jacobi_ref.rows(*csr_b)
    fac = LD(fac)
    _, s, den = scaling(da, db, fac)
    return ((s + offa + abs(fac) * offb) / den).max(), ((lna + lnb + 5) * LD(U) * (tota + abs(fac) * totb) / den).max()


def reference(csr_a, csr_b, x, hi, fac, d, lo_fraction):
    """(z_d, E_d) in long double; hi: the upper end the interval is built on"""
    n = csr_a[0]
    ra, va = cheb_ref._rows(n, csr_a[1]), csr_a[3].astype(LD)
    rb, vb = cheb_ref._rows(n, csr_b[1]), csr_b[3].astype(LD)
    ia, ib = csr_a[2], csr_b[2]
    ava, avb = np.abs(va), np.abs(vb)
    da, _, _, lna = cheb_jacobi_ref.rows(*csr_a)
    db, _, _, lnb = cheb_jacobi_ref.rows(*csr_b)
    x, fac, u, hi = x.astype(LD), LD(fac), LD(U), LD(hi)
    if hi <= GUARD:
        return x, np.zeros_like(x)
    r = (1 / scaling(da, db, fac)[2])[:, None]
    ln = (lna + lnb + 12)[:, None]
    theta, delta, rho = cheb_ref.scalars(hi, LD(lo_fraction) * hi, d)
    y = x * r
    ey = 2 * u * np.abs(y)
    z0, z1 = np.zeros_like(x), y / theta
    e0, e1 = np.zeros_like(x), 3 * u * np.abs(z1)
    spmm = cheb_ref._spmm
    af = abs(fac)
    for k in range(1, d):
        a, b = rho[k] * rho[k - 1], 2 * rho[k] / delta
        z2 = z1 + a * (z1 - z0) + b * (y - r * (spmm(n, ra, ia, va, z1) + fac * spmm(n, rb, ib, vb, z1)))
        absz = spmm(n, ra, ia, ava, np.abs(z1)) + af * spmm(n, rb, ib, avb, np.abs(z1))
        e2 = ((1 + a) * e1 + a * e0 + b * (ey + r * (spmm(n, ra, ia, ava, e1) + af * spmm(n, rb, ib, avb, e1)))
              + u * ln * (np.abs(z1) + a * (np.abs(z1) + np.abs(z0)) + b * (np.abs(y) + r * absz)))
        z0, z1, e0, e1 = z1, z2, e1, e2
    return z1, e1


def float64(a, b, x, hi, fac, d, lo_fraction, fac_b=None):
    """the recurrence in float64 on scipy matrices; fac_b: the factor of B in the product where it is not fac (a seeded error)"""
    if hi <= GUARD:
        return x.copy()
    fac_b = fac if fac_b is None else fac_b
    r = (1.0 / scaling(a.diagonal(), b.diagonal(), fac)[2])[:, None]
    theta, delta, rho = cheb_ref.scalars(hi, lo_fraction * hi, d, np.float64)
    y = x * r
    z0, z1 = np.zeros_like(x), y / theta
    for k in range(1, d):
        a_, b_ = rho[k] * rho[k - 1], 2.0 * rho[k] / delta
        z0, z1 = z1, z1 + a_ * (z1 - z0) + b_ * (y - r * (a @ z1 + fac_b * (b @ z1)))
    return z1


# ---- the cases of tests/test_cheb_pencil_ref.py and tests/test_spmm_cheb_pencil_gpu.py: (hbA, hbB, m, d, fac) with A = banded(N, hbA)
# and B = metric_band(N, hbB).  The pairs cover every rung of the pair ladder 4 / 8 / 16 / streaming by max(wA, wB), and B wider than A.
# d = 8 only with fac >= 0 (negative fac exceeds the teeth cap there); the row that hits the guard exactly; rows with den0 < 0.
BAND_CASES = [(1, 1, 1, 8, 0.0), (3, 6, 3, 8, 0.5), (6, 2, 8, 8, 0.5), (12, 12, 13, 8, 0.0), (12, 6, 5, 8, 0.0), (17, 3, 3, 8, 0.5),
              (3, 17, 13, 8, 0.5),
              (6, 6, 13, 3, -1.25), (1, 3, 8, 2, -1.25), (17, 17, 8, 1, -1.25),
              (6, 2, 5, 3, GUARD_FAC),
              (3, 6, 8, 3, -3.0), (17, 1, 13, 2, -3.0)]
# the sliced and mixed cases at n = 5000: (A, B) by name, each with these (m, d, fac)
BIG_PAIRS = [("skewed", "metric3"), ("banded6", "skewed"), ("skewed", "skewed")]
BIG_RUNS = [(5, 8, 0.5), (9, 3, -0.7)]


def panel(n, m, seed=3):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((n, m)))


def band_pair(hba, hbb):
    return cheb_ref.banded(N, hba), metric_band(N, hbb)


def big_matrix(name):
    """raw CSR of one of the n = 5000 matrices (the skewed one has unsorted columns, duplicates and a dense row)"""
    if name == "skewed":
        return (5000,) + tuple(spmm_cases.skewed_csr(np.random.default_rng(7), 5000))
    return cheb_ref.raw({"metric3": lambda: metric_band(5000, 3), "banded6": lambda: cheb_ref.banded(5000, 6)}[name]())


def as_scipy(csr):
    n, indptr, indices, data = csr
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


def oracle_counts(oracle, which):
    """(ok, iterations, eigenvalues) of the oracle's gen_davidson and lobpcg_gen on (diffusion(32, 1e3), mass(32)) with numpy callbacks,
    from cheb_ref.guess: which = "pencil" (the float64 recurrence above on the long-double hi of each fac) or "diag"
    (x / (a_ii + fac b_ii) under the harness' guard).  SOLVE with its cap of 150 iterations."""
    if which in _COUNTS:
        return _COUNTS[which]
    a, b = diffusion(ORDER, CONTRAST), mass(ORDER)
    csr_a, csr_b = cheb_ref.raw(a), cheb_ref.raw(b)
    n = a.shape[0]
    da, db = a.diagonal(), b.diagonal()
    s = SOLVE
    c_dp, c_ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def product(mat):
        def h(pn, pm, px, pax):
            k = pm[0]
            np.ctypeslib.as_array(pax, (k, n)).T[:, :] = mat @ np.ctypeslib.as_array(px, (k, n)).T
        return h

    def h_pc(pn, pm, pf, px, ppx):
        k = pm[0]
        x = np.asfortranarray(np.ctypeslib.as_array(px, (k, n)).T)
        if which == "pencil":
            out = float64(a, b, x, float(upper(csr_a, csr_b, pf[0])[0]), pf[0], s["steps"], s["lo_fraction"])
        else:
            den = da + pf[0] * db
            out = np.where(np.abs(den)[:, None] > GUARD, x / den[:, None], x)
        np.ctypeslib.as_array(ppx, (k, n)).T[:, :] = out

    mvt = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp)
    cmv, cbv = mvt(product(a)), mvt(product(b))
    cpc = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)(h_pc)
    amv, abv, apc = (C.cast(f, C.c_void_p).value for f in (cmv, cbv, cpc))
    g0 = cheb_ref.guess(n, s["n_max"])
    ed, _, okd, trd = oracle.gen_davidson(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], s["max_dav"], 0.0, amv, apc, abv, g0)
    el, _, okl, trl = oracle.lobpcg_gen(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], 0.0, amv, apc, abv, g0)
    _COUNTS[which] = {"davidson": (okd, int(trd.iters), ed[:s["n_targ"]].copy()), "lobpcg": (okl, int(trl.iters), el[:s["n_targ"]].copy())}
    return _COUNTS[which]


_COUNTS = {}
