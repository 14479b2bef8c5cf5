"""Test helper: the reference of the diagonally scaled Chebyshev preconditioner (include/diaglib_amd.h, dla_spmm_precnd_cheb_jacobi)
and its bound.  The scalars, the banded matrices and the teeth condition are those of tests/cheb_ref.py.

rows()       diag, off and len per row of raw CSR arrays in np.longdouble (duplicates summed as they come).
upper()      (hi, slack): hi = max_i (s_i + off_i) / den_i in long double, and what a float64 evaluation may differ by.  A float64
             q_i is len_i - 1 additions for off_i and the stored diagonal, one rounding each for diag + fac, s + off and the
             division: at most (len_i + 3) u (sum_p |v_p| + |fac|) / den_i to first order, which also covers a diagonal that is a
             cancelling sum of duplicates.  slack is the maximum of that over the rows.
reference()  the recurrence of the contract in long double (y = x o r, z_1 = y / theta, z_{k+1} = z_k + a (z_k - z_{k-1})
             + b (y - r o (A z_k + fac z_k))) and beside it the first-order running bound of a float64 evaluation, u = 2^-53:
               E_0 = 0,  E_y = 2 u |y|,  E_1 = 3 u |z_1|,
               E_{k+1} = (1 + a) E_k + a E_{k-1} + b (E_y + r (|A| E_k + |fac| E_k))
                         + u (len_i + 10) (|z_k| + a (|z_k| + |z_{k-1}|) + b (|y| + r (|A||z_k| + |fac||z_k|)))
             The tolerance on px is 2 E_d element by element, and a case is bound-checked only while
             max(2 E_d) / max|z_d| <= cheb_ref.TEETH (cheb_ref.assert_bound_has_teeth).
float64()    the same recurrence in plain float64 numpy; rho_off = (k, rel) perturbs rho_k.
diffusion()  the five-point -div(kappa grad) with a coefficient of the given contrast.
oracle_counts()  the oracle's Davidson and LOBPCG on diffusion(32, 1e3) with numpy callbacks, computed once per kind."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import cheb_ref

LD = np.longdouble
U = cheb_ref.U
GUARD = 1e-5
ORDER, CONTRAST = 32, 1e3
SOLVE = dict(cheb_ref.SOLVE, max_iter=150)


def diffusion(order, contrast):
    """five-point -div(kappa grad) on an order x order grid, row i * order + j, kappa(i, j) = contrast ** (0.5 + 0.5 sin(1.3 i) cos(0.9 j));
    the weight of an edge is the harmonic mean 2 k1 k2 / (k1 + k2), entered as -w off the diagonal; the diagonal is the sum of the
    row's weights plus kappa(i, j) per missing neighbour (Dirichlet)"""
    i, j = np.meshgrid(np.arange(order), np.arange(order), indexing="ij")
    kap = float(contrast) ** (0.5 + 0.5 * np.sin(1.3 * i) * np.cos(0.9 * j))
    idx = i * order + j
    n = order * order
    diag = np.zeros(n)
    rows, cols, vals = [], [], []
    for di, dj in ((1, 0), (0, 1)):
        k1, k2 = kap[:order - di, :order - dj], kap[di:, dj:]
        w = (2.0 * k1 * k2 / (k1 + k2)).ravel()
        p, q = idx[:order - di, :order - dj].ravel(), idx[di:, dj:].ravel()
        rows += [p, q]; cols += [q, p]; vals += [-w, -w]
        np.add.at(diag, p, w)
        np.add.at(diag, q, w)
    missing = (i == 0).astype(int) + (i == order - 1) + (j == 0) + (j == order - 1)
    diag += (missing * kap).ravel()
    rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(diag)
    a = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def rows(n, indptr, indices, data):
    """(diag, off, tot, len) per row in long double: the sum of the (i, i) entries, of |v| off the diagonal, of every |v|, and the
    number of entries"""
    r, v = cheb_ref._rows(n, indptr), data.astype(LD)
    on = indices == r
    diag, off, tot = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(diag, r[on], v[on])
    np.add.at(off, r[~on], np.abs(v[~on]))
    np.add.at(tot, r, np.abs(v))
    return diag, off, tot, np.diff(indptr).astype(LD)


def scaling(diag, fac):
    """(s, den) of the contract in the type of diag"""
    s = np.abs(diag + fac)
    return s, np.where(s > GUARD, s, np.ones_like(s))


def upper(n, indptr, indices, data, fac):
    """(hi, slack) in long double"""
    diag, off, tot, ln = rows(n, indptr, indices, data)
    s, den = scaling(diag, LD(fac))
    return ((s + off) / den).max(), ((ln + 3) * LD(U) * (tot + abs(LD(fac))) / den).max()


def reference(n, indptr, indices, data, x, hi, fac, d, lo_fraction):
    """(z_d, E_d) in long double; hi: the upper end the interval is built on"""
    r_, v = cheb_ref._rows(n, indptr), data.astype(LD)
    av = np.abs(v)
    diag, _, _, ln = rows(n, indptr, indices, data)
    x, fac, u, hi = x.astype(LD), LD(fac), LD(U), LD(hi)
    if hi <= GUARD:
        return x, np.zeros_like(x)
    r = (1 / scaling(diag, fac)[1])[:, None]
    ln = (ln + 10)[:, None]
    theta, delta, rho = cheb_ref.scalars(hi, LD(lo_fraction) * hi, d)
    y = x * r
    ey = 2 * u * np.abs(y)
    z0, z1 = np.zeros_like(x), y / theta
    e0, e1 = np.zeros_like(x), 3 * u * np.abs(z1)
    spmm = cheb_ref._spmm
    for k in range(1, d):
        a, b = rho[k] * rho[k - 1], 2 * rho[k] / delta
        z2 = z1 + a * (z1 - z0) + b * (y - r * (spmm(n, r_, indices, v, z1) + fac * z1))
        absz = spmm(n, r_, indices, av, np.abs(z1))
        e2 = ((1 + a) * e1 + a * e0 + b * (ey + r * (spmm(n, r_, indices, av, e1) + abs(fac) * e1))
              + u * ln * (np.abs(z1) + a * (np.abs(z1) + np.abs(z0)) + b * (np.abs(y) + r * (absz + abs(fac) * np.abs(z1)))))
        z0, z1, e0, e1 = z1, z2, e1, e2
    return z1, e1


def float64(a, x, hi, fac, d, lo_fraction, rho_off=None):
    """the recurrence in float64 on a scipy matrix; rho_off = (k, rel): rho_k is off by the relative rel"""
    if hi <= GUARD:
        return x.copy()
    r = (1.0 / scaling(a.diagonal(), fac)[1])[:, None]
    theta, delta, rho = cheb_ref.scalars(hi, lo_fraction * hi, d, np.float64)
    if rho_off is not None:
        rho[rho_off[0]] *= 1.0 + rho_off[1]
    y = x * r
    z0, z1 = np.zeros_like(x), y / theta
    for k in range(1, d):
        a_, b_ = rho[k] * rho[k - 1], 2.0 * rho[k] / delta
        z0, z1 = z1, z1 + a_ * (z1 - z0) + b_ * (y - r * (a @ z1 + fac * z1))
    return z1


def oracle_counts(oracle, which):
    """(ok, iterations, eigenvalues) of the oracle's Davidson and LOBPCG on diffusion(32, 1e3) with numpy callbacks, from
    cheb_ref.guess: which = "scaled" (the float64 recurrence above on the long-double hi of each fac), "plain" (cheb_ref.float64 on
    the long-double Gershgorin bound) or "diag" (x / (a_ii + fac) under the harness' guard).  SOLVE with its cap of 150 iterations."""
    if which in _COUNTS:
        return _COUNTS[which]
    a = diffusion(ORDER, CONTRAST)
    csr = cheb_ref.raw(a)
    n = a.shape[0]
    diag = a.diagonal()
    g = float(cheb_ref.gershgorin(*csr)[0])
    s = SOLVE
    c_dp, c_ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def h_mv(pn, pm, px, pax):
        k = pm[0]
        np.ctypeslib.as_array(pax, (k, n)).T[:, :] = a @ np.ctypeslib.as_array(px, (k, n)).T

    def h_pc(pn, pm, pf, px, ppx):
        k = pm[0]
        x = np.asfortranarray(np.ctypeslib.as_array(px, (k, n)).T)
        if which == "scaled":
            out = float64(a, x, float(upper(*csr, pf[0])[0]), pf[0], s["steps"], s["lo_fraction"])
        elif which == "plain":
            out = cheb_ref.float64(a, x, g, pf[0], s["steps"], s["lo_fraction"])
        else:
            den = diag + pf[0]
            out = np.where(np.abs(den)[:, None] > GUARD, x / den[:, None], x)
        np.ctypeslib.as_array(ppx, (k, n)).T[:, :] = out

    cmv = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp)(h_mv)
    cpc = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)(h_pc)
    amv, apc = C.cast(cmv, C.c_void_p).value, C.cast(cpc, C.c_void_p).value
    g0 = cheb_ref.guess(n, s["n_max"])
    ed, _, okd, trd = oracle.davidson(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], s["max_dav"], 0.0, amv, apc, g0)
    el, _, okl, trl = oracle.lobpcg(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], 0.0, amv, apc, g0)
    _COUNTS[which] = {"davidson": (okd, int(trd.iters), ed[:s["n_targ"]].copy()), "lobpcg": (okl, int(trl.iters), el[:s["n_targ"]].copy())}
    return _COUNTS[which]


_COUNTS = {}
