"""Test helper: the reference of the Chebyshev polynomial preconditioner (include/diaglib_amd.h, dla_spmm_precnd_cheb) and its bound.

reference()  the three-term recurrence of the contract in np.longdouble on raw CSR arrays (unsorted columns and duplicates as they
             come), the sparse product entry by entry in long double, and beside it the first-order running error bound E_k of a
             float64 evaluation (u = 2^-53, E_0 = 0, E_1 = u |z_1|):
               E_{k+1} = (1 + a) E_k + a E_{k-1} + b (|A| E_k + |fac| E_k)
                         + u (len_i + 8) (|z_k| + a (|z_k| + |z_{k-1}|) + b (|x| + |A||z_k| + |fac||z_k|))
             with a = rho_k rho_{k-1}, b = 2 rho_k / delta and len_i the entries of row i.  The tolerance on px is 2 E_d element by
             element: the factor 2 covers the second-order terms and the rounding of the host-side coefficients.  The bound grows
             by about 6x per step, so a case is only bound-checked while max(2 E_d) / max|z_d| <= 1e-9 (assert_bound_has_teeth).
float64()    the same recurrence in plain float64 numpy (what the oracle's numpy callback applies, and what the teeth test perturbs).
The matrices of the tests: the banded matrix of tests/test_spmm_sharded.py and its ragged variant, spmm_cases.skewed_csr, and the
five-point Laplacian on 32 x 32 plus 0.05 cos(0.37 i) on the diagonal."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
TEETH = 1e-9
LAPLACE_ORDER = 32
SOLVE = dict(n_targ=4, n_max=6, max_dav=10, tol=1e-8, max_iter=60, steps=8, lo_fraction=0.02)


def banded(n, half_band, ragged=False):
    """diagonal 2 + i / 50, off-diagonals 0.3 / d cos(i + d), d = 1 .. half_band; ragged: (r, r + d) is present iff
    d <= 1 + (r mod half_band), mirrored, and the zeros are dropped, so the rows really are of different lengths"""
    i = np.arange(n, dtype=np.float64)
    diags, offs = [2.0 + i / 50.0], [0]
    for d in range(1, half_band + 1):
        v = 0.3 / d * np.cos(i[:n - d] + d)
        if ragged:
            v = np.where(d <= 1 + (np.arange(n - d) % half_band), v, 0.0)
        diags += [v, v]; offs += [d, -d]
    a = sp.diags(diags, offs, shape=(n, n), format="csr")
    a.eliminate_zeros()
    return a


def laplacian(order=LAPLACE_ORDER):
    t = sp.diags([-np.ones(order - 1), 2.0 * np.ones(order), -np.ones(order - 1)], [-1, 0, 1])
    eye = sp.identity(order)
    n = order * order
    return (sp.kron(eye, t) + sp.kron(t, eye) + sp.diags(0.05 * np.cos(0.37 * np.arange(n)))).tocsr()


def raw(a):
    a = a.tocsr()
    return a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)


def guess(n, n_max):
    """evec[i, j] = [i = 7 j] + 1e-3 cos(0.7 (i + 1)(j + 1))"""
    i, j = np.meshgrid(np.arange(n), np.arange(n_max), indexing="ij")
    return np.asfortranarray((i == 7 * j) + 1e-3 * np.cos(0.7 * (i + 1.0) * (j + 1.0)))


def _rows(n, indptr):
    return np.repeat(np.arange(n), np.diff(indptr))


def gershgorin(n, indptr, indices, data):
    """(g, slack) in long double: g = max_i diag[i] + sum_{col != i} |v|, and the tolerance of the contract on a float64
    evaluation, (maxlen + 2) u max_i sum |v_p|"""
    rows, v = _rows(n, indptr), data.astype(LD)
    on = indices == rows
    diag, off, tot = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    np.add.at(diag, rows[on], v[on])
    np.add.at(off, rows[~on], np.abs(v[~on]))
    np.add.at(tot, rows, np.abs(v))
    return (diag + off).max(), (int(np.diff(indptr).max()) + 2) * LD(U) * tot.max()


def _spmm(n, rows, indices, v, z):
    out = np.zeros((n, z.shape[1]), v.dtype)
    np.add.at(out, rows, v[:, None] * z[indices])
    return out


def scalars(hi, lo, d, dtype=LD):
    """theta, delta and rho_0 .. rho_{d-1}"""
    hi, lo = dtype(hi), dtype(lo)
    theta, delta = (hi + lo) / 2, (hi - lo) / 2
    sigma = theta / delta
    rho = [1 / sigma]
    for _ in range(1, d):
        rho.append(1 / (2 * sigma - rho[-1]))
    return theta, delta, rho


def reference(n, indptr, indices, data, x, g, fac, d, lo_fraction):
    """(z_d, E_d) in long double; g: the upper bound the interval is built on"""
    rows, v = _rows(n, indptr), data.astype(LD)
    av = np.abs(v)
    ln = (np.diff(indptr).astype(LD) + 8)[:, None]
    x, fac, u = x.astype(LD), LD(fac), LD(U)
    hi = LD(g) + fac
    theta, delta, rho = scalars(hi, LD(lo_fraction) * hi, d)
    z0, z1 = np.zeros_like(x), x / theta
    e0, e1 = np.zeros_like(x), u * np.abs(z1)
    for k in range(1, d):
        a, b = rho[k] * rho[k - 1], 2 * rho[k] / delta
        z2 = z1 + a * (z1 - z0) + b * (x - (_spmm(n, rows, indices, v, z1) + fac * z1))
        absz = _spmm(n, rows, indices, av, np.abs(z1))
        e2 = ((1 + a) * e1 + a * e0 + b * (_spmm(n, rows, indices, av, e1) + abs(fac) * e1)
              + u * ln * (np.abs(z1) + a * (np.abs(z1) + np.abs(z0)) + b * (np.abs(x) + absz + abs(fac) * np.abs(z1))))
        z0, z1, e0, e1 = z1, z2, e1, e2
    return z1, e1


def assert_bound_has_teeth(z, e):
    ratio = float((2 * e).max() / np.abs(z).max())
    assert ratio <= TEETH, ratio
    return ratio


def float64(a, x, g, fac, d, lo_fraction, rho_off=None):
    """the recurrence in float64 on a scipy matrix; rho_off = (k, rel): rho_k is off by the relative rel"""
    hi = g + fac
    if hi <= 1e-5:
        return x.copy()
    theta, delta, rho = scalars(hi, lo_fraction * hi, d, np.float64)
    if rho_off is not None:
        rho[rho_off[0]] *= 1.0 + rho_off[1]
    z0, z1 = np.zeros_like(x), x / theta
    for k in range(1, d):
        a_, b_ = rho[k] * rho[k - 1], 2.0 * rho[k] / delta
        z0, z1 = z1, z1 + a_ * (z1 - z0) + b_ * (x - (a @ z1 + fac * z1))
    return z1


def oracle_counts(oracle, which):
    """(ok, iterations, eigenvalues) of the oracle's Davidson and LOBPCG on the Laplacian with numpy callbacks, from the guess above:
    which = "cheb" (8 steps, lo_fraction 0.02, the float64 recurrence on the long-double Gershgorin bound) or "diag".  Computed once."""
    if which in _COUNTS:
        return _COUNTS[which]
    a = laplacian()
    n = a.shape[0]
    diag = a.diagonal()
    g = float(gershgorin(*raw(a))[0])
    s = SOLVE
    c_dp, c_ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

    def h_mv(pn, pm, px, pax):
        k = pm[0]
        np.ctypeslib.as_array(pax, (k, n)).T[:, :] = a @ np.ctypeslib.as_array(px, (k, n)).T

    def h_pc(pn, pm, pf, px, ppx):
        k = pm[0]
        x = np.asfortranarray(np.ctypeslib.as_array(px, (k, n)).T)
        if which == "cheb":
            out = float64(a, x, g, pf[0], s["steps"], s["lo_fraction"])
        else:
            den = diag + pf[0]
            out = np.where(np.abs(den)[:, None] > 1e-5, x / den[:, None], x)
        np.ctypeslib.as_array(ppx, (k, n)).T[:, :] = out

    cmv = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp)(h_mv)
    cpc = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)(h_pc)
    amv, apc = C.cast(cmv, C.c_void_p).value, C.cast(cpc, C.c_void_p).value
    g0 = guess(n, s["n_max"])
    ed, _, okd, trd = oracle.davidson(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], s["max_dav"], 0.0, amv, apc, g0)
    el, _, okl, trl = oracle.lobpcg(n, s["n_targ"], s["n_max"], s["max_iter"], s["tol"], 0.0, amv, apc, g0)
    _COUNTS[which] = {"davidson": (okd, int(trd.iters), ed[:s["n_targ"]].copy()), "lobpcg": (okl, int(trl.iters), el[:s["n_targ"]].copy())}
    return _COUNTS[which]


_COUNTS = {}
