"""Test helper: sparse linear-response pencils (A B; B A)(Y Z) = w (S D; -D -S)(Y Z) handed over as the four parts A+B, A-B, S+D,
S-D (tests/test_spmm_lr_gpu.py, tests/test_fortran_sparse_lr_caller_gpu.py), their dense solution, the harness' lrprec_1 / lrprec_2
in numpy with the order of operations lr_precnd_kernel fixes, and the host-callback solve that sets the tolerance of the device
solves."""
import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp

from diaglib_amd import capi

PARTS = ("apb", "amb", "spd", "smd")
MUL = {p: f"dla_spmm_{p}mul" for p in PARTS}


def _pairs(rng, n, per_row, size):
    """strictly upper-triangular U with `per_row` random entries per row where the row allows it (distinct pairs, |u| <= size)"""
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.integers(0, n, rows.size)
    keep = rows != cols
    lo, hi = np.minimum(rows, cols)[keep], np.maximum(rows, cols)[keep]
    key = np.unique(lo.astype(np.int64) * n + hi)
    return sp.csr_matrix((rng.uniform(-size, size, key.size), (key // n, key % n)), shape=(n, n))


def random_pencil(n, seed=11):
    """apb = diag(i + 5) + E, amb = diag(i + 2) + 0.2 E (i = 1 .. n; E symmetric, about 6 off-diagonal entries per row, |e| <= 0.05);
    S = diag(1 + 0.5 / (1 + i mod 7)) + 0.01 E', D antisymmetric with entries <= 0.02.  Diagonally dominant by a wide margin: the
    off-diagonal row sums of E stay below about 20 x 0.05 = 1 against diagonals >= 3, those of 0.01 E' below 0.01 against >= 1.06
    (positive_definite() checks it with eigvalsh all the same)."""
    rng = np.random.default_rng(seed)
    i = np.arange(1.0, n + 1.0)
    u = _pairs(rng, n, 3, 0.05)
    e = u + u.T
    u = _pairs(rng, n, 3, 0.05)
    e2 = u + u.T
    u = _pairs(rng, n, 3, 0.02)
    d = u - u.T
    s = sp.diags(1.0 + 0.5 / (1.0 + (np.arange(1, n + 1) % 7))) + 0.01 * e2
    mats = {"apb": sp.diags(i + 5.0) + e, "amb": sp.diags(i + 2.0) + 0.2 * e, "spd": s + d, "smd": s - d}
    return {k: v.tocsr() for k, v in mats.items()}


def positive_definite(mats):
    """A + B, A - B and S = ((S+D) + (S-D)) / 2 are symmetric positive definite, D = ((S+D) - (S-D)) / 2 is antisymmetric"""
    apb, amb, spd, smd = (mats[p].toarray() for p in PARTS)
    s, d = 0.5 * (spd + smd), 0.5 * (spd - smd)
    sym = all(np.array_equal(x, x.T) for x in (apb, amb)) and np.abs(s - s.T).max() < 1e-15 and np.abs(d + d.T).max() < 1e-15
    return sym and all(np.linalg.eigvalsh(0.5 * (x + x.T)).min() > 0 for x in (apb, amb, s))


def dense_roots(mats, t):
    """the t lowest positive eigenvalues of the 2n x 2n pencil, by scipy.linalg.eig"""
    apb, amb, spd, smd = (mats[p].toarray() for p in PARTS)
    a, b, s, d = 0.5 * (apb + amb), 0.5 * (apb - amb), 0.5 * (spd + smd), 0.5 * (spd - smd)
    big = np.block([[a, b], [b, a]])
    met = np.block([[s, d], [-d, -s]])
    w = sl.eig(big, met, right=False)
    assert np.abs(w.imag).max() <= 1e-9 * np.abs(w.real).max()
    w = np.sort(w.real)
    return w[w > 0][:t]


def lrprec_numpy(variant, fac, d_apb, d_amb, d_spd, xp, xm):
    """lr_precnd_kernel's expression with its order of operations: every product, sum and quotient rounded on its own, products left
    to right (numpy's elementwise operations do not fuse)"""
    fac = float(fac)
    aa = 0.5 * (d_apb + d_amb)
    sg = d_spd
    if variant == 1:
        den = -1.0 / (aa * aa - fac * fac * sg * sg)
        ca, cs = aa, fac * sg
    else:
        den = 1.0 / (fac * fac * aa * aa - sg * sg)
        ca, cs = fac * aa, sg
    den, ca, cs = den[:, None], ca[:, None], cs[:, None]
    return den * (ca * xp + cs * xm), den * (ca * xm + cs * xp)


def unit_guess(n, m):
    g = np.zeros((2 * n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    return g


def solve_host_mode(ctx, mats, trad, t, m, max_iter, tol, max_dav, guess=None):
    """the driver in host-callback mode: scipy products and the numpy lrprec on blocks staged through host memory"""
    n = mats["apb"].shape[0]
    da, dm, ds = (mats[p].diagonal() for p in ("apb", "amb", "spd"))
    mv = [(lambda x, a=mats[p]: a @ x) for p in PARTS]
    variant = 1 if trad else 2
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    solve = ctx.caslr_driver if trad else ctx.caslr_eff_driver
    eig, _, ok, info = solve(n, t, m, max_iter, tol, max_dav, *mv, lambda fac, xp, xm: lrprec_numpy(variant, fac, da, dm, ds, xp, xm),
                             unit_guess(n, m) if guess is None else guess)
    return eig[:t], ok, info


def solve_device_mode(ctx, mats, trad, t, m, max_iter, tol, max_dav, fmt="ell", guess=None):
    """the same solve on the sparse parts in HBM: dla_spmm_apbmul .. dla_spmm_smdmul and dla_spmm_lrprec1 / 2 as device callbacks"""
    n = mats["apb"].shape[0]
    for p in PARTS:
        ctx.spmm_setup_lr(p, mats[p], fmt=fmt)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    try:
        fns = [capi.fn_address(MUL[p]) for p in PARTS] + [capi.fn_address("dla_spmm_lrprec1" if trad else "dla_spmm_lrprec2")]
        ev = ctx.panel(unit_guess(n, m) if guess is None else guess)
        solve = ctx.caslr_driver if trad else ctx.caslr_eff_driver
        eig, _, ok, info = solve(n, t, m, max_iter, tol, max_dav, *fns, ev)
        vec = ev.download()
        ev.free()
    finally:
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    return eig[:t], ok, info, vec


def tolerance(host_eig, want):
    """ten times the relative error of the host-callback solve against the dense solve, never more than 1e-8"""
    host_err = float(np.abs(host_eig / want - 1.0).max())
    return host_err, min(10.0 * host_err, 1e-8)
