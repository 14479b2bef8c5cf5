"""CPU: the host side of the Chebyshev polynomial preconditioner (include/diaglib_amd.h, dla_spmm_precnd_cheb) and the reference the
GPU tests hold the kernels against (tests/cheb_ref.py).

1. dla::cheb_coefficients, the function the HIP engine takes its per-step coefficients from, against the same scalars in long
   double.  tests/cheb_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
   tests/test_plans.py does).
2. The reference is the Chebyshev polynomial: on a diagonal matrix its residual 1 - lambda q_d(lambda) is bounded by 1 / T_d(sigma)
   on [lo, hi] and reaches that at lambda = lo.
3. The bound 2 E_d has teeth: a float64 recurrence with one rho_k off by a relative 1e-6 violates it.
4. What the preconditioner is for: the oracle's Davidson and LOBPCG on the 32 x 32 Laplacian reach tol 1e-8 within 60 iterations
   with it and do not with the diagonal preconditioner (measured: 15 / 17 iterations against 189 / 107)."""
import os
import subprocess

import numpy as np
import pytest

import cheb_ref
import hostsim

LD = np.longdouble
SRC = os.path.join(hostsim.ROOT, "tests", "cheb_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"), os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "cheb_driver")
INTERVALS = [(8.05, 0.161), (23.0, 0.46), (1.0, 0.999)]
DEGREES = [1, 2, 3, 8, 24]


def run_driver(requests):
    """per request (hi, lo, fac, d): (theta, delta, [(alpha, beta, gamma, eta)] * (d - 1)) as the product computes them"""
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    text = "".join("%s %s %s %d\n" % (float(hi).hex(), float(lo).hex(), float(fac).hex(), d) for hi, lo, fac, d in requests)
    p = subprocess.run([EXE], input=text, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    lines = iter(p.stdout.splitlines())
    out = []
    for _, _, _, d in requests:
        theta, delta = (float.fromhex(t) for t in next(lines).split())
        out.append((theta, delta, [tuple(float.fromhex(t) for t in next(lines).split()) for _ in range(d - 1)]))
    assert next(lines, None) is None
    return out


def coefficients_ld(hi, lo, fac, d):
    """the folded coefficients of dla::cheb_coefficients in long double, and per alpha its largest term"""
    theta, delta, rho = cheb_ref.scalars(hi, lo, d)
    fac = LD(fac)
    steps, terms = [], []
    for k in range(1, d):
        a, b = rho[k] * rho[k - 1], 2 * rho[k] / delta
        alpha, beta, gamma, eta = 1 + a - b * fac, -a, b, -b
        big = max(1 + a, abs(b * fac))
        if k == 1:
            alpha, eta, beta, big = alpha / theta, eta / theta, LD(0), big / theta
        if k == 2:
            beta = beta / theta
        steps.append((alpha, beta, gamma, eta)); terms.append(big)
    return theta, delta, steps, terms


def ulps(got, want, scale=None):
    """|got - want| in units in the last place of float64 at `scale` (default: at want)"""
    s = np.spacing(np.float64(abs(want if scale is None else scale)))
    return float(abs(LD(got) - want) / LD(s))


@pytest.mark.parametrize("fac", [0.0, 0.5, -1.25])
def test_coefficient_function_against_long_double(fac):
    """every coefficient within 8 ulp of its long-double value: each is a few roundings of exact scalars.  alpha = 1 + a - b fac is a
    sum, so its ulp is taken at its largest term (the two agree unless the terms cancel, which rounds the sum no better)"""
    requests = [(hi, lo, fac, d) for hi, lo in INTERVALS for d in DEGREES]
    worst = 0.0
    for (hi, lo, _, d), (theta, delta, steps) in zip(requests, run_driver(requests)):
        t_ld, d_ld, s_ld, terms = coefficients_ld(hi, lo, fac, d)
        assert len(steps) == d - 1
        errs = [ulps(theta, t_ld), ulps(delta, d_ld)]
        for got, want, big in zip(steps, s_ld, terms):
            errs.append(ulps(got[0], want[0], max(abs(want[0]), big)))
            errs += [ulps(g, w) for g, w in zip(got[1:], want[1:]) if w != 0]
            assert got[1] == 0.0 or want[1] != 0
        worst = max(worst, max(errs))
        assert max(errs) <= 8, (hi, lo, fac, d, errs)
    print("worst coefficient error: %.2f ulp" % worst)


@pytest.mark.parametrize("d", [1, 2, 3, 8])
def test_reference_is_the_chebyshev_polynomial(d):
    hi, f = 8.05, 0.02
    lam = np.linspace(f * hi, hi, 200)
    lam[-1] = hi
    n, indptr, indices, data = 200, np.arange(201, dtype=np.int64), np.arange(200, dtype=np.int32), lam
    g, _ = cheb_ref.gershgorin(n, indptr, indices, data)
    assert g == LD(hi)
    q, _ = cheb_ref.reference(n, indptr, indices, data, np.ones((n, 1)), g, 0.0, d, f)
    res = np.abs(1 - lam.astype(LD) * q[:, 0])
    theta, delta, _ = cheb_ref.scalars(LD(hi), LD(f) * LD(hi), 1)
    sigma = theta / delta
    t_d = np.cosh(d * np.arccosh(sigma))
    assert res.max() <= (1 + LD(1e-12)) / t_d, (float(res.max()), float(1 / t_d))
    assert res[0] >= (1 - LD(1e-12)) * res.max(), (int(res.argmax()), float(res[0]), float(res.max()))
    assert abs(res[0] * t_d - 1) <= 1e-12


def _banded_case():
    a = cheb_ref.banded(777, 3)
    x = np.asfortranarray(np.random.default_rng(11).standard_normal((777, 3)))
    g, _ = cheb_ref.gershgorin(*cheb_ref.raw(a))
    return a, x, float(g)


def test_plain_float64_stays_inside_the_bound():
    a, x, g = _banded_case()
    for fac in (0.0, -1.25, 0.5):
        z, e = cheb_ref.reference(*cheb_ref.raw(a), x, g, fac, 8, 0.02)
        cheb_ref.assert_bound_has_teeth(z, e)
        got = cheb_ref.float64(a, x, g, fac, 8, 0.02)
        share = float((np.abs(got.astype(LD) - z) / (2 * e)).max())
        print("fac %+.2f: float64 uses %.3f of the tolerance" % (fac, share))
        assert share <= 1.0, (fac, share)


def test_the_bound_has_teeth():
    """one rho_k off by a relative 1e-6 must not pass"""
    a, x, g = _banded_case()
    z, e = cheb_ref.reference(*cheb_ref.raw(a), x, g, 0.0, 8, 0.02)
    cheb_ref.assert_bound_has_teeth(z, e)
    for k in range(1, 8):
        got = cheb_ref.float64(a, x, g, 0.0, 8, 0.02, rho_off=(k, 1e-6))
        assert np.any(np.abs(got.astype(LD) - z) > 2 * e), k


def test_iteration_counts_from_the_oracle(oracle):
    cheb, diag = cheb_ref.oracle_counts(oracle, "cheb"), cheb_ref.oracle_counts(oracle, "diag")
    want = np.linalg.eigvalsh(cheb_ref.laplacian().toarray())[:cheb_ref.SOLVE["n_targ"]]
    print("oracle iterations:", {k: v[1] for k, v in cheb.items()}, "diagonal:", {k: (v[0], v[1]) for k, v in diag.items()})
    for driver in ("davidson", "lobpcg"):
        ok, iters, eig = cheb[driver]
        assert ok and iters <= cheb_ref.SOLVE["max_iter"], (driver, ok, iters)
        assert np.abs(eig - want).max() <= 1e-7, (driver, eig, want)
        assert not diag[driver][0], (driver, diag[driver])
