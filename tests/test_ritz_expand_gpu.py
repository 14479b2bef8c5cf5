"""GPU: the Ritz sweep that also forms and measures the next Davidson block (davidson_expand_kernel behind dla_ritz_expand) against numpy in
long double.

One call forms R = AV Y - (V Y) Lambda with its norms, stores U0 = R(:, first:) / (d + fac) by the library's diagonal rule behind the
basis, and leaves [V | U0]^T U0 for the orthogonalisation chain.  Held here:

  a. R and the norms within the dot-product bound (2 m + 2) eps (|AV||Y| + |V||Y Lambda|), elementwise; columns of locked roots and
     columns behind n_res stay uncorrected (AV Y alone) and have no norm; R is also dla_ritz_residual's, bit for bit (the same
     products and correction, step by step), and the norms are its norms to the rounding of another order of summation
  b. the stored U0 is EXACTLY where(|d + fac| > 1e-5, R_stored / (d + fac), R_stored) -- rows under the threshold, and one at it, included
  c. the reduced [V | U0]^T U0 within the Gram bound of tests/dense_ref.py (64 eps |X|^T|U|) of the long-double product of the stored
     U0, and of what the existing OP_GRAMX sweep (dla_gram on [V | U0]) gives on the same stored U0
  d. a basis of 113 columns, odd n, a pencil preconditioner and a request for Ritz vectors decline: the call returns what
     dla_ritz_residual returns, bit for bit, U0 is not touched and no fused sweep is counted

1e30 guard columns stand behind R and behind the U0 block and must come back untouched.  The diagonal is the stored sparse operator's
(a diagonal matrix set up for the purpose), so the test chooses it."""
import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LD = np.longdouble
GUARD = 1.0e30
FAC = -1.0e-5
# (n_max, first): one block of 13 columns with the first open root at the front, in the middle and last; a full tile
BLOCKS = [(13, 1), (13, 5), (13, 13), (16, 1)]
WIDTHS = [13, 16, 17, 48, 97, 112]
ROWS = [66, 4098]


def _diagonal(n, rng):
    """a diagonal with rows where |d + FAC| <= 1e-5 (0, just under, negative side) and one where d + FAC is EXACTLY 1e-5
    (FAC = -1e-5 and d = 2e-5: the sum of the two doubles is the double 1e-5)"""
    d = rng.uniform(1.0, 3.0, n)
    d[3] = -FAC                       # den = 0
    d[n // 2] = -FAC + 9.0e-6         # under the threshold
    d[n - 2] = -FAC - 5.0e-6          # under it, negative
    d[7] = 2.0e-5                     # den == 1e-5 exactly: `>` keeps the row unscaled
    assert d[7] + FAC == 1.0e-5 and abs(d[n // 2] + FAC) < 1.0e-5 and abs(d[n - 2] + FAC) < 1.0e-5
    d[n - 1] = -FAC + 2.0e-5          # just above: scaled by 5e4
    return d


@pytest.fixture(scope="module")
def operators(ctx):
    """the diagonal operators, set up once per row count (the stored sparse slot holds one at a time)"""
    made = {}

    def use(n):
        if made.get("n") != n:
            d = _diagonal(n, np.random.default_rng(n))
            ctx.spmm_setup(sp.diags(d).tocsr())
            made["n"], made["d"] = n, d
        return made["d"]
    return use


def _inputs(n, m, nb, first, seed):
    rng = np.random.default_rng(seed)
    v = np.asfortranarray(rng.standard_normal((n, m)))
    av = np.asfortranarray(rng.standard_normal((n, m)))
    y = np.asfortranarray(rng.standard_normal((m + 3, nb)) / np.sqrt(m))     # (ldy > l: three rows nobody may read)
    y[m:] = np.nan
    eig = np.sort(rng.uniform(0.5, 2.0, nb))
    skip = np.zeros(nb, dtype=np.int32)
    skip[:first - 1] = 1                                                     # the locked roots in front
    n_res = min(nb, first + 3)
    return v, av, y, eig, skip, n_res


def _reference(v, av, y, eig, skip, n_res):
    """R in long double, its magnitude |AV||Y| + |V||Y Lambda|, and which columns are corrected"""
    m, nb = v.shape[1], y.shape[1]
    yl = y[:m].astype(LD)
    open_ = np.array([j < n_res and not skip[j] for j in range(nb)])
    lam = np.where(open_, eig, 0.0).astype(LD)
    ref = av.astype(LD) @ yl - v.astype(LD) @ (yl * lam)
    mag = np.abs(av).astype(LD) @ np.abs(yl) + np.abs(v).astype(LD) @ np.abs(yl * lam)
    return ref, mag, open_


def _run(ctx, d, v, av, y, eig, skip, n_res, first, precnd="dla_spmm_precnd", evec=False):
    n, m = v.shape
    nb = y.shape[1]
    k = nb - first + 1
    space = np.full((n, m + k + 2), GUARD, order="F")
    space[:, :m] = v
    pspace = ctx.panel(space)
    pav = ctx.panel(av)
    pres = ctx.panel(np.full((n, nb + 2), GUARD, order="F"))
    pevec = ctx.panel(np.full((n, nb), GUARD, order="F")) if evec else None
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    rn, fused = ctx.ritz_expand(pspace.col(0, m), pav, y, eig, n_res, skip, pevec, pres.col(0, nb), capi.fn_address(precnd), FAC, first,
                                pspace.col(m, k), m=nb)
    measured = ctx.ritz_expand_measured(m, k) if fused else None
    gramx = None
    if fused:
        # the existing measuring sweep on the same stored block: X^T U0 and U0^T U0
        gramx = np.vstack([ctx.gram(pspace.col(0, m), pspace.col(m, k)), ctx.gram(pspace.col(m, k), pspace.col(m, k))])
    out = {"rn": rn, "fused": fused, "space": pspace.download(), "res": pres.download(), "measured": measured, "gramx": gramx,
           "evec": pevec.download() if evec else None}
    return out


@pytest.mark.parametrize("nb,first", BLOCKS)
@pytest.mark.parametrize("m", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_fused_sweep_against_long_double(ctx, operators, n, m, nb, first):
    d = operators(n)
    v, av, y, eig, skip, n_res = _inputs(n, m, nb, first, seed=1000 * m + 10 * nb + first + n)
    run0, _ = ctx.ritz_expand_counts()
    out = _run(ctx, d, v, av, y, eig, skip, n_res, first)
    assert out["fused"], "the fused sweep declined a shape it is built for"
    assert ctx.ritz_expand_counts()[0] == run0 + 1
    k = nb - first + 1
    # guards: the basis itself, the columns behind the block, the columns behind R
    assert np.array_equal(out["space"][:, :m], v)
    assert np.all(out["space"][:, m + k:] == GUARD) and np.all(out["res"][:, nb:] == GUARD)
    # (a) R and the norms
    r = out["res"][:, :nb]
    ref, mag, open_ = _reference(v, av, y, eig, skip, n_res)
    bound = (2 * m + 2) * EPS * mag
    ratio = float((np.abs(r.astype(LD) - ref) / bound).max())
    print(f"n={n} m={m} nb={nb} first={first}: max |R - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    for j in range(n_res):
        if not open_[j]:
            continue
        rj, bj = ref[:, j], bound[:, j]
        ssq_ref = float((rj * rj).sum())
        ssq_bound = float((2 * np.abs(rj) * bj + bj * bj).sum()) + (n + 2) * EPS * ssq_ref
        ssq_got = (out["rn"][0, j] * np.sqrt(n)) ** 2
        print(f"  root {j}: sum r^2 {ssq_got:.17g} (ref {ssq_ref:.17g}, bound {ssq_bound:.3g}), max {out['rn'][1, j]:.17g}")
        assert abs(ssq_got - ssq_ref) <= ssq_bound + 8 * EPS * ssq_ref           # (+ the square root and its square: a few eps)
        assert abs(out["rn"][1, j] - float(np.abs(rj).max())) <= float(bj.max())
        assert out["rn"][1, j] == np.abs(r[:, j]).max()                            # the maximum of what was stored, exactly
    rn_plain, res_plain, _ = _plain(ctx, v, av, y, eig, skip, n_res)
    assert np.array_equal(out["res"], res_plain), "R differs from the plain sweep's"
    assert np.allclose(out["rn"][:, open_[:n_res]], rn_plain[:, open_[:n_res]], rtol=(n + 2) * EPS, atol=0)
    # (b) the stored block: the library's rule on the stored R, exactly
    u0 = out["space"][:, m:m + k]
    den = d + FAC
    want = np.where((np.abs(den) > 1.0e-5)[:, None], r[:, first - 1:] / den[:, None], r[:, first - 1:])
    assert np.array_equal(u0, want)
    assert np.array_equal(u0[3], r[3, first - 1:]) and np.array_equal(u0[7], r[7, first - 1:])   # under and at the threshold: unscaled
    # (c) what the chain will read, against the long-double product of the stored block and against the existing sweep
    xu = np.hstack([v, u0])
    gref = xu.astype(LD).T @ u0.astype(LD)
    gbound = 64 * EPS * (np.abs(xu).astype(LD).T @ np.abs(u0).astype(LD)) + np.finfo(np.float64).tiny
    gratio = float((np.abs(out["measured"].astype(LD) - gref) / gbound).max())
    xratio = float((np.abs(out["measured"].astype(LD) - out["gramx"].astype(LD)) / (2 * gbound)).max())
    print(f"  [V | U0]^T U0: against long double {gratio:.3f} of the bound, against the OP_GRAMX sweep {xratio:.3f} of twice the bound")
    assert gratio <= 1.0 and xratio <= 1.0


def _plain(ctx, v, av, y, eig, skip, n_res, evec=False):
    n, m = v.shape
    nb = y.shape[1]
    pv, pav = ctx.panel(v), ctx.panel(av)
    pres = ctx.panel(np.full((n, nb + 2), GUARD, order="F"))
    pevec = ctx.panel(np.full((n, nb), GUARD, order="F")) if evec else None
    rn = ctx.ritz_residual(pv, pav, y, eig, n_res, skip, pevec, pres.col(0, nb), m=nb)
    return rn, pres.download(), pevec.download() if evec else None


@pytest.mark.parametrize("why", ["m=113", "odd n", "pencil preconditioner", "Ritz vectors", "knob"])
def test_shapes_and_requests_it_does_not_take_are_the_plain_sweep(ctx, operators, why):
    n = 67 if why == "odd n" else 66
    m = 113 if why == "m=113" else 48
    nb, first = 13, 5
    d = operators(n)
    if why == "knob":
        ctx.set_option(100, 16)
    v, av, y, eig, skip, n_res = _inputs(n, m, nb, first, seed=77)
    run0, dropped0 = ctx.ritz_expand_counts()
    out = _run(ctx, d, v, av, y, eig, skip, n_res, first, precnd="dla_spmm_precnd_pencil" if why == "pencil preconditioner" else "dla_spmm_precnd",
               evec=why == "Ritz vectors")
    assert not out["fused"]
    assert ctx.ritz_expand_counts() == (run0, dropped0)
    rn, res, evec = _plain(ctx, v, av, y, eig, skip, n_res, evec=why == "Ritz vectors")
    assert np.array_equal(out["rn"], rn) and np.array_equal(out["res"], res)
    assert np.all(out["space"][:, m:] == GUARD), "a declined call wrote the block"
    if why == "Ritz vectors":
        assert np.array_equal(out["evec"], evec)


def test_the_chain_takes_the_record_and_anything_in_between_drops_it(ctx, operators):
    """dla_ortho_vs_x right behind the fused sweep starts from its measurement (no OP_GRAMX sweep is booked) and ends with the block
    orthonormal and orthogonal to the basis (50 eps, the bound of tests/test_ortho_chain_gpu.py; fac = 1 keeps every denominator in
    [1, 4], a block as well conditioned as that file's); a preconditioner call in between drops the record, and the chain sweeps as before"""
    n, m, nb, first = 4098, 48, 13, 1
    d = operators(n)
    rng = np.random.default_rng(5)
    q, _ = np.linalg.qr(rng.standard_normal((n, m)))
    av = np.asfortranarray(rng.standard_normal((n, m)))
    y = np.asfortranarray(rng.standard_normal((m, nb)) / np.sqrt(m))
    eig = np.sort(rng.uniform(0.5, 2.0, nb))
    skip = np.zeros(nb, dtype=np.int32)
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    gramx = "gram_lds_kernel<3, 1, 1, 16, 0, 0, 0, 1>"
    for between in (False, True):
        space = np.full((n, m + nb), GUARD, order="F")
        space[:, :m] = q
        pspace, pav, pres = ctx.panel(space), ctx.panel(av), ctx.panel(n, nb)
        run0, dropped0 = ctx.ritz_expand_counts()
        _, fused = ctx.ritz_expand(pspace.col(0, m), pav, y, eig, nb, skip, None, pres, capi.fn_address("dla_spmm_precnd"), 1.0, first,
                                   pspace.col(m, nb), m=nb)
        assert fused
        if between:
            ctx._chk(ctx.lib.dla_call_precnd(ctx.h, capi.fn_address("dla_spmm_precnd"), n, nb, 1.0, pres.ptr, pspace.col(m, nb).ptr))
        ctx.reset_stats()
        ctx.ortho_vs_x(pspace.col(0, m), pspace.col(m, nb))
        ctx.sync()
        booked = {name: st["launches"] for name, st in ctx.kernel_stats().items() if st["launches"] > 0}
        assert ctx.ritz_expand_counts() == (run0 + 1, dropped0 + (1 if between else 0))
        assert (gramx in booked) == between, booked
        got = pspace.download()
        u = got[:, m:]
        assert np.array_equal(got[:, :m], q)
        print(f"between={between}: max |U^T U - I| = {np.abs(u.T @ u - np.eye(nb)).max():.3e}, max |X^T U| = {np.abs(q.T @ u).max():.3e}")
        assert np.abs(u.T @ u - np.eye(nb)).max() < 50 * EPS and np.abs(q.T @ u).max() < 50 * EPS
