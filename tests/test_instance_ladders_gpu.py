"""GPU: the dispatch ladders of hip_engine.hip launch the instance the planners name, for every row of the instance lists of
hip_plans.h (GRAM_TILES, GRAM_LOW_TILES, WP_TILES, RITZ_INSTANCES) that a small call can reach, and for the gemm_kernel instances
(GEMM_INSTANCES) of one to three column tiles: plain and fused, in the kernel arguments and packed, with quarter tiles, accumulating,
and at the pipeline depths of knob 2.

Each call must succeed (a plan without a row is "no kernel instance"), give the right numbers, and book the name that the CPU
planners (tests/plans_driver.cpp, through tests/test_plans.py) print for the request line of exactly that shape.  n = 1000 is even
with a partial last wave tile (the 16-byte path, the LDS-staged kernels); n = 999 is odd (the 8-byte path, the direct-load kernels).
Bounds are the neighbours': tests/test_kernels_gpu.py for the Gram matrices and the Ritz sweep, test_chain_ortho_vs_x_vs_oracle of
tests/test_ortho_chain_gpu.py for the chains, tests/test_dense_sweeps_gpu.py (the checkers of tests/dense_ref.py) for the panel
products.  Nothing here forces a failure path (tests/test_lds_refusal_gpu.py does)."""
import re
import zlib

import numpy as np
import pytest

import dense_ref
from test_plans import LDS, env_line, run_plans

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TUNE_CHAIN = 100 + 6
N_EVEN, N_ODD = 1000, 999
SWEEPS = r"(gram_lds_kernel|gram_kernel|ritz_kernel)<"


@pytest.fixture(scope="module")
def panels():
    """seeded random panels, computed once and read only: 208 columns for the X side, 109 for the U side, 1000 rows (999: the first)"""
    rng = np.random.default_rng(20241018)
    x, u = np.asfortranarray(rng.standard_normal((N_EVEN, 208))), np.asfortranarray(rng.standard_normal((N_EVEN, 109)))
    q = np.asfortranarray(np.linalg.qr(x[:, :192])[0])
    for a in (x, u, q):
        a.setflags(write=False)
    return x, u, q


def names_of(lines):
    return [name for _, name in run_plans([env_line()] + lines)[0]]


def booked(ctx, family=SWEEPS):
    return sorted(name for name, st in ctx.kernel_stats().items() if st["launches"] > 0 and re.match(family, name))


def gram_bound(x, u):
    return 64 * EPS * (np.abs(x).T @ np.abs(u)) + 1e-300


GRAM_CASES = [(16 * t - 3, k, 0, 0) for t in range(1, 14) for k in (13, 29, 45, 61)] + [(4, 13, 0, 0)] + [(k, k, 1, 0) for k in (13, 29, 45)] + \
             [(k, k, 0, 1) for k in (61, 77, 93, 109)]


@pytest.mark.parametrize("n", [N_EVEN, N_ODD])
def test_gram_ladders(ctx, panels, n):
    """X^T U of l = 16 t - 3 columns (t = 1 .. 13 X tiles) against 1 .. 4 U tiles, a pass narrower than one tile, blocks against
    themselves, and gram_lower of 4 .. 7 tiles (single-pass lower triangle on even n): (l, k, same, lower)"""
    x, u, _ = panels
    x, u = np.asfortranarray(x[:n]), np.asfortranarray(u[:n])
    px, pu = ctx.panel(x), ctx.panel(u)
    want_names = names_of([f"gram {n} {l} {k} {same} {1 - n % 2} {low}" for l, k, same, low in GRAM_CASES])
    seen = set()
    for (l, k, same, low), want_name in zip(GRAM_CASES, want_names):
        a, pa = (u, pu) if same else (x, px)
        ctx.reset_stats()
        got = ctx.gram_lower(pa.col(0, l), pu.col(0, k)) if low else ctx.gram(pa.col(0, l), pu.col(0, k))      # (raises unless DLA_OK)
        assert booked(ctx) == [want_name], (n, l, k, same, low, want_name, booked(ctx))
        want = a[:, :l].T @ u[:, :k]
        ok = np.abs(got - want) <= gram_bound(a[:, :l], u[:, :k])
        if low:
            ok = ok[np.tril(np.ones((l, l), bool))]
        assert np.all(ok), (n, l, k, same, low, want_name)
        seen.add(want_name)
    print(n, sorted(seen))


CHAIN_CASES = [(16 * t - 3, 13, s) for t in range(1, 13) for s in (0, 13)] + [(m, 29, 0) for m in (13, 61, 125)] + [(m, 45, 0) for m in (13, 77)]


def test_pending_factor_sweeps(ctx, panels):
    """ortho_vs_x of a k-column block behind m basis columns in one panel (m = 16 t - 3: 1 .. 12 X tiles beside the block's) under
    the default schedule and the three-pass one (knob 6 = 13: the projection sweep WP == 2), and two- and three-tile blocks;
    n = 1000 takes the chain (the 16-byte path: the block starts at 8000 m bytes)"""
    _, u, q = panels
    n = N_EVEN
    for m, k, schedule in CHAIN_CASES:
        what = (m, k, schedule)
        big = ctx.panel(np.asfortranarray(np.hstack([q[:, :m], u[:, :k]])))
        ctx.set_option(TUNE_CHAIN, schedule)
        ctx.reset_stats()
        try:
            ctx.ortho_vs_x(big.col(0, m), big.col(m, k))
        finally:
            ctx.set_option(TUNE_CHAIN, 0)
        ran = booked(ctx, r"gram_lds_kernel<")
        got = big.col(m, k).download()
        assert np.array_equal(big.col(0, m).download(), q[:, :m]), what
        assert np.abs(got.T @ got - np.eye(k)).max() < 50 * EPS, what
        assert np.abs(q[:, :m].T @ got).max() < 50 * EPS, what
        # the sweeps a chain of this (m, k) is made of: the pending-factor sweeps, and the plain Gram matrices of the other schedules
        lines = [f"wp {n} {m} {k} 0"] + ([f"wp {n} 0 {k} 0", f"wp {n} {m} {k} 1"] if k <= 16 else [])
        lines += [f"gram {n} {k} {k} 1 1 0", f"gram {n} {m} {k} 0 1 0", f"gram {n} {m + k} {k} 0 1 0"]
        allowed = names_of(lines)
        print(what, ran)
        assert ran and set(ran) <= set(allowed), (what, ran, allowed)
        if k <= 16:
            assert allowed[0] in ran, (what, ran, allowed)                    # the measuring sweep over [X | U]
        if schedule == 13:
            assert allowed[2] in ran, (what, ran, allowed)                    # the projection sweep that measures what it stores


@pytest.mark.parametrize("n", [N_EVEN, N_ODD])
def test_ritz_ladder(ctx, panels, n):
    x, _, _ = panels
    l = 64
    v, av = np.asfortranarray(x[:n, :l]), np.asfortranarray(x[:n, 100:100 + l])
    pv, pav = ctx.panel(v), ctx.panel(av)
    rng = np.random.default_rng(7)
    for m in (8, 21, 29, 37, 45):
        y = np.asfortranarray(rng.standard_normal((l, m)))
        eig = rng.standard_normal(m)
        skip = np.zeros(m, np.int32); skip[1] = 1
        pe, pr, pa = ctx.panel(n, m), ctx.panel(n, m), ctx.panel(n, m)
        ctx.reset_stats()
        rn = ctx.ritz_residual(pv, pav, y, eig, m, skip, pe, pr, pa)
        assert booked(ctx) == names_of([f"ritz {n} {l} {m} 0 {1 - n % 2} 1"]), (n, m, booked(ctx))
        check_ritz(v, av, y, eig, skip, pe.download(), pr.download(), pa.download(), rn, n)


def check_ritz(v, av, y, eig, skip, e_got, r_got, a_got, rn, n):
    """the bounds of test_ritz_residual (tests/test_kernels_gpu.py)"""
    ev_want, avy_want = v @ y, av @ y
    r_want = avy_want - np.where(skip, 0.0, eig)[None, :] * ev_want
    b1 = 64 * EPS * (np.abs(v) @ np.abs(y)) + 1e-300
    b2 = 64 * EPS * (np.abs(av) @ np.abs(y)) + 1e-300
    assert np.all(np.abs(e_got - ev_want) <= b1)
    assert np.all(np.abs(a_got - avy_want) <= b2)
    assert np.all(np.abs(r_got - r_want) <= b2 + np.abs(eig)[None, :] * b1 + 4 * EPS * np.abs(r_want))
    for i in range(len(eig)):
        if skip[i]:
            assert rn[0, i] == 0.0 and rn[1, i] == 0.0
        else:
            assert np.isclose(rn[0, i], np.linalg.norm(r_got[:, i]) / np.sqrt(n), rtol=1e-13)
            assert rn[1, i] == np.abs(r_got[:, i]).max()


def test_ritz_ladder_with_extra_products(ctx, panels):
    """[Y | C2] of 2, 2 and 5 column tiles in one pass"""
    x, _, _ = panels
    n, l = N_EVEN, 64
    v, av = np.asfortranarray(x[:, :l]), np.asfortranarray(x[:, 100:100 + l])
    pv, pav = ctx.panel(v), ctx.panel(av)
    rng = np.random.default_rng(8)
    for m, k2 in ((13, 13), (21, 5), (37, 37)):
        y, c2 = np.asfortranarray(rng.standard_normal((l, m))), np.asfortranarray(rng.standard_normal((l, k2)))
        eig = rng.standard_normal(m)
        skip = np.zeros(m, np.int32); skip[m // 2] = 1
        pe, pr, pa, pp, pap = ctx.panel(n, m), ctx.panel(n, m), ctx.panel(n, m), ctx.panel(n, k2), ctx.panel(n, k2)
        ctx.reset_stats()
        rn = ctx.ritz_residual_p(pv, pav, y, eig, m, skip, pe, pr, pa, c2, pp, pap)
        assert booked(ctx) == names_of([f"ritz {n} {l} {m} {k2} 1 1"]), (m, k2, booked(ctx))
        check_ritz(v, av, y, eig, skip, pe.download(), pr.download(), pa.download(), rn, n)
        assert np.all(np.abs(pp.download() - v @ c2) <= 64 * EPS * (np.abs(v) @ np.abs(c2)) + 1e-300)
        assert np.all(np.abs(pap.download() - av @ c2) <= 64 * EPS * (np.abs(av) @ np.abs(c2)) + 1e-300)


TUNE_GEMM = 100 + 2
GEMM_K = (13, 21, 29, 37, 45)              # one to three column tiles; quarter tiles of 2 at 21 and 37
GEMM_L = (13, 42, 104)                     # l = 13 under k = 13 travels in the kernel arguments


class PanelDraws:
    """the generator the checkers of tests/dense_ref.py draw from: a block of n rows is the leading columns of the module's panels (the
    first one a checker asks for of X, the second of U), the coefficient blocks are drawn from a seed"""

    def __init__(self, panels, n, seed):
        self.n, self.blocks, self.rng = n, [panels[0][:n], panels[1][:n]], np.random.default_rng(seed)

    def standard_normal(self, shape):
        return self.blocks.pop(0)[:, :shape[1]] if shape[0] == self.n else self.rng.standard_normal(shape)


def fuses(depth, k):
    """what update_gram_once, trmm_gram_once and can_combo ask of a contraction of `depth` rows: the packed coefficients and three spare
    rows in 64 KiB, and the LDS of the sweep (fused_lds) within the limit"""
    kt, l4 = -(-k // 16), -(-depth // 4) * 4
    return k <= 48 and 128 * (depth + 3) * kt <= 65536 and 8 * (kt * l4 * 16 + 64 * (16 * kt + 9)) <= LDS


def gemm_cases(n):
    """[(checker, its shape, knob 2, the planner's request lines)]"""
    v = 1 - n % 2

    def line(l, k, mode, fuse):
        return f"gemm {n} {l} {k} {mode} {fuse} 0 {v}"

    out = []
    for k in GEMM_K:
        # (a shape the engine does not fuse: the triangular update, or the update, as a sweep of its own and the Gram matrix behind it)
        out += [("check_product", (n, k, k, "trmm"), 0, [line(k, k, 2, 0)]),
                ("check_fused", (n, k, k, "trmm_gram"), 0, [line(k, k, 2, 1 if fuses(k, k) else 0)])]
        for l in GEMM_L:
            assert fuses(l + k, k), (l, k)                                                # (dla_combo_gram has no other form)
            out += [("check_product", (n, l, k, "gemm"), 0, [line(l, k, 0, 0)]), ("check_product", (n, l, k, "update"), 0, [line(l, k, 1, 0)]),
                    ("check_fused", (n, l, k, "update_gram"), 0, [line(l, k, 1, 1 if fuses(l, k) else 0)]),
                    ("check_fused", (n, l, k, "combo_gram"), 0, [line(l + k, k, 0, 1)])]
    # 208 rows of three-tile coefficients are two LDS chunks of at most 168: the second one accumulates (mode 3)
    out.append(("check_product", (n, 208, 45, "gemm"), 0, [line(168, 45, 0, 0), line(40, 45, 3, 0)]))
    for knob in (1, 4):                                                                    # pipeline depth 0 / 4 (16-byte path)
        out += [("check_product", (n, l, 29, mode), knob, [line(l, 29, m, 0)]) for l in GEMM_L for m, mode in enumerate(("gemm", "update"))]
    return out


@pytest.mark.parametrize("n", [N_EVEN, N_ODD])
def test_gemm_ladder(ctx, panels, n):
    """dla_panel_gemm, dla_panel_update, dla_trmm_linvt and the fused dla_trmm_gram, dla_update_gram, dla_combo_gram on k columns and a
    contraction of l: launch_gemm launches the instance the plan names, or none"""
    cases = gemm_cases(n)
    want = {knob: iter(run_plans([env_line(t2=knob)] + [ln for _, _, kn, lines in cases if kn == knob for ln in lines])[0]) for knob in (0, 1, 4)}
    seen = set()
    for fn, shape, knob, lines in cases:
        names = sorted(next(want[knob])[1] for _ in lines)
        ctx.set_option(TUNE_GEMM, knob)
        ctx.reset_stats()
        try:
            getattr(dense_ref, fn)(ctx, PanelDraws(panels, n, zlib.crc32(repr((fn, shape, knob)).encode())), *shape)      # (raises unless DLA_OK)
        finally:
            ctx.set_option(TUNE_GEMM, 0)
        assert booked(ctx, r"gemm_kernel<") == names, (fn, shape, knob, lines, names, booked(ctx, r"gemm_kernel<"))
        assert all(st["launches"] == 1 for name, st in ctx.kernel_stats().items() if name in names), (fn, shape, knob)
        seen |= set(names)
    print(n, len(seen), sorted(seen))
