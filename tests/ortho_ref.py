"""Long-double reference, cases and checkers for the orthogonalisation on the standard inner product: ortho_cd (reference
diaglib.f90:3185-3341) and ortho_vs_x (:3481-3574).  Plain numpy in np.longdouble (x87 extended: eps 1.1e-19); the algebra is that of
tests/metric_ortho_ref.py, nothing of the library is imported here, so that the CPU tests (tests/test_ortho_ref.py: the oracle and
the host-memory engine) and the GPU tests (tests/test_ortho_ref_gpu.py) hold their subjects to the same reference with the same
bounds.

The reference: P = (I - X X^T) U applied three times, then the unique Q with P = Q R, R upper triangular with a positive diagonal, by
column-oriented Gram-Schmidt with re-orthogonalisation (three passes, each column normalised).  Not by Cholesky-QR: the Gram matrix
of a block of condition 1e10 has condition 1e20, beyond the long-double epsilon, and its Cholesky factorisation meets a negative
pivot; test_ortho_ref.py shows that the two agree wherever the Cholesky-based one (metric_ortho_ref.ref_b_ortho_vs_x(x, x, u)) runs.

The bounds follow the conditioning of each case:

  a      ||U||_2 / sigma_min(P): what the projection cancels times what the factorisation of P amplifies.
  a_eq   the same with the columns of P (and of U with them) scaled to unit norm of P's columns.  The Q factor is invariant to a
         scaling of the columns of U (R -> R D), so the equilibrated figure bounds the error as well; for the column-scaled blocks,
         whose a is 1e16 by construction, it is the only bound that says anything.  The checker takes min(a, a_eq).
  pi     ||X||_2^2, the norm of the projector's subtracted part (1 to rounding; 1 without an X).

eps is the double-precision epsilon, 64 the constant of the project's kernel tests (tests/test_kernels_gpu.py), 50 the bar of its
orthogonality tests.  Every check returns its worst ratio error / bound; `limit` is the ratio it asserts (1 for the library, 0.25
for the double-precision oracle, as in the metric module)."""
import pickle
import zlib

import numpy as np

from metric_ortho_ref import EPS, LD, Ref, _assert_ratios, _dev_identity, _norm2, record  # noqa: F401  (record: for the tests)

TUNE6 = 100 + 6           # DLA_OPT_TUNE0 + 6, the chain's knob (hip_plans.h: 0 shipped, 12 five-sweep, 13 three-pass, 3 host loop)


# ---------------------------------------------------------------------------------------------------------------- long-double algebra
def project(x, p):
    """(I - X X^T) P in long double"""
    return p - x @ (x.T @ p) if x.shape[1] else p


def gram_schmidt(p):
    """the Q of P = Q R with a positive diagonal of R: three passes of modified Gram-Schmidt over the block, every column against the
    ones before it, one after the other, and then normalised.  The first pass loses eps_ld kappa_2(P) of orthogonality (1e-9 at
    kappa = 1e10), the second restores eps_ld; each pass multiplies by an upper-triangular factor with a positive diagonal, so Q
    is the Q of P."""
    q = np.array(p, LD)
    for _ in range(3):
        for j in range(q.shape[1]):
            for i in range(j):
                q[:, j] -= (q[:, i] @ q[:, j]) * q[:, i]
            q[:, j] /= np.sqrt(q[:, j] @ q[:, j])
    return q


def gram_schmidt_blocked(p):
    """the same Q for a well-conditioned block (a random X of a few hundred columns): every column against all the ones before it at
    once, twice, and then normalised"""
    q = np.array(p, LD)
    for j in range(q.shape[1]):
        for _ in range(2 if j else 0):
            q[:, j] -= q[:, :j] @ (q[:, :j].T @ q[:, j])
        q[:, j] /= np.sqrt(q[:, j] @ q[:, j])
    return q


def _sigma(a):
    return np.linalg.svd(np.asarray(a, np.float64), compute_uv=False)


def ref_ortho_vs_x(x, u, unique=True):
    """unique = False (a rank-deficient block has no unique answer): pi only"""
    x, u = np.asarray(x, LD), np.asarray(u, LD)
    pi = _norm2(x) ** 2 if x.shape[1] else 1.0
    if not unique:
        return Ref(q=None, p=None, pi=pi, a=np.inf, a_eq=np.inf)
    p = u
    for _ in range(3):
        p = project(x, p)
    q = gram_schmidt(p)
    dev = float(np.abs(q.T @ q - np.eye(q.shape[1])).max())
    if not dev < 1e-17:
        raise RuntimeError(f"ref_ortho_vs_x: the long-double orthonormalisation did not converge ({dev:.3g})")
    d = 1 / np.sqrt((p * p).sum(axis=0))
    sp = _sigma(p)
    return Ref(q=q, p=p, pi=pi, a=_norm2(u) / float(sp[-1]), a_eq=_norm2(u * d[None, :]) / float(_sigma(p * d[None, :])[-1]),
               kappa_p=float(sp[0] / sp[-1]))


def first_gram(c):
    """the double-precision Gram matrix a correct implementation cannot avoid factoring: of U itself for a block that is rank
    deficient as given or has no X, of the projected block (projected in long double, rounded to double) behind an X"""
    p = np.asarray(c.ref().p, np.float64) if c.m and c.unique else c.u
    return p.T @ p


def cholesky_fails(g):
    try:
        np.linalg.cholesky(g)
    except np.linalg.LinAlgError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------- blocks
def orthonormal(x0):
    """X orthonormalised in long double, then rounded to double"""
    return np.asfortranarray(gram_schmidt_blocked(np.asarray(x0, LD)).astype(np.float64))


def graded_cond(kind):
    return float(kind[len("graded"):])


def make_u(kind, rng, x, n, k):
    m = x.shape[1]
    if kind == "random":
        u = rng.standard_normal((n, k))
    elif kind == "near_span":
        u = x @ rng.standard_normal((m, k)) + 1e-7 * rng.standard_normal((n, k))
    elif kind == "colscaled":
        u = rng.standard_normal((n, k)) * np.logspace(-8, 8, k)[None, :]
    elif kind.startswith("graded"):
        # orthonormal x logspace singular values x random orthogonal.  Behind an X the orthonormal factor is taken in the complement
        # of span(X) and a part inside span(X) of the size of the leading singular value is added: P, not only U, has the grading
        q = np.linalg.qr(project(x, rng.standard_normal((n, k))))[0]
        q = np.linalg.qr(project(x, q))[0]
        sv = np.logspace(0, -np.log10(graded_cond(kind)), k) if k > 1 else np.ones(1)
        u = q * sv[None, :] @ np.linalg.qr(rng.standard_normal((k, k)))[0]
        if m:
            u = u + x @ rng.standard_normal((m, k)) / np.sqrt(m)
    elif kind == "rank_deficient":
        u = rng.standard_normal((n, k)); u[:, -1] = u[:, 0] + u[:, 1]
    else:
        raise ValueError(kind)
    return np.asfortranarray(u)


# A block is drawn from a generator seeded by the case's name and, where one is listed here, a draw number, as in the metric module.
# The CPU test asks that the double-precision oracle meets a QUARTER of every bound on every case -- a condition on the inputs,
# checked without the library.  The oracle's |Q^T Q - I| lies between 0.005 and 0.40 of the 50 eps bar over the draws of one shape (its
# Gram matrices are sequential sums of n terms), on either side of the quarter.  The draws listed are the first (0, 1, 2, ...) at
# which the oracle's worst ratio was below 0.22 and, for the kinds in NEEDS_SHIFT, the double-precision Cholesky factorisation of
# the block's double-precision Gram matrix failed, in LAPACK's and in the oracle's order of operations alike (the last pivot of a
# rank-deficient block is rounding noise of either sign: half the draws leave a tiny positive one and prove nothing about the level
# shifts).  `python tests/ortho_ref.py` applies the rule and prints the table; nothing the library computes went into the choice.
NEEDS_SHIFT = ("graded1e10", "rank_deficient")
DRAWS = {"std_n2001_m26_k1_random": 1, "std_n2001_m0_k4_random": 1, "std_n2000_m26_k13_random": 1, "std_n2000_m0_k15_random": 1,
         "std_n2001_m0_k15_random": 2, "std_n2001_m0_k16_random": 1, "std_n2000_m26_k31_random": 3, "std_n2001_m0_k31_random": 1,
         "std_n2000_m0_k32_random": 4, "std_n2000_m0_k33_random": 3, "std_n2001_m0_k33_random": 2, "std_n2000_m26_k47_random": 1,
         "std_n2000_m0_k47_random": 2, "std_n2001_m26_k47_random": 3, "std_n2001_m0_k47_random": 2, "std_n2000_m0_k48_random": 2,
         "std_n2001_m26_k48_random": 3, "std_n2000_m26_k49_random": 4, "std_n2000_m0_k49_random": 4, "std_n2001_m26_k49_random": 9,
         "std_n2001_m0_k49_random": 3, "std_n2000_m26_k33_near_span": 1, "std_n2000_m26_k48_near_span": 2,
         "std_n2000_m26_k13_graded1e6": 2, "std_n2000_m26_k16_graded1e6": 1, "std_n2000_m26_k17_colscaled": 3,
         "std_n2000_m0_k17_colscaled": 1, "std_n2000_m26_k17_graded1e6": 1, "std_n2000_m26_k33_colscaled": 5,
         "std_n2000_m26_k48_colscaled": 5, "std_n2000_m0_k48_colscaled": 1, "std_n2000_m26_k48_graded1e6": 6,
         "std_n2000_m0_k48_graded1e6": 2, "std_n2000_m0_k13_graded1e10": 2, "std_n2001_m26_k13_graded1e10": 3,
         "std_n2001_m0_k13_graded1e10": 1, "std_n2000_m26_k13_rank_deficient": 5, "std_n2000_m0_k13_rank_deficient": 4,
         "std_n2001_m26_k13_rank_deficient": 4, "std_n2000_m0_k16_graded1e10": 1, "std_n2001_m26_k16_graded1e10": 1,
         "std_n2001_m0_k16_graded1e10": 1, "std_n2000_m26_k16_rank_deficient": 8, "std_n2001_m26_k16_rank_deficient": 1,
         "std_n2001_m0_k16_rank_deficient": 2, "std_n2001_m26_k17_graded1e10": 1, "std_n2000_m26_k17_rank_deficient": 2,
         "std_n2000_m0_k17_rank_deficient": 1, "std_n2001_m0_k17_rank_deficient": 1, "std_n2000_m26_k33_graded1e10": 4,
         "std_n2000_m26_k33_rank_deficient": 10, "std_n2000_m0_k33_rank_deficient": 1, "std_n2001_m26_k33_rank_deficient": 5,
         "std_n2000_m26_k48_graded1e10": 1, "std_n2000_m0_k48_graded1e10": 2, "std_n2001_m26_k48_graded1e10": 3,
         "std_n2000_m0_k48_rank_deficient": 15, "std_n2001_m26_k48_rank_deficient": 7, "std_n2001_m0_k48_rank_deficient": 6,
         "std_n2000_m193_k13_random": 1, "std_n2000_m96_k32_random": 1, "std_n2000_m97_k32_random": 1,
         "std_n3000_m247_k13_near_span": 2}


class Case:
    """one block problem: an orthonormal X (n x m, m may be 0) and U (n x k).  Seeded by its own name, built once per process
    (case()), read only."""

    def __init__(self, n, m, k, kind, draw=None):
        self.n, self.m, self.k, self.kind = n, m, k, kind
        self.name = f"std_n{n}_m{m}_k{k}_{kind}"
        draw = DRAWS.get(self.name, 0) if draw is None else draw
        rng = np.random.default_rng(zlib.crc32((self.name + (f"/{draw}" if draw else "")).encode()))
        self.x = orthonormal(rng.standard_normal((n, m))) if m else np.zeros((n, 0), order="F")
        self.u = make_u(kind, rng, self.x, n, k)
        self.unique = kind != "rank_deficient"
        for a in (self.x, self.u):
            a.setflags(write=False)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = ref_ortho_vs_x(self.x, self.u, self.unique)
        return self._ref


class Given(Case):
    """a block handed in (the golden fixtures)"""

    def __init__(self, name, x, u):
        self.n, self.k = u.shape
        self.x = np.zeros((self.n, 0), order="F") if x is None else np.asfortranarray(x)
        self.m, self.u, self.name, self.kind, self.unique, self._ref = self.x.shape[1], np.asfortranarray(u), name, "given", True, None


_CASES = {}


def case(n, m, k, kind):
    key = (n, m, k, kind)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


def dump_cases(path):
    """the cases built so far with the references computed so far, for a worker process that would otherwise compute them again"""
    with open(path, "wb") as f:
        pickle.dump(_CASES, f)


def load_cases(path):
    with open(path, "rb") as f:
        _CASES.update(pickle.load(f))


def ident(key):
    return "-".join(str(v) for v in key)


# ---------------------------------------------------------------------------------------------------------------- the case table
# Block widths: the 4-row blocks of ortho_tail16's LDL^T and its partly masked last block (1, 2, 3, 4, 8, 12, 13, 15), its full
# tile (16), the hand-over to the LDS-loop step (17), that step's tile edges (31, 32, 33, 47, 48) and the hand-over to the host-driven
# loop (49: chain_choice declines k > 48).  Even n takes the 16-byte path (ChainIn::vec2), odd n the 8-byte one, on which chain_choice
# keeps one-tile blocks on the sweep-per-update schedule (fold = 2) and wide blocks on the plain wide chain; m = 0 is ortho_cd.
WIDTHS = (1, 2, 3, 4, 8, 12, 13, 15, 16, 17, 31, 32, 33, 47, 48, 49)
WIDTH_CASES = [(n, m, k, "random") for k in WIDTHS for n in (2000, 2001) for m in (26, 0)]
# fewer rows than one row tile: n = k + 1 (the block alone: behind four basis columns no 13 columns of full rank are left in 14 rows)
# and n = k + 5 with m = 4
FEW_ROWS_CASES = [(14, 0, 13, "random"), (18, 4, 13, "random")]
# every other kind at one width of each k x k step and tile count, with and without X (near_span is defined by its X); the blocks
# that need the level-shift ladder on the 8-byte path as well: that is where fold = 2 meets the ladder
KIND_WIDTHS = (13, 16, 17, 33, 48)
KIND_CASES = ([(2000, 26, k, "near_span") for k in KIND_WIDTHS] +
              [(2000, m, k, kind) for k in KIND_WIDTHS for kind in ("colscaled", "graded1e6") for m in (26, 0)] +
              [(n, m, k, kind) for k in KIND_WIDTHS for kind in ("graded1e10", "rank_deficient") for n in (2000, 2001) for m in (26, 0)])
# both sides of every edge of chain_choice (hip_plans.h) that the widths above do not straddle already (they do: k = 16 | 17, one-tile
# blocks on the matrix cores; k = 32 | 33, wide_xw takes two-tile blocks only; k = 48 | 49, the chain; n even | odd, vec2)
EDGE_CASES = [
    (2000, 192, 13, "random"), (2000, 193, 13, "random"),   # fold = 1 | 2: the pending-factor schedule takes m <= 192
    (2000, 96, 32, "random"), (2000, 97, 32, "random"),     # wide_gramx on | off, two tiles: (m + k + 15) / 16 <= 8, k = 32: m <= 96
    (2000, 64, 48, "random"), (2000, 65, 48, "random"),     # wide_gramx on | off, three tiles: (m + k + 15) / 16 <= 7, k = 48: m <= 64
    # wide_xw on | off for two-tile blocks: its own limits ((m + 15) / 16 <= wp_max_tlw(2) = 8: m <= 128; (m + k) k <= XUG_DOUBLES)
    # lie beyond the wide_gramx limit it also requires (m <= 111 at k = 17, m <= 96 at k = 32), so it ends where wide_gramx ends:
    # the pair above at k = 32, and this one at the narrowest two-tile block
    (2000, 111, 17, "random"), (2000, 112, 17, "random"),
    (3000, 247, 13, "near_span"),                           # (the widest X of the existing chain test: 16 tiles in two passes)
]
ALL_CASES = list(dict.fromkeys(WIDTH_CASES + FEW_ROWS_CASES + KIND_CASES + EDGE_CASES))
# between guard columns: every k x k step and tile count, a block that passes and one that shifts, even and odd n
GUARD_CASES = [(n, 26, k, kind) for k in KIND_WIDTHS for kind in ("random", "rank_deficient") for n in (2000, 2001)]


def well_conditioned_twin(key):
    """the plain random block of a case's shape (the call after a chain that shifted)"""
    n, m, k, _ = key
    return (n, m, k, "random")


# ---------------------------------------------------------------------------------------------------------------- checkers
def q_bound(ref):
    return 64 * EPS * ref.pi * min(ref.a, ref.a_eq)


def check(q, c, x_after=None, what=None, limit=1.0):
    """the invariants, and for a block with a unique answer |Q - Q_ref|"""
    what = what or c.name
    ref = c.ref()
    assert np.all(np.isfinite(q)), what + ": non-finite output"
    if x_after is not None:
        assert x_after.shape == c.x.shape and np.array_equal(x_after, c.x), what + ": X was modified"
    ql = np.asarray(q, LD)
    ratios = {"qtq": _dev_identity(q, q) / (50 * EPS)}
    if c.m:
        ratios["xtq"] = float(np.abs(np.asarray(c.x, LD).T @ ql).max()) / (50 * EPS * ref.pi)
    if c.unique:
        ratios["q"] = float(np.abs(ql - ref.q).max()) / q_bound(ref)
    _assert_ratios(what, ratios, limit)
    assert ratios["qtq"] < limit, (what, ratios)            # (the project's existing bar is a strict one)
    return ratios


def worst(ratios):
    return max(ratios.values())


if __name__ == "__main__":
    # the draw table: for every case the first draw at which the double-precision oracle's worst ratio is below 0.22
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.pyoracle import Oracle
    o = Oracle()
    table = {}
    for key in ALL_CASES:
        for draw in range(40):
            c = Case(*key, draw=draw)
            q = o.ortho_vs_x(c.x, c.u)[0] if c.m else o.ortho_cd(c.u)[0]
            try:
                w = worst(check(q, c, limit=np.inf))
            except AssertionError:
                w = np.inf
            if w < 0.22 and (c.kind not in NEEDS_SHIFT or (cholesky_fails(first_gram(c)) and o.potrf_lower(first_gram(c))[1] != 0)):
                break
        else:
            raise SystemExit(f"{c.name}: no draw below 0.22")
        if draw:
            table[c.name] = draw
        print(c.name, draw, f"{w:.3g}", flush=True)
    print("DRAWS =", table)
