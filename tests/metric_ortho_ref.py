"""Long-double references, cases and checkers for the metric (B-) orthogonalisation: b_ortho (reference diaglib.f90:3094-3183),
b_ortho_vs_x (:3576-3663) and the expansion step dla_expand_project_metric builds from them.  Plain numpy in np.longdouble (x87
extended: eps 1.1e-19) plus scipy.sparse for storage; nothing of the library is imported here, so that the CPU tests
(tests/test_metric_ortho_ref.py: the oracle and the host-memory engine) and the GPU tests (tests/test_metric_ortho_gpu.py) hold
their subjects to the same references with the same bounds.

The bounds follow the conditioning of each case (a fixed 1e-12 is wrong for one case or toothless for another):

  kappa  kappa_2(M) of the Gram matrix M = U^T B U that b_ortho factors.  One Cholesky-QR pass without refinement loses eps kappa.
         The checkers use min(kappa_2(M), kappa_2(S M S)) with S = diag(M)^-1/2: Cholesky-QR is invariant to a scaling of the
         columns of U (M -> S M S, L -> S L, Q unchanged column by column), so the equilibrated condition bounds the error as well;
         for the column-scaled blocks, whose kappa_2(M) is 1e32 by construction, it is the only bound that says anything, and it is
         never wider than the one with kappa_2(M).
  pi     ||X||_2 ||BX||_2, the norm of the oblique projector I - X (BX)^T (1 without an X).
  a      ||U||_2 / sigma_min(P), P = (I - X (BX)^T) U: what the projection cancels.

eps is the double-precision epsilon, 64 the constant of the project's kernel tests (tests/test_kernels_gpu.py), 50 the bar of its
orthogonality tests.  Every check returns its worst ratio error / bound; `limit` is the ratio it asserts (1 for the library, 0.25
for the double-precision oracle: the CPU test thereby shows that every bound leaves the device a factor 4 over what double
arithmetic in the reference's own order achieves)."""
import pickle
import zlib

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
EPS = np.finfo(np.float64).eps
TINY = LD(1e-300)


# ---------------------------------------------------------------------------------------------------------------- long-double algebra
def bmul(b, x):
    """B x in long double from the raw CSR triplets of a scipy.sparse matrix (B is never formed densely)"""
    b = b.tocsr()
    x = np.asarray(x, LD)
    rows = np.repeat(np.arange(b.shape[0], dtype=np.int64), np.diff(b.indptr))
    y = np.zeros(x.shape, LD)
    np.add.at(y, rows, b.data.astype(LD)[:, None] * x[b.indices])
    return y


def absmul(b, x):
    """|B| |x| in long double: the magnitude a dot-product bound is stated in"""
    return bmul(abs(b.tocsr()), np.abs(np.asarray(x, LD)))


def chol_lower(mat):
    """hand-written Cholesky of the lower triangle in long double; raises when a pivot is not positive"""
    k = mat.shape[0]
    l = np.zeros((k, k), LD)
    for j in range(k):
        d = mat[j, j] - l[j, :j] @ l[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is {float(d):.3e}")
        l[j, j] = np.sqrt(d)
        for i in range(j + 1, k):
            l[i, j] = (mat[i, j] - l[i, :j] @ l[j, :j]) / l[j, j]
    return l


def solve_lt(u, l):
    """U L^-T by forward substitution over the columns"""
    q = np.zeros(u.shape, LD)
    for j in range(l.shape[0]):
        q[:, j] = (u[:, j] - q[:, :j] @ l[j, :j]) / l[j, j]
    return q


def _sym_from_lower(mat):
    low = np.tril(mat)
    return low + np.tril(low, -1).T


def _cond2(mat):
    s = np.linalg.svd(np.asarray(mat, np.float64), compute_uv=False)
    return float(s[0] / s[-1])


def _norm2(a):
    a = np.asarray(a, np.float64)
    return float(np.linalg.norm(a, 2)) if a.size else 0.0


def gram_condition(mat):
    """(kappa_2(M), kappa_2(S M S)) of a symmetric positive definite M, S = diag(M)^-1/2"""
    m = np.asarray(mat, LD)
    s = 1 / np.sqrt(np.diag(m))
    return _cond2(m), _cond2(s[:, None] * m * s[None, :])


class Ref(dict):
    """a reference's results by name"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def ref_b_ortho(u, bu):
    """the pair as given, as the routine's contract has it: M = lower triangle of u^T bu, L = chol(M), Q = u L^-T, BQ = bu L^-T"""
    u, bu = np.asarray(u, LD), np.asarray(bu, LD)
    mat = _sym_from_lower(u.T @ bu)
    l = chol_lower(mat)
    kappa, kappa_eq = gram_condition(mat)
    return Ref(q=solve_lt(u, l), bq=solve_lt(bu, l), kappa=kappa, kappa_eq=kappa_eq, l=l)


def _project(x, bx, p):
    return p - x @ (bx.T @ p) if x.shape[1] else p


def ref_b_ortho_vs_x(x, bx, u):
    """P = (I - X (BX)^T) U (the projection applied three times), then the Euclidean-orthonormal Q of P with a positive-diagonal
    triangular factor: Cholesky-QR plus one re-projection until |Q^T Q - I| < 1e-17.  Every step multiplies by an upper-triangular
    factor with a positive diagonal, so Q is the unique block the reference's ortho_cd sequence converges to."""
    x, bx, u = np.asarray(x, LD), np.asarray(bx, LD), np.asarray(u, LD)
    k = u.shape[1]
    p = u
    for _ in range(3):
        p = _project(x, bx, p)
    q = p
    for _ in range(12):
        g = q.T @ q
        if np.abs(g - np.eye(k)).max() < 1e-17:
            break
        q = _project(x, bx, solve_lt(q, chol_lower(g)))
    else:
        raise RuntimeError("ref_b_ortho_vs_x: the long-double orthonormalisation did not converge")
    pi = _norm2(x) * _norm2(bx) if x.shape[1] else 1.0
    smin = float(np.linalg.svd(np.asarray(p, np.float64), compute_uv=False)[-1])
    return Ref(q=q, p=p, pi=pi, a=_norm2(u) / smin)


def ref_expand(b, x, bx, u):
    """the unique B-orthonormal Q of P with a positive-diagonal factor: long-double B-Cholesky-QR until |Q^T B Q - I| < 1e-17.
    kappa is taken from M = Q1^T B Q1 with Q1 the ref_b_ortho_vs_x result: the matrix the library actually factors."""
    r1 = ref_b_ortho_vs_x(x, bx, u)
    k = u.shape[1]
    q, l1 = r1.q, None
    for _ in range(12):
        g = _sym_from_lower(q.T @ bmul(b, q))
        if l1 is None:
            mat = g
        if np.abs(g - np.eye(k)).max() < 1e-17:
            break
        l = chol_lower(g)
        l1 = l if l1 is None else l1
        q = solve_lt(q, l)
    else:
        raise RuntimeError("ref_expand: the long-double B-orthonormalisation did not converge")
    kappa, kappa_eq = gram_condition(mat)
    l1 = np.eye(k, dtype=LD) if l1 is None else l1
    linv_norm = 1.0 / float(np.linalg.svd(np.asarray(l1, np.float64), compute_uv=False)[-1])
    return Ref(q=q, q1=r1.q, p=r1.p, pi=r1.pi, a=r1.a, kappa=kappa, kappa_eq=kappa_eq, linv_norm=linv_norm)


# ---------------------------------------------------------------------------------------------------------------- metrics
def _tri(n):
    return sp.diags([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1], format="csr")


def metric(name, n):
    """"tri": tridiagonal (-1, 2.5, -1); "scaled": D tri D with D log-spaced over [s^-1/2, s^1/2], s = 1e3, in a seeded random row
    order; "indef": tri with one diagonal entry set to -50 (the error path only).  All sparse and symmetric."""
    if name == "tri":
        return _tri(n)
    if name == "scaled":
        s = 1e3
        d = np.logspace(-0.5 * np.log10(s), 0.5 * np.log10(s), n)[np.random.default_rng(n).permutation(n)]
        return (sp.diags(d) @ _tri(n) @ sp.diags(d)).tocsr()
    if name == "indef":
        b = _tri(n).tolil()
        b[indef_row(n), indef_row(n)] = -50.0
        return b.tocsr()
    raise ValueError(name)


def indef_row(n):
    return n // 3


def operator(n):
    """the second sparse matrix of the expansion tests (A of A x = lambda B x): a symmetric band of five diagonals"""
    i = np.arange(n, dtype=np.float64)
    off1, off2 = 0.3 * np.cos(0.7 * i[:-1]), 0.2 * np.sin(0.3 * i[:-2])
    return sp.diags([off2, off1, 1.0 + 3.0 * i / n, off1, off2], [-2, -1, 0, 1, 2], format="csr")


# ---------------------------------------------------------------------------------------------------------------- blocks
def b_orthonormal(b, x0):
    """X B-orthonormalised in long double (Cholesky-QR, three passes), then rounded to double"""
    x = np.asarray(x0, LD)
    for _ in range(3):
        x = solve_lt(x, chol_lower(x.T @ bmul(b, x)))
    return np.asfortranarray(x.astype(np.float64))


def make_u(kind, rng, b, x, n, k):
    if kind == "random":
        u = rng.standard_normal((n, k))
    elif kind == "near_span":
        u = x @ rng.standard_normal((x.shape[1], k)) + 1e-7 * rng.standard_normal((n, k))
    elif kind == "mix":
        # E W + 1e-3 noise: E selects k rows spread evenly over the sorted diagonal of B, W is a random orthogonal matrix --
        # kappa_2(U^T B U) is large (the spread of the selected diagonal over what the noise adds to it) and M is not diagonal
        rows = np.argsort(b.diagonal(), kind="stable")[np.round(np.linspace(0, n - 1, k)).astype(int)]
        e = np.zeros((n, k)); e[rows, np.arange(k)] = 1.0
        w = np.linalg.qr(rng.standard_normal((k, k)))[0]
        u = e @ w + 1e-3 * rng.standard_normal((n, k))
    elif kind == "colscaled":
        u = rng.standard_normal((n, k)) * np.logspace(-8, 8, k)[None, :]
    elif kind == "rank_deficient":
        u = rng.standard_normal((n, k)); u[:, -1] = u[:, 0] + u[:, 1]
    else:
        raise ValueError(kind)
    return np.asfortranarray(u)


# A block is drawn from a generator seeded by the case's name and, where one is listed here, a draw number.  The CPU test asks that the
# double-precision oracle meets a QUARTER of every bound on every case -- a condition on the inputs, checked without the library.
# The oracle's Gram matrices are sequential sums of n terms (about eps / 2 sqrt(n / 3) = 13 eps at n = 2001), which its Cholesky-QR
# hands on to |Q^T Q - I|: over the draws of one shape that figure lies between 0.12 and 0.36 of the 50 eps bar, on either side of
# the quarter.  The draws listed are the first (0, 1, 2, ...) at which the oracle's worst ratio was below 0.22; nothing the library
# computes went into the choice.
DRAWS = {"n2001_m26_k13_random_scaled": 1, "n2000_m39_k37_random_scaled": 3, "n1500_m16_k48_random_scaled": 1,
         "n2001_m26_k4_random_scaled": 1, "n2001_m26_k16_random_scaled": 1, "n2001_m26_k31_random_scaled": 2,
         "n2001_m26_k32_random_scaled": 2, "n2001_m26_k33_random_scaled": 1, "n2001_m26_k47_random_scaled": 6,
         "n2001_m26_k13_mix_scaled": 1, "n2001_m26_k37_mix_scaled": 3, "n2001_m26_k49_random_scaled": 2}


class Case:
    """one block problem: the metric B, a B-orthonormal X (n x m, m may be 0) with BX = B @ X in double, and U (n x k).  Seeded by
    its own name, built once per process (case()), read only."""

    def __init__(self, n, m, k, kind, metric_name):
        self.n, self.m, self.k, self.kind, self.metric_name = n, m, k, kind, metric_name
        self.name = f"n{n}_m{m}_k{k}_{kind}_{metric_name}"
        draw = DRAWS.get(self.name, 0)
        rng = np.random.default_rng(zlib.crc32((self.name + (f"/{draw}" if draw else "")).encode()))
        self.b = metric(metric_name, n)
        self.x = b_orthonormal(self.b, rng.standard_normal((n, m))) if m else np.zeros((n, 0), order="F")
        self.bx = np.asfortranarray(self.b @ self.x)
        self.u = make_u(kind, rng, self.b, self.x, n, k)
        for a in (self.x, self.bx, self.u):
            a.setflags(write=False)
        self._refs = {}

    def _cached(self, key, make):
        if key not in self._refs:
            self._refs[key] = make()
        return self._refs[key]

    @property
    def bu(self):
        """B @ U in double: the second block of a direct b_ortho call"""
        return self._cached("bu", lambda: np.asfortranarray(self.b @ self.u))

    def ref_b_ortho(self):
        return self._cached("b_ortho", lambda: ref_b_ortho(self.u, self.bu))

    def ref_vs_x(self):
        return self._cached("vs_x", lambda: ref_b_ortho_vs_x(self.x, self.bx, self.u))

    def ref_expand(self):
        return self._cached("expand", lambda: ref_expand(self.b, self.x, self.bx, self.u))


_CASES = {}


def case(n, m, k, kind, metric_name):
    key = (n, m, k, kind, metric_name)
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


# the matrix of tests/test_metric_ortho_gpu.py; the CPU tests run the same cases through the oracle and the host-memory engine
B_ORTHO_KS = (1, 2, 5, 13, 16, 17, 21, 32, 33, 37, 48)
B_ORTHO_GRIDS = ((257, "tri"), (1001, "scaled"), (2000, "scaled"))
B_ORTHO_CASES = [(n, 0, k, kind, met) for k in B_ORTHO_KS for (n, met) in B_ORTHO_GRIDS
                 for kind in ("random", "mix") + (("colscaled",) if k in (13, 17, 37) else ())]
B_ORTHO_FEW_ROWS = (14, 0, 13, "random", "tri")            # n = k + 1: fewer rows than one row tile
B_ORTHO_VIEWS = (1001, 0, 13, "random", "scaled")          # as column views of wider panels between guard columns
B_ORTHO_WIDE = [(1001, 0, 49, "random", "scaled"), (1001, 0, 64, "random", "scaled")]
VS_X_CASES = [(600, 3, 1, "random", "tri"), (1001, 13, 5, "random", "scaled"), (2001, 26, 13, "random", "scaled"),
              (2000, 130, 16, "mix", "scaled"), (1001, 13, 17, "random", "scaled"), (2000, 39, 37, "random", "scaled"),
              (1500, 16, 48, "random", "scaled"), (2001, 52, 11, "near_span", "scaled"), (2000, 74, 37, "near_span", "tri"),
              (3000, 247, 13, "near_span", "tri")]
VS_X_RANK_DEFICIENT = (1000, 26, 13, "rank_deficient", "scaled")
EXPAND_MODE2_KS = (1, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48)
EXPAND_MODE01_KS = (1, 16, 17, 33, 48)
EXPAND_FURTHER = [(2001, 26, 13, "mix", "scaled"), (2001, 26, 37, "mix", "scaled"), (2001, 52, 11, "near_span", "scaled"),
                  (2001, 0, 13, "random", "scaled")]
EXPAND_HOST_STEP = (2001, 26, 49, "random", "scaled")


def expand_width_case(k):
    return (2001, 26, k, "random", "scaled")


EXPAND_CASES = ([(expand_width_case(k), 2) for k in EXPAND_MODE2_KS] +
                [(expand_width_case(k), mode) for k in EXPAND_MODE01_KS for mode in (0, 1)] +
                [(c, mode) for c in EXPAND_FURTHER for mode in (0, 1, 2)] +
                [(EXPAND_HOST_STEP, mode) for mode in (0, 2)])
INDEF_CASE = (1001, 13, 5)
SHIFT = {0: 0.0, 1: 0.25, 2: 0.0}


def indef_blocks():
    """n = 1001, m = 13, k = 5 with the indefinite metric: X is B-orthonormal in `tri` and has no weight on the negative row (so that
    it is B-orthonormal in `indef` as well), U has weight 1 on it: U^T B U has a negative direction and the factorisation must stop"""
    n, m, k = INDEF_CASE
    rng = np.random.default_rng(4711)
    b, row = metric("indef", n), indef_row(n)
    x0 = rng.standard_normal((n, m)); x0[row - 1:row + 2] = 0.0
    x = b_orthonormal(metric("tri", n), x0)
    assert np.all(x[row - 1:row + 2] == 0.0)
    u = 0.01 * rng.standard_normal((n, k)); u[row, :] = 1.0 + np.arange(k)
    return b, x, np.asfortranarray(b @ x), np.asfortranarray(u)


# ---------------------------------------------------------------------------------------------------------------- checkers
def _assert_ratios(what, ratios, limit):
    bad = {key: v for key, v in ratios.items() if not v <= limit}
    assert not bad, f"{what}: error / bound above {limit}: " + ", ".join(f"{key} = {v:.3g}" for key, v in bad.items()) + \
                    "  (all: " + ", ".join(f"{key} = {v:.3g}" for key, v in ratios.items()) + ")"
    return ratios


def _columns(got, want, bound_factor):
    """worst over the columns j of max|got_j - want_j| / (bound_factor max|want_j|)"""
    assert np.all(np.isfinite(got)), "non-finite output"
    err = np.abs(np.asarray(got, LD) - want).max(axis=0)
    return float((err / (bound_factor * np.abs(want).max(axis=0) + TINY)).max())


def _dev_identity(a, b):
    return float(np.abs(np.asarray(a, LD).T @ np.asarray(b, LD) - np.eye(a.shape[1])).max())


def check_b_ortho(q, bq, ref, what="b_ortho", limit=1.0):
    kap = min(ref.kappa, ref.kappa_eq)
    ratios = {"q": _columns(q, ref.q, 64 * EPS * kap), "bq": _columns(bq, ref.bq, 64 * EPS * kap),
              "qtbq": _dev_identity(q, bq) / (64 * EPS * kap)}
    return _assert_ratios(what, ratios, limit)


def check_b_ortho_vs_x(q, ref, c, x_after=None, bx_after=None, what="b_ortho_vs_x", limit=1.0, vs_reference=True):
    """vs_reference = False: the invariants only (a rank-deficient block has no unique answer)"""
    assert np.all(np.isfinite(q)), what + ": non-finite output"
    if x_after is not None:
        assert np.array_equal(x_after, c.x) and np.array_equal(bx_after, c.bx), what + ": X or BX was modified"
    ql = np.asarray(q, LD)
    pi = ref.pi if ref is not None else _norm2(c.x) * _norm2(c.bx)
    ratios = {"qtq": _dev_identity(q, q) / (50 * EPS),
              "bxtq": float(np.abs(np.asarray(c.bx, LD).T @ ql).max()) / (50 * EPS * pi) if c.m else 0.0}
    if vs_reference:
        ratios["q"] = float(np.abs(ql - ref.q).max()) / (64 * EPS * ref.pi * ref.a)
    _assert_ratios(what, ratios, limit)
    assert ratios["qtq"] < limit, (what, ratios)            # (the project's existing bar is a strict one)
    return ratios


def check_expand(q, bq, ref, c, mode=2, a=None, shift=0.0, ax=None, aq=None, h=None, x_after=None, what="expand", limit=1.0):
    """Q and BQ as the expansion left them; modes 0 and 1 with the operator a (scipy.sparse): AQ and h against A @ Q and
    [X Q]^T A [X Q], computed in long double from the returned Q"""
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(bq)), what + ": non-finite output"
    if x_after is not None:
        assert np.array_equal(x_after, c.x), what + ": X was modified"
    kap = min(ref.kappa, ref.kappa_eq)
    ql = np.asarray(q, LD)
    ratios = {"q": _columns(q, ref.q, 64 * EPS * (ref.pi * ref.a + kap)),
              "qtbq": _dev_identity(q, bq) / (64 * EPS * kap),
              "bxtq": float(np.abs(np.asarray(c.bx, LD).T @ ql).max()) / (50 * EPS * ref.pi * ref.linv_norm) if c.m else 0.0}
    if a is not None and mode in (0, 1):
        want_aq = bmul(a, ql) + LD(shift) * ql
        mag_aq = absmul(a, ql) + abs(shift) * np.abs(ql)
        ratios["aq"] = float((np.abs(np.asarray(aq, LD) - want_aq) / (64 * EPS * mag_aq + TINY)).max())
        s = np.hstack([np.asarray(c.x, LD), ql])
        if mode == 0:
            want_h, mag_h, got_h = s.T @ want_aq, np.abs(s).T @ mag_aq, np.asarray(h, LD)
            ratios["h"] = float((np.abs(got_h - want_h) / (64 * EPS * mag_h + TINY)).max())
        else:
            t = np.hstack([np.asarray(ax, LD), want_aq])
            want_h, mag_h = s.T @ t, np.abs(s).T @ np.hstack([np.abs(np.asarray(ax, LD)), mag_aq])
            low = np.tril(np.ones(want_h.shape, bool))
            ratios["h"] = float((np.abs(np.asarray(h, LD) - want_h)[low] / (64 * EPS * mag_h[low] + TINY)).max())
    return _assert_ratios(what, ratios, limit)


def record(path, rows):
    """append `name key=ratio ...` lines to the bookkeeping file"""
    if not path:
        return
    with open(path, "a") as f:
        for name, ratios in rows:
            f.write(name + "  " + "  ".join(f"{key}={v:.3g}" for key, v in sorted(ratios.items())) + "\n")
