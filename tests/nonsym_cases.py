"""Shared inputs of the nonsym_driver tests (numpy only).

The matrix: A0 is the reference harness' test matrix, a_ii = i + 1, a_ij = 1 / (i + j) (1-based, reference main.f90:312-315), and
A = (I - N) A0 (I + N) with a nilpotent N = U V^T, N^2 = 0, scaled to ||N||_2 = t: U is n x 3 standard normal, V = W - Q Q^T W for a
second n x 3 standard normal W and Q = qr(U), so V^T U = 0.  (I + N)^-1 = I - N, so A has exactly the spectrum of A0 -- the truth is
eigvalsh(A0) -- with right eigenvectors (I - N) x0 and left ones (I + N)^T x0: the eigenvector matrix has condition number at most
(1 + t)^2.  The guess is e_1 .. e_n_max on both sides, the preconditioner the harness' mprec (main.f90:146-171) on diag(A).

The tests read U and V from tests/golden/reference_nonsym_fixtures.npz (so that they do not depend on a generator's stream); the
fixture's generator makes them with `factors` below.
"""
import numpy as np

# (n, n_targ, n_max, max_dav, tol, side, t)
CASES = [
    (301, 4, 4, 3, 1e-9, "c", 0.05),
    (301, 6, 6, 2, 1e-9, "c", 0.1),
    (96, 3, 5, 10, 1e-8, "c", 0.05),
    (301, 5, 8, 3, 1e-9, "c", 0.1),
    (301, 5, 8, 3, 1e-9, "r", 0.2),
    (200, 4, 4, 10, 1e-8, "l", 0.05),
    (130, 2, 3, 4, 1e-9, "c", 0.2),
]
# this project's addition to the list: the basis (10 blocks of 2) fills up before the roots converge, so both passes restart
RESTART_CASE = (301, 2, 2, 2, 1e-12, "c", 0.2)
MAX_ITER = 200
SEED = 1


def case_name(case) -> str:
    n, n_targ, n_max, max_dav, tol, side, t = case
    return f"n{n}_t{n_targ}_m{n_max}_d{max_dav}_{side}_{t}"


def harness_matrix(n: int) -> np.ndarray:
    i = np.arange(1, n + 1, dtype=np.float64)
    a = 1.0 / (i[:, None] + i[None, :])
    a[np.arange(n), np.arange(n)] = i + 1.0
    return a


def factors(n: int, seed: int = SEED):
    """U and the unscaled V of N = U V^T (V^T U = 0)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    w = rng.standard_normal((n, 3))
    q, _ = np.linalg.qr(u)
    return u, w - q @ (q.T @ w)


def matrix(n: int, t: float, u: np.ndarray, v: np.ndarray):
    """(A, A0) for the factors u, v and ||N||_2 = t"""
    a0 = harness_matrix(n)
    nil = u @ v.T
    nil *= t / np.linalg.norm(nil, 2)
    eye = np.eye(n)
    return np.asfortranarray((eye - nil) @ a0 @ (eye + nil)), a0


def truth(a0: np.ndarray) -> np.ndarray:
    return np.linalg.eigvalsh(a0)


def guess(n: int, n_max: int) -> np.ndarray:
    g = np.zeros((n, n_max), order="F")
    g[np.arange(n_max), np.arange(n_max)] = 1.0
    return g


def mprec(diag: np.ndarray):
    """the harness' preconditioner as a Python callback (fac, x) -> px"""
    def apply(fac, x):
        d = diag + fac
        safe = np.abs(d) > 1.0e-5
        return np.where(safe[:, None], x / np.where(safe, d, 1.0)[:, None], x)
    return apply


def rms_residuals(op: np.ndarray, vec: np.ndarray, eig: np.ndarray, k: int) -> np.ndarray:
    """||op x_j - eig_j x_j||_2 / sqrt(n), j < k, for the vectors as returned (norm 1 up to rounding)"""
    r = op @ vec[:, :k] - vec[:, :k] * eig[:k]
    return np.linalg.norm(r, axis=0) / np.sqrt(op.shape[0])


def biorth_error(lvec: np.ndarray, rvec: np.ndarray) -> float:
    return float(np.abs(lvec.T @ rvec - np.eye(rvec.shape[1])).max())


def subspace_residual(a: np.ndarray, lvec: np.ndarray, rvec: np.ndarray) -> float:
    """||A R - R (L^T A R)||_F / sqrt(n)"""
    ar = a @ rvec
    return float(np.linalg.norm(ar - rvec @ (lvec.T @ ar)) / np.sqrt(a.shape[0]))
