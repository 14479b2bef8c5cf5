"""GPU: examples/fortran_dense_lr_caller -- a Fortran caller hands the dense A, B, S and D of a linear-response pencil to the library
in two calls (dla_dense_setup_lr_pair) and calls caslr_eff_driver and caslr_driver through the unmodified module interface with
dla_dense_apbmul / ambmul / spdmul / smdmul and dla_dense_lrprec2 / lrprec1 in device mode.  Compiled and run the way
tests/test_fortran_sparse_lr_caller_gpu.py runs its example (a fresh child process under a time limit); eigenvalues against
scipy.linalg.eig of the dense pencil rebuilt here, within ten times the error of the same drivers in host-callback mode on the same
matrices (at most 1e-8 relative)."""
import os
import re
import subprocess

import numpy as np
import pytest

from spmm_lr_cases import dense_roots, positive_definite, solve_host_mode, tolerance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


class _Dense(np.ndarray):
    """a dense matrix with the two methods tests/spmm_lr_cases.py asks of a sparse one"""

    def toarray(self):
        return np.asarray(self)

    def diagonal(self):
        return np.diag(np.asarray(self)).copy()


def example_pencil(n=300):
    """the caller's matrices (its header), 1-based i, j: the parts as numpy forms them from A, B, S and D"""
    i = np.arange(1, n + 1)
    ii, jj = np.meshgrid(i, i, indexing="ij")
    off = ii != jj
    a = np.where(off, 0.12 / (ii + jj), 0.0) + np.diag(i + 3.5)
    b = np.where(off, 0.08 / (ii + jj), 0.0) + np.diag(np.full(n, 1.5))
    s = np.where(off, 0.01 * np.cos((ii + jj).astype(float)) / (1 + np.abs(ii - jj)), 0.0) + np.diag(1.0 + 0.5 / (1 + i % 7))
    d = np.where(off, 0.02 * np.sin(0.3 * (ii + jj)) * np.sign(jj - ii) / (1 + np.abs(ii - jj)), 0.0)
    mats = {"apb": a + b, "amb": a - b, "spd": s + d, "smd": s - d}
    return {p: np.asfortranarray(v).view(_Dense) for p, v in mats.items()}


def test_fortran_caller_dense_linear_response_on_the_device(tmp_path, ctx):
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_dense_lr_caller", "dense_lr_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "dense_lr_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    n, t, m = 300, 4, 8
    mats = example_pencil(n)
    assert positive_definite(mats)
    r, j = np.arange(1, 2 * n + 1)[:, None], np.arange(1, m + 1)[None, :]
    guess = np.sin(0.37 * (r * j) + j)                  # the caller's guess
    guess[40:] *= 1e-2
    guess = np.asfortranarray(guess)
    want = dense_roots(mats, t)
    for tag, trad in (("DENSE CASLR_EFF", False), ("DENSE CASLR", True)):
        eig_h, ok_h, info_h = solve_host_mode(ctx, mats, trad, t, m, 100, 1e-9, 20, guess=guess)
        assert ok_h, info_h
        host_err, allowed = tolerance(eig_h, want)
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and abs(int(m1.group(1)) - info_h["iters"]) <= 1, (out, info_h)
        vals = np.array([float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()])
        err = float(np.abs(vals / want - 1.0).max())
        print(f"{tag}: host-callback error {host_err:.3e} ({info_h['iters']} iterations), error of the printed eigenvalues {err:.3e} "
              f"({m1.group(1)} iterations), allowed {allowed:.3e}")
        assert err <= allowed, (tag, vals, want, err, allowed)
        res = float(re.search(tag + r" max residual:(.*)", out).group(1))
        assert res < 1e-7, (tag, res)
