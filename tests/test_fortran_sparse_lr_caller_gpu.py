"""GPU: examples/fortran_sparse_lr_caller -- a Fortran caller hands the four sparse parts of a linear-response pencil to the library
(dla_spmm_setup_lr_csr) and calls caslr_eff_driver and caslr_driver through the unmodified module interface with dla_spmm_apbmul /
ambmul / spdmul / smdmul and dla_spmm_lrprec2 / lrprec1 in device mode.  Compiled and run the way tests/test_fortran_caller_gpu.py
runs its examples (a fresh child process under a time limit); eigenvalues against scipy.linalg.eig of the dense pencil rebuilt
here, within ten times the error of the same drivers in host-callback mode on the same matrices (at most 1e-8 relative)."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from spmm_lr_cases import dense_roots, positive_definite, solve_host_mode, tolerance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def example_pencil(n=300):
    """the caller's matrices (its header), 1-based i, j"""
    i = np.arange(1, n + 1)
    ii, jj = np.meshgrid(i, i, indexing="ij")
    k = np.abs(ii - jj)
    e = np.where((k >= 1) & (k <= 3), 0.05 * np.sin((ii + jj).astype(float)), 0.0)
    s = np.where((k >= 1) & (k <= 2), 0.0005 * np.cos((ii + jj).astype(float)), 0.0) + np.diag(1.0 + 0.5 / (1 + i % 7))
    d = np.where((k >= 1) & (k <= 2), 0.02 * np.sin(0.3 * (ii + jj)) * np.sign(jj - ii), 0.0)
    mats = {"apb": np.diag(i + 5.0) + e, "amb": np.diag(i + 2.0) + 0.2 * e, "spd": s + d, "smd": s - d}
    return {p: sp.csr_matrix(v) for p, v in mats.items()}


def test_fortran_caller_sparse_linear_response_on_the_device(tmp_path, ctx):
    """Measured on an MI355X: the host-callback solves of this pencil are 3.18e-14 (caslr_eff_driver) and 3.21e-14 (caslr_driver) from
    the dense solve, so the printed eigenvalues are held to 3.2e-13; they are 3.20e-14 from it."""
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_sparse_lr_caller", "sparse_lr_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "sparse_lr_caller.exe")
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
    for tag, trad in (("SPARSE CASLR_EFF", False), ("SPARSE CASLR", True)):
        eig_h, ok_h, info_h = solve_host_mode(ctx, mats, trad, t, m, 100, 1e-9, 20, guess=guess)
        assert ok_h, info_h
        host_err, allowed = tolerance(eig_h, want)
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and abs(int(m1.group(1)) - info_h["iters"]) <= 1, (out, info_h)
        vals = np.array([float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()])
        err = float(np.abs(vals / want - 1.0).max())
        print(f"{tag}: host-callback error {host_err:.3e}, error of the printed eigenvalues {err:.3e}, allowed {allowed:.3e}")
        assert err <= allowed, (tag, vals, want, err, allowed)
        res = float(re.search(tag + r" max residual:(.*)", out).group(1))
        assert res < 1e-7, (tag, res)
