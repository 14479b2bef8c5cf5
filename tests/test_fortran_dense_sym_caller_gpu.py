"""GPU: examples/fortran_dense_sym_caller -- a Fortran caller builds the reference harness' dense matrix and a dense SPD metric,
hands over one triangle of each with dla_dense_setup_sym (operator 'L', metric 'U'; the other strict triangle holds -huge()) and
calls davidson_driver, lobpcg_driver and gen_david_driver through the unmodified module interface with dla_dense_matvec /
dla_dense_precnd / dla_dense_bvec in device mode.  Compiled and run the way tests/test_fortran_dense_caller_gpu.py runs its example;
eigenvalues against the dense eigensolvers on the matrices rebuilt here."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def test_fortran_caller_symmetric_dense_matrices_stored_as_triangles(tmp_path, ctx):
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_dense_sym_caller", "dense_sym_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "dense_sym_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    # the caller's matrices (its header): a_ii = i + 1, a_ij = 1 / (i + j); b_ii = 1 + 0.25 sin^2(0.003 (i - 1)),
    # b_ij = 0.05 / (i - j)^2 (1-based)
    n, t = 1000, 6
    idx = np.arange(1.0, n + 1.0)
    a = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a, idx + 1.0)
    with np.errstate(divide="ignore"):
        b = 0.05 / (idx[:, None] - idx[None, :]) ** 2
    np.fill_diagonal(b, 1.0 + 0.25 * np.sin(0.003 * (idx - 1.0)) ** 2)
    plain = np.linalg.eigvalsh(a)[:t]
    gen = sl.eigh(a, b, eigvals_only=True, subset_by_index=[0, t - 1])
    for tag, want in (("DENSE SYM DAVIDSON", plain), ("DENSE SYM LOBPCG", plain), ("DENSE SYM GEN_DAVIDSON", gen)):
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and 0 < int(m1.group(1)) < 300, out
        vals = [float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()]
        assert np.allclose(vals, want, rtol=1e-9, atol=0), (tag, vals, want)
        res, orth = [float(v) for v in re.search(tag + r" max residual, max \|x\^T B x - 1\|:(.*)", out).group(1).split()]
        assert res < 1e-6 and orth < 1e-10, (tag, res, orth)
