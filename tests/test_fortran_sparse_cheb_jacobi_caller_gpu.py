"""GPU: examples/fortran_sparse_cheb_jacobi_caller -- a Fortran caller hands diffusion(32, 1e3) (coefficients over three orders of
magnitude) to the sparse operator, configures the Chebyshev preconditioner and calls davidson_driver and lobpcg_driver through the
unmodified module interface with dla_spmm_matvec / dla_spmm_precnd_cheb_jacobi in device mode.  Compiled and run the way
tests/test_fortran_sparse_cheb_caller_gpu.py runs its example; eigenvalues against the dense eigensolver on the matrix rebuilt here."""
import os
import re
import subprocess

import numpy as np
import pytest

import cheb_jacobi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def test_fortran_caller_scaled_chebyshev_preconditioner_on_the_device(tmp_path, ctx):
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_sparse_cheb_jacobi_caller", "sparse_cheb_jacobi_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "sparse_cheb_jacobi_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    want = np.linalg.eigvalsh(cheb_jacobi_ref.diffusion(32, 1e3).toarray())[:4]
    for tag in ("CHEB-JACOBI DAVIDSON", "CHEB-JACOBI LOBPCG"):
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and 0 < int(m1.group(1)) <= 150, out
        vals = [float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()]
        assert np.abs(np.array(vals) - want).max() <= 1e-9, (tag, vals, want)
        res = float(re.search(tag + r" max residual:(.*)", out).group(1))
        assert res < 1e-6, (tag, res)
