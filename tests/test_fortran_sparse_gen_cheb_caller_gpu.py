"""GPU: examples/fortran_sparse_gen_cheb_caller -- a Fortran caller hands the stiffness / mass pair (diffusion(32, 1e3), mass(32)) to
the sparse operator and its metric, configures the Chebyshev preconditioner and calls gen_david_driver and lobpcg_driver
(gen_eig = .true.) through the unmodified module interface with dla_spmm_matvec / dla_spmm_precnd_cheb_pencil / dla_spmm_bvec in
device mode.  Compiled and run the way tests/test_fortran_sparse_cheb_jacobi_caller_gpu.py runs its example; eigenvalues against the
dense eigensolver on the pencil rebuilt here."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg

import cheb_pencil_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def test_fortran_caller_pencil_chebyshev_preconditioner_on_the_device(tmp_path, ctx):
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_sparse_gen_cheb_caller", "sparse_gen_cheb_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "sparse_gen_cheb_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    a, b = cheb_pencil_ref.diffusion(32, 1e3), cheb_pencil_ref.mass(32)
    want = scipy.linalg.eigh(a.toarray(), b.toarray(), eigvals_only=True)[:4]
    for tag in ("CHEB-PENCIL GEN_DAVIDSON", "CHEB-PENCIL GEN_LOBPCG"):
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and 0 < int(m1.group(1)) <= 150, out
        vals = [float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()]
        assert np.allclose(vals, want, rtol=1e-9, atol=0.0), (tag, vals, want)
        res = float(re.search(tag + r" max residual:(.*)", out).group(1))
        assert res < 1e-6 * max(1.0, want.max()), (tag, res)
