"""GPU: examples/fortran_sparse_gen_caller -- a Fortran caller hands a sparse pencil (A to the sparse operator, B to the metric
slot beside it) to the library and calls gen_david_driver and lobpcg_driver(gen_eig = .true.) through the unmodified module
interface with dla_spmm_matvec / dla_spmm_precnd / dla_spmm_bvec in device mode.  Compiled and run the way
tests/test_fortran_caller_gpu.py runs examples/fortran_sparse_caller; eigenvalues against the dense eigensolver on the same pencil
rebuilt here."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def test_fortran_caller_sparse_pencil_on_the_device(tmp_path, ctx):
    if not os.path.exists(FLANG):
        pytest.skip("no Fortran compiler on this box")
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_sparse_gen_caller", "sparse_gen_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "sparse_gen_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    # the caller's pencil (its header): a_ii = i + 1, a_ij = 1 / (i + j) for |i - j| <= 6 (1-based);
    # b_ii = 1 + 0.25 sin^2(0.003 i), b_ij = 0.15 / k cos(0.01 min(i, j)) for k = |i - j| = 1, 2 (0-based)
    n, half, t = 4000, 6, 6
    idx = np.arange(1.0, n + 1.0)
    a = sp.diags([1.0 / (idx[:-k] + idx[k:]) for k in range(1, half + 1)], list(range(1, half + 1)), shape=(n, n))
    a = (a + a.T + sp.diags(idx + 1.0)).toarray()
    i = np.arange(n, dtype=np.float64)
    b = sp.diags([0.15 / k * np.cos(0.01 * i[:n - k]) for k in (1, 2)], [1, 2], shape=(n, n))
    b = (b + b.T + sp.diags(1.0 + 0.25 * np.sin(0.003 * i) ** 2)).toarray()
    want = sl.eigh(a, b, eigvals_only=True, subset_by_index=[0, t - 1])
    for tag in ("SPARSE GEN_DAVIDSON", "SPARSE GEN_LOBPCG"):
        m1 = re.search(tag + r" ok/iterations:\s+T\s+(\d+)", out)
        assert m1 and 0 < int(m1.group(1)) < 300, out
        vals = [float(v) for v in re.search(tag + r" eig:(.*)", out).group(1).split()]
        assert np.allclose(vals, want, rtol=1e-9, atol=0), (tag, vals, want)
        res, orth = [float(v) for v in re.search(tag + r" max residual, max \|x\^T B x - 1\|:(.*)", out).group(1).split()]
        assert res < 1e-6 and orth < 1e-10, (tag, res, orth)
