"""GPU: examples/fortran_sparse_nonsym_caller -- a Fortran caller builds a sparse non-symmetric matrix with a known real spectrum
(A = D S D^-1, S symmetric and banded, D = diag(exp(t_i)) with |t_i| <= 0.01), hands its CSR arrays over once with
dla_spmm_setup_csr_fmt, prepares the transposed index and calls nonsym_driver through the module interface with side = 'c' and
dla_spmm_matvec / dla_spmm_matvec_t / dla_spmm_precnd in device mode.  Compiled and run the way
tests/test_fortran_nonsym_caller_gpu.py runs its example, under the same assertions; the eigenvalues against those of S."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_nonsym_sparse_gpu import example_matrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLANG = "/opt/rocm/lib/llvm/bin/flang"


def test_fortran_caller_of_nonsym_driver_with_one_stored_sparse_matrix(tmp_path, ctx):
    assert os.path.exists(FLANG), "the Fortran compiler the library itself is built with is missing"
    lib = os.path.join(ROOT, "diaglib_amd", "lib")
    srcs = [os.path.join(ROOT, "diaglib_amd", "fortran", "real_precision.f90"),
            os.path.join(ROOT, "diaglib_amd", "fortran", "diaglib.f90"),
            os.path.join(ROOT, "examples", "fortran_sparse_nonsym_caller", "sparse_nonsym_caller.f90")]
    objs = []
    for s in srcs:
        o = str(tmp_path / (os.path.basename(s) + ".o"))
        subprocess.run([FLANG, "-O2", "-c", s, "-o", o, "-module-dir", str(tmp_path), "-I", str(tmp_path)], check=True)
        objs.append(o)
    exe = str(tmp_path / "sparse_nonsym_caller.exe")
    subprocess.run([FLANG, "-o", exe] + objs + ["-L" + lib, "-ldiaglib_amd", "-Wl,-rpath," + lib], check=True)
    n, t, tol = 300, 4, 1e-9
    want = np.linalg.eigvalsh(example_matrix(n)[1])[:t]
    outs = {}
    for mode in ("device", "host"):
        p = subprocess.run([exe, str(n)] + (["host"] if mode == "host" else []), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stdout + p.stderr
        out = outs[mode] = p.stdout
        m1 = re.search(r"NONSYM ok/iterations/matvec columns:\s+T\s+(\d+)\s+(\d+)", out)
        assert m1 and 0 < int(m1.group(1)) < 200, out
        vals = [float(v) for v in re.search(r"NONSYM eig:(.*)", out).group(1).split()]
        # the eigenvector matrix D Q has condition number at most e^0.02 (Bauer-Fike, rms residual below tol)
        assert np.abs(np.array(vals) - want).max() <= np.exp(0.02) * np.sqrt(n) * tol, (vals, want)
        assert float(re.search(r"NONSYM max \|L\^T R - I\|:\s*(\S+)", out).group(1)) <= n * np.finfo(float).eps
        assert re.search(r"NONSYM mode/n/seconds:\s+" + mode + r"\s+300", out), out
    cols = [int(re.search(r"columns:\s+T\s+\d+\s+(\d+)", outs[m]).group(1)) for m in ("device", "host")]
    assert abs(cols[0] - cols[1]) <= 8, cols          # the same algorithm on another summation order: at most one block apart
