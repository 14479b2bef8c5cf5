"""CPU: dense_pack_pair in diaglib_amd/csrc/hip_plans.h, the host twin of dense_pack_pair_kernel (the contract: include/diaglib_amd.h,
dla_dense_setup_lr_pair).

tests/dense_lr_layout_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_dense_operator_layout.py builds its driver).  The two copies it forms from p and q must equal, element by element and
padding included, what dense_pack stores for the arrays p + q and p - q formed here by NumPy (one rounded addition, one rounded
subtraction per element), and the two diagonals must equal too.  The sources have independent leading dimensions ldp = n + 3 and
ldq = n + 5; their rows beyond n hold NaN, which must reach neither a copy nor a diagonal."""
import os
import subprocess

import numpy as np
import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "dense_lr_layout_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h")]
EXE = os.path.join(hostsim.BUILD, "dense_lr_layout_driver")
SIZES = [1, 15, 16, 17, 33]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("dense_lr")

    def run(p, q):
        n = p.shape[0]
        ldp, ldq = n + 3, n + 5
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        hp, hq = np.full((ldp, n), np.nan, order="F"), np.full((ldq, n), np.nan, order="F")
        hp[:n, :], hq[:n, :] = p, q
        with open(fin, "wb") as f:
            np.array([n, ldp, ldq], np.int64).tofile(f)
            for held in (hp, hq, np.asfortranarray(p + q), np.asfortranarray(p - q)):
                held.T.tofile(f)                                  # column-major bytes
        r = subprocess.run([EXE, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
        n_pad = int(np.frombuffer(raw, np.int64, 1)[0])
        at, out = 8, {}
        for name, count in (("pair_sum", n_pad * n_pad), ("pair_dif", n_pad * n_pad), ("pair_sum_diag", n), ("pair_dif_diag", n),
                            ("pack_sum", n_pad * n_pad), ("pack_dif", n_pad * n_pad), ("pack_sum_diag", n), ("pack_dif_diag", n)):
            out[name] = np.frombuffer(raw, np.uint64, count, at)     # bits: -0.0 and +0.0 differ, NaN equals itself
            at += 8 * count
        assert at == len(raw)
        return n_pad, out
    return run


@pytest.mark.parametrize("n", SIZES)
def test_the_pair_packing_stores_what_dense_pack_stores_for_the_sum_and_the_difference(driver, n):
    rng = np.random.default_rng(500 + n)
    p, q = rng.standard_normal((n, n)), rng.standard_normal((n, n)) * 1e-3      # (p + q rounds: the sum is not exact)
    q[0, 0] = p[0, 0]                                                           # an exact 0.0 as a difference
    n_pad, out = driver(p, q)
    assert n_pad == -(-n // 16) * 16
    for kind in ("sum", "dif"):
        assert np.array_equal(out["pair_" + kind], out["pack_" + kind]), (n, kind)
        assert np.array_equal(out["pair_" + kind + "_diag"], out["pack_" + kind + "_diag"]), (n, kind)
    assert np.array_equal(out["pair_sum_diag"].view(np.float64), np.diag(p) + np.diag(q))
    assert np.array_equal(out["pair_dif_diag"].view(np.float64), np.diag(p) - np.diag(q))
    # the padding is +0.0 and nothing is left of the poison or of the NaN rows: the stored values are those of the array, as a multiset
    for kind, want in (("sum", p + q), ("dif", p - q)):
        stored = out["pair_" + kind]
        assert int((stored == 0).sum()) >= n_pad * n_pad - n * n and np.all(np.isfinite(stored.view(np.float64)))
        padded = np.concatenate([want.ravel(), np.zeros(n_pad * n_pad - n * n)])
        assert np.array_equal(np.sort(stored.view(np.float64)), np.sort(padded)), (n, kind)
