#!/usr/bin/env python3
"""Golden fixtures for nonsym_driver, from the UNMODIFIED reference (reference diaglib.f90:2252-2943; oracle/_ref built by
`make -C oracle ref`).

    python tests/golden/make_golden_nonsym.py      ->  tests/golden/reference_nonsym_fixtures.npz

Data only.  The cases, the matrix and the guess are those of tests/nonsym_cases.py; the reference is called through its module symbol
(every argument by reference, the hidden length of `side` as a trailing 64-bit 1), one child process per case because it can
`stop`.  Per case <name> the file holds
    <name>__u, <name>__v          the factors of the nilpotent N (so that the tests do not depend on a generator's stream)
    <name>__eig                   the eigenvalues the reference returned (n_max of them)
    <name>__cols                  columns it handed to matvec and to matvec_l
    <name>__eig_err               max |eig - truth| over the n_targ wanted roots, truth = eigvalsh(A0)
    <name>__biorth                max |L^T R - I|               (side c; nan otherwise)
    <name>__subres                ||A R - R (L^T A R)||_F / sqrt(n)   (side c with n_targ = n_max; nan otherwise)
    <name>__seed                  the seed of the factors
A case is kept only when the reference returns ok and reaches the lowest n_targ eigenvalues of A0 to 1e-9; otherwise the next
seed is tried (and recorded).
"""
import json
import os
import subprocess
import sys
import tempfile

os.environ.setdefault("OMP_NUM_THREADS", "8")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import nonsym_cases as nc  # noqa: E402

CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import nonsym_cases as nc
from oracle.pyoracle import REF_SO
spec = json.loads(%r)
n, n_targ, n_max, max_dav, tol, side, t = spec['case']
u, v = nc.factors(n, spec['seed'])
a, a0 = nc.matrix(n, t, u, v)
at = np.asfortranarray(a.T)
prec = nc.mprec(np.diag(a).copy())
cols = [0, 0]
c_ip, c_dp = C.POINTER(C.c_int), C.POINTER(C.c_double)

def block(p, n, m):
    return np.ctypeslib.as_array(p, (m, n)).T

def mv(pn, pm, px, pax):
    cols[0] += pm[0]
    block(pax, pn[0], pm[0])[:, :] = a @ block(px, pn[0], pm[0])

def mvl(pn, pm, px, pax):
    cols[1] += pm[0]
    block(pax, pn[0], pm[0])[:, :] = at @ block(px, pn[0], pm[0])

def pc(pn, pm, pf, px, ppx):
    block(ppx, pn[0], pm[0])[:, :] = prec(pf[0], block(px, pn[0], pm[0]))

MV = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp)
PC = C.CFUNCTYPE(None, c_ip, c_ip, c_dp, c_dp, c_dp)
f_mv, f_mvl, f_pc = MV(mv), MV(mvl), PC(pc)
lib = C.CDLL(REF_SO, mode=C.RTLD_GLOBAL)
drv = getattr(lib, "_QMdiaglibPnonsym_driver")
drv.restype = None
drv.argtypes = [C.c_void_p] * 16 + [C.c_int64]
i4 = lambda x: C.byref(C.c_int(x))
f8 = lambda x: C.byref(C.c_double(x))
eig = np.zeros(n_max)
r = nc.guess(n, n_max); l = nc.guess(n, n_max)
ok = C.c_int(0)
drv(i4(0), i4(n), i4(n_targ), i4(n_max), i4(nc.MAX_ITER), f8(tol), i4(max_dav), f8(0.0),
    C.cast(f_mv, C.c_void_p), C.cast(f_mvl, C.c_void_p), C.cast(f_pc, C.c_void_p),
    eig.ctypes.data, r.ctypes.data, l.ctypes.data, C.c_char_p(side.encode()), C.byref(ok), 1)
sys.stdout.flush()
tr = nc.truth(a0)
both = side == 'c'
np.savez(spec['out'], u=u, v=v, eig=eig, cols=np.array(cols), ok=bool(ok.value & 1),
         eig_err=np.abs(eig[:n_targ] - tr[:n_targ]).max(),
         biorth=nc.biorth_error(l, r) if both else np.nan,
         subres=nc.subspace_residual(a, l, r) if both and n_targ == n_max else np.nan)
"""


def run_case(case, seed, tmp):
    out = os.path.join(tmp, nc.case_name(case) + f"_{seed}.npz")
    spec = json.dumps(dict(case=list(case), seed=seed, out=out))
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), spec)], capture_output=True, text=True)
    if p.returncode != 0 or not os.path.exists(out):
        print(f"  {nc.case_name(case)} seed {seed}: the reference ended with status {p.returncode}\n{p.stdout[-400:]}{p.stderr[-400:]}")
        return None
    return dict(np.load(out))


def main():
    store = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in nc.CASES + [nc.RESTART_CASE]:
            for seed in (nc.SEED, 2):
                res = run_case(case, seed, tmp)
                if res is not None and bool(res["ok"]) and float(res["eig_err"]) <= 1e-9:
                    break
                print(f"  {nc.case_name(case)}: seed {seed} not kept")
            else:
                raise SystemExit(f"no seed gives a usable reference run for {nc.case_name(case)}")
            name = nc.case_name(case)
            for key in ("u", "v", "eig", "cols", "eig_err", "biorth", "subres"):
                store[f"{name}__{key}"] = res[key]
            store[f"{name}__seed"] = np.array(seed)
            print(f"{name}: seed {seed} cols {res['cols']} eig_err {float(res['eig_err']):.2e} "
                  f"biorth {float(res['biorth']):.2e} subres {float(res['subres']):.2e}")
    np.savez_compressed(os.path.join(HERE, "reference_nonsym_fixtures.npz"), **store)


if __name__ == "__main__":
    main()
