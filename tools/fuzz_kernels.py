#!/usr/bin/env python3
"""Randomised shape sweep of the block kernels.  The panel products, the update and the Ritz sweep go through the guarded checkers
of tests/dense_ref.py (long-double references, sentinel columns around the outputs, NaN columns around the inputs, NaN rows under the
coefficient blocks); the Gram matrices against the oracle (float64 dot-product bound).
    python tools/fuzz_kernels.py [cases] [seed]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from diaglib_amd import capi  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402
import dense_ref as D  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
EPS = np.finfo(np.float64).eps
ctx = capi.Context()
o = Oracle()
bad = 0
for it in range(cases):
    n = int(rng.choice([rng.integers(1, 70), rng.integers(70, 700), rng.integers(700, 9000)]))
    if rng.random() < 0.6:
        n += n % 2                                  # mostly even n (16-byte paths)
    l = int(rng.choice([rng.integers(1, 17), rng.integers(17, 130), rng.integers(130, 300)]))
    k = int(rng.choice([rng.integers(1, 17), rng.integers(17, 49)]))
    x = np.asfortranarray(rng.standard_normal((n, l)))
    u = np.asfortranarray(rng.standard_normal((n, k)))
    px, pu = ctx.panel(x), ctx.panel(u)
    errs = {}
    got = ctx.gram(px, pu)
    errs["gram"] = np.max(np.abs(got - o.gemm_tn(x, u)) / (64 * EPS * (np.abs(x).T @ np.abs(u)) + 1e-300))
    if l <= 300:
        gl = ctx.gram_lower(px, ctx.panel(x[:, ::-1].copy(order="F")))
        want = o.gemm_tn(x, np.asfortranarray(x[:, ::-1]))
        low = np.tril(np.ones((l, l), bool))
        errs["gram_lower"] = np.max((np.abs(gl - want) / (64 * EPS * (np.abs(x).T @ np.abs(x[:, ::-1])) + 1e-300))[low])
    pad = int(rng.integers(0, 4))
    off = [None, None, None, "x", "z"][int(rng.integers(0, 5))]
    m = min(k, 48)
    nres = int(rng.integers(0, m + 1))
    skip = (rng.random(m) < 0.3).astype(np.int32)
    some = n > 2000                                 # (long panels: the long-double references on every 97th row and the last 300)
    for name, check in (("gemm", lambda: D.check_product(ctx, rng, n, l, k, "gemm", off=off, pad=pad, sample=some)[1]),
                        ("update", lambda: D.check_product(ctx, rng, n, l, k, "update", off=off, pad=pad, sample=some)[1]),
                        ("ritz", lambda: D.check_ritz(ctx, rng, n, l, m, evec=bool(rng.random() < 0.7), avy=bool(rng.random() < 0.5), n_res=nres,
                                                      skip=skip, ypad=pad, sample=some)["ratio"])):
        try:
            errs[name] = check()
        except AssertionError as e:
            errs[name] = float("inf")
            print("FAIL", name, str(e)[:400], flush=True)
    worst = max(errs.values())
    if worst > 1.0 or not np.isfinite(worst):
        bad += 1
        print("FAIL", dict(n=n, l=l, k=k, nres=nres, pad=pad, off=off), {a: float(b) for a, b in errs.items()}, flush=True)
    for p in (px, pu):
        p.free()
print(f"{cases} cases, {bad} failures", flush=True)
sys.exit(1 if bad else 0)
