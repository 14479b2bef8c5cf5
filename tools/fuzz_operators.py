#!/usr/bin/env python3
"""Randomised sweep of the device-resident operators and preconditioners against their definitions in longdouble: the ELLPACK product
and its diagonal preconditioner on ragged, unsorted CSR input (unsharded and one-shard setup), the six sample operators, dla_synth_precnd,
lrprec 1 / 2, the counter-based generator, axpy / nrm2.  Generators, references and bounds are those of tests/test_operators_gpu.py.
    python tools/fuzz_operators.py [cases] [seed]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from diaglib_amd import capi  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402
import test_operators_gpu as T  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
ctx = capi.Context()
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
o = Oracle()
FAMILIES = ["spmm", "spmm_precnd", "synth_precnd", "synth_apply", "synth_lrprec", "random_fill", "axpy_nrm2"]
bad = 0
for it in range(cases):
    fam = FAMILIES[it % len(FAMILIES)]
    n = int(rng.choice([rng.integers(1, 70), rng.integers(70, 700), rng.integers(700, 20001)]))
    if rng.random() < 0.5:
        n += n % 2                                  # half of the cases on even n (16-byte paths)
    m = int(rng.choice([rng.integers(1, 9), rng.integers(1, 65)]))
    w_max = int(rng.choice([rng.integers(1, 9), rng.integers(9, 34), rng.integers(34, 81)]))
    row0 = int(rng.choice([0, 1, 12_345, T.ROW0_FAR, 5 * 10 ** 9]))
    n_global = row0 + n + int(rng.integers(0, 1000))
    case = dict(family=fam, n=n, m=m)
    try:
        if fam == "spmm":
            m = max(1, min(m, 2_000_000 // (n * w_max)))            # (the longdouble reference holds nnz x m products)
            case.update(m=m, w_max=w_max, sharded=bool(rng.random() < 0.3))
            T.check_spmm(ctx, rng, n, w_max, m, sharded=case["sharded"])
        elif fam == "spmm_precnd":
            m = min(m, 16)
            case.update(m=m, w_max=w_max)
            T.check_spmm_precnd(ctx, rng, n, w_max, m)
        elif fam == "synth_precnd":
            kw = dict(row0=row0, n_global=n_global, x_offset=8 * int(rng.random() < 0.2), px_offset=8 * int(rng.random() < 0.2))
            if rng.random() < 0.5:
                kw["guard_row"] = int(rng.integers(0, n))
            else:
                kw["fac"] = float(rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 3.0))
            case.update(kw)
            T.check_synth_precnd(ctx, o, rng, n, m, **kw)
        elif fam == "synth_apply":
            names = tuple(rng.choice(list(T.SYNTH_KINDS), 2, replace=False))
            case.update(row0=row0, kinds=names)
            T.check_synth_apply(ctx, o, rng, n, m, row0=row0, n_global=n_global, names=names)
        elif fam == "synth_lrprec":
            case.update(row0=row0)
            T.check_synth_lrprec(ctx, o, rng, n, m, row0=row0, n_global=n_global)
        elif fam == "random_fill":
            support = int(rng.choice([0, row0 + int(rng.integers(0, n + 1)), row0 + n + 3]))
            case.update(row0=row0, seed=int(rng.integers(1, 100)), support_rows=support)
            T.check_random_fill(ctx, n, m, row0=row0, seed=case["seed"], support_rows=support)
        else:
            case.update(alpha=float(rng.choice([0.0, rng.standard_normal()])))
            T.check_axpy_nrm2(ctx, rng, n, m, case["alpha"])
        print("ok", case, flush=True)
    except (AssertionError, capi.DlaError) as e:
        bad += 1
        print("FAIL", case, str(e)[:600], flush=True)
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
print(f"{cases} cases, {bad} failures", flush=True)
sys.exit(1 if bad else 0)
