#!/usr/bin/env python3
"""The Chebyshev polynomial preconditioner (dla_spmm_precnd_cheb) at a user's size: the five-point Laplacian on a side x side grid
plus 0.05 cos(0.37 i) on the diagonal (side 1448: n = 2 096 704).

1. The fused step (ell_cheb_step_kernel / sell_cheb_step_kernel: the product kernel with the combination as its epilogue) against the
   un-fused one (knob 7 = 30: the product kernel into a work panel plus one combining sweep), in ELLPACK and in sliced ELLPACK, m = 8
   and 13.  The two paths alternate call by call in one process after a warm-up; the time of a call of 8 steps (7 kernels or 7 pairs)
   is taken by device events on the context's stream.  Reported per path: median, and the spread of the per-round medians (the
   run-to-run spread the verdict is held against).  Also the achieved rate of a fused step against its booked algorithmic bytes
   (12 w n + 32 n m: the matrix, three panel reads with the gather counted once, one write): a gather-bound kernel's rate, not a
   share of a streaming peak.
2. Whole solves, 8 roots, n_max 13, tol 1e-8, Davidson (max_dav 20) and LOBPCG, with dla_spmm_precnd and with 4, 8 and 12 steps at
   lo_fraction 0.02: ok, iterations, launches and wall time per solve, each from the same guess, capped at max_iter iterations (a
   run that has not converged by then is reported as such).

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/cheb_precnd_ab.py [side] [rounds] [max_iter] [record]     (defaults 1448, 10, 1000, profiles/cheb_precnd.txt)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

STEPS, F, CALLS_PER_ROUND = 8, 0.02, 5
LEGS = [("step ell", 420), ("step sell", 420), ("solve davidson", 900), ("solve lobpcg", 900)]


def laplacian(side):
    t = sp.diags([-np.ones(side - 1), 2.0 * np.ones(side), -np.ones(side - 1)], [-1, 0, 1])
    eye = sp.identity(side)
    n = side * side
    return (sp.kron(eye, t) + sp.kron(t, eye) + sp.diags(0.05 * np.cos(0.37 * np.arange(n)))).tocsr()


def context(side, fmt):
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    a = laplacian(side)
    ctx.spmm_setup(a, fmt)
    return capi, ctx, a.shape[0]


def leg_step(side, rounds, fmt):
    import torch
    capi, ctx, n = context(side, fmt)
    ctx.spmm_cheb_config(STEPS, F)
    info = ctx.spmm_info()
    w = info["stored"] / n
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    fn = capi.fn_address("dla_spmm_precnd_cheb")
    print(f"format {info['format']}: n = {n}, stored entries per row {w:.2f}, upper bound {ctx.spmm_cheb_info()['upper']:.6f}")
    for m in (8, 13):
        x, px = ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)

        def call(knob):
            ctx.set_option(107, knob)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx._chk(ctx.lib.dla_call_precnd(ctx.h, fn, n, m, 0.0, x.ptr, px.ptr))
            b.record(stream)
            return a, b

        for knob in (0, 30, 0, 30, 0, 30):               # warm-up: code objects, work panels, the bound
            call(knob)
        ctx.sync()
        ms = {0: [], 30: []}
        for _ in range(rounds):
            pairs = [(knob, call(knob)) for _ in range(CALLS_PER_ROUND) for knob in (0, 30)]
            ctx.sync()
            for knob in (0, 30):
                ms[knob].append([a.elapsed_time(b) for k, (a, b) in pairs if k == knob])
        ctx.set_option(107, 0)
        med, spread = {}, {}
        for knob, label in ((0, "fused"), (30, "un-fused")):
            t = np.array(ms[knob])
            per_round = np.median(t, axis=1)
            med[knob], spread[knob] = float(np.median(t)), float(per_round.max() - per_round.min())
            print(f"  m = {m:2d} {label:8s} {t.size} calls of {STEPS} steps: median {med[knob]:8.3f} ms  (min {t.min():8.3f}, max {t.max():8.3f}; "
                  f"per-round medians spread {spread[knob]:6.3f} ms)")
        gain, band = med[30] - med[0], max(spread.values())
        verdict = "fused is faster by more than the spread" if gain > band else "NOT faster by more than the spread"
        booked = 12.0 * w * n + 32.0 * n * m
        print(f"  m = {m:2d} un-fused - fused = {gain:+.3f} ms ({gain / med[30]:+.1%}), spread {band:.3f} ms: {verdict}")
        print(f"  m = {m:2d} a fused step: {booked / 1e6:.0f} MB booked in {med[0] / (STEPS - 1) * 1e3:.0f} us = "
              f"{booked * (STEPS - 1) / med[0] / 1e6:.0f} GB/s (a gather-bound kernel's rate over its algorithmic bytes)")
        x.free(); px.free()
    ctx.spmm_cheb_config(0, F)


def leg_solve(side, max_iter, driver):
    capi, ctx, n = context(side, "ell")
    n_targ, n_max, tol = 8, 13, 1e-8
    guess = np.zeros((n, n_max), order="F")
    for j in range(n_max):                                # evec[i, j] = [i = 7 j] + 1e-3 cos(0.7 (i + 1)(j + 1))
        guess[:, j] = 1e-3 * np.cos(0.7 * (np.arange(n) + 1.0) * (j + 1.0))
        guess[7 * j, j] += 1.0
    mv = capi.fn_address("dla_spmm_matvec")
    print(f"{driver}: n = {n}, {n_targ} roots, n_max {n_max}, tol {tol:g}, max_iter {max_iter}, ELLPACK")
    for steps in (0, 4, 8, 12):
        ctx.spmm_cheb_config(steps, F)
        pc = capi.fn_address("dla_spmm_precnd_cheb" if steps else "dla_spmm_precnd")
        for cap in (3, max_iter):                         # (three iterations to warm up, then the solve that is timed)
            ev = ctx.panel(guess)
            ctx.reset_stats(); ctx.sync()
            t0 = time.perf_counter()
            if driver == "davidson":
                eig, _, ok, info = ctx.davidson_driver(n, n_targ, n_max, cap, tol, 20, 0.0, mv, pc, ev)
            else:
                eig, _, ok, info = ctx.lobpcg_driver(n, n_targ, n_max, cap, tol, 0.0, mv, pc, ev)
            ctx.sync()
            sec, st = time.perf_counter() - t0, ctx.stats()
            ev.free()
        launches = sum(st[c]["launches"] for c in capi.OP_NAMES)
        label = f"Chebyshev, {steps:2d} steps" if steps else "diagonal (dla_spmm_precnd)"
        state = "converged" if ok else f"NOT converged at {max_iter}"
        print(f"  {label:28s} {state:24s} {info['iters']:5d} iterations  {launches:7d} launches  {sec:8.3f} s   eig[0] = {eig[0]:.10e}", flush=True)
    ctx.spmm_cheb_config(0, F)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        kind, which, side, rounds, max_iter = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        leg_step(side, rounds, which) if kind == "step" else leg_solve(side, max_iter, which)
        return 0
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1448
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    max_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    record = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "cheb_precnd.txt")
    assert rounds * CALLS_PER_ROUND >= 50, "at least 50 calls per path"
    text = [f"tools/cheb_precnd_ab.py {side} {rounds} {max_iter}: dla_spmm_precnd_cheb on the five-point Laplacian, {side} x {side}"]
    for leg, limit in LEGS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg"] + leg.split() + [str(side), str(rounds), str(max_iter)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                             # (as it comes: a long leg is not silent)
            print(line, end="", flush=True)
            text.append(line.rstrip())
        if p.wait() != 0:
            print(f"leg '{leg}' ended with status {p.returncode}: stopping here", flush=True)
            return p.returncode
    with open(record, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
