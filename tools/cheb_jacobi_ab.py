#!/usr/bin/env python3
"""The diagonally scaled Chebyshev preconditioner (dla_spmm_precnd_cheb_jacobi) against the plain one (dla_spmm_precnd_cheb) at a
user's size: the five-point -div(kappa grad) of tests/cheb_jacobi_ref.py on a side x side grid with contrast 1e3 (side 1448:
n = 2 096 704).

1. A plain call against a scaled call, 8 steps each, alternating call by call in one process after a warm-up, in ELLPACK and in
   sliced ELLPACK, m = 8 and 13.  The time of a call is taken by device events on the context's stream, so the scaled call's host
   wait (the block maxima of its bound kernel travel to the host before the scalars exist) is inside it.  Reported per callback:
   median, and the spread of the per-round medians (the run-to-run band).  The comparand of the scaled call is the plain fused call
   of the same process.  Expected extra per call: the booked bytes of the bound kernel (24 n), of the scale sweep (16 n m + 8 n) and
   of r in every step (8 n (d - 1)) at the triad rate a = b + s c that this process measures on panels of the same size, plus one
   host wait, measured as the wall time of a bound query (dla_spmm_cheb_jacobi_upper: the bound kernel and the wait) less the bound
   kernel's bytes at the triad rate.  Then, with DLA_OPT_PROFILE, the time of every kernel of both callbacks by the library's own
   event pairs: where the difference sits.
2. Whole solves, 8 roots, n_max 13, tol 1e-8, Davidson (max_dav 20) and LOBPCG, with dla_spmm_precnd, with 8 plain steps and with 8
   and 12 scaled steps at lo_fraction 0.02: ok, iterations, launches and wall time per solve, each from the same guess, capped at
   max_iter iterations (a run that has not converged by then is reported as such).

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/cheb_jacobi_ab.py [side] [rounds] [max_iter] [record]     (defaults 1448, 10, 1000, profiles/cheb_jacobi.txt)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

STEPS, F, CALLS_PER_ROUND, CONTRAST = 8, 0.02, 5, 1e3
LEGS = [("step ell", 420), ("step sell", 420), ("solve davidson", 900), ("solve lobpcg", 900)]


def diffusion(order, contrast=CONTRAST):
    """row i * order + j, kappa(i, j) = contrast ** (0.5 + 0.5 sin(1.3 i) cos(0.9 j)), harmonic means on the edges as -w, the
    diagonal the sum of the row's weights plus kappa per missing neighbour"""
    i, j = np.meshgrid(np.arange(order), np.arange(order), indexing="ij")
    kap = float(contrast) ** (0.5 + 0.5 * np.sin(1.3 * i) * np.cos(0.9 * j))
    idx = i * order + j
    n = order * order
    diag = np.zeros(n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], []
    for di, dj in ((1, 0), (0, 1)):
        k1, k2 = kap[:order - di, :order - dj], kap[di:, dj:]
        w = (2.0 * k1 * k2 / (k1 + k2)).ravel()
        p, q = idx[:order - di, :order - dj].ravel(), idx[di:, dj:].ravel()
        rows += [p, q]; cols += [q, p]; vals += [-w, -w]
        np.add.at(diag, p, w)
        np.add.at(diag, q, w)
    diag += (((i == 0).astype(int) + (i == order - 1) + (j == 0) + (j == order - 1)) * kap).ravel()
    a = sp.coo_matrix((np.concatenate([diag] + vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    a.sort_indices()
    return a


def context(side, fmt):
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    a = diffusion(side)
    ctx.spmm_setup(a, fmt)
    return capi, ctx, a.shape[0]


def leg_step(side, rounds, fmt):
    import torch
    capi, ctx, n = context(side, fmt)
    ctx.spmm_cheb_config(STEPS, F)
    info = ctx.spmm_info()
    w = info["stored"] / n
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    fns = {"plain": capi.fn_address("dla_spmm_precnd_cheb"), "scaled": capi.fn_address("dla_spmm_precnd_cheb_jacobi")}
    print(f"format {info['format']}: n = {n}, stored entries per row {w:.2f}, Gershgorin bound {ctx.spmm_cheb_info()['upper']:.6f}, "
          f"scaled bound {ctx.spmm_cheb_jacobi_upper(0.0):.6f}")
    for m in (8, 13):
        x, px = ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)

        def call(which):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx._chk(ctx.lib.dla_call_precnd(ctx.h, fns[which], n, m, 0.0, x.ptr, px.ptr))
            b.record(stream)
            return a, b

        # the triad rate of this process on panels of this size, and the host wait of a bound query
        with torch.cuda.stream(stream):
            ta, tb, tc = (torch.rand(n * m, dtype=torch.float64, device="cuda") for _ in range(3))
            tri = []
            for _ in range(12):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                torch.add(tb, tc, alpha=1.5, out=ta)
                b.record(stream)
                stream.synchronize()
                tri.append(a.elapsed_time(b))
            del ta, tb, tc
        triad = 24.0 * n * m / (float(np.median(tri[2:])) * 1e-3)
        ctx.sync()
        waits = []
        for _ in range(12):
            t0 = time.perf_counter()
            ctx.spmm_cheb_jacobi_upper(0.0)
            waits.append((time.perf_counter() - t0) * 1e3)
        query = float(np.median(waits[2:]))
        for which in ("plain", "scaled") * 3:              # warm-up: code objects, work panels, the bounds
            call(which)
        ctx.sync()
        ms = {"plain": [], "scaled": []}
        for _ in range(rounds):
            pairs = [(which, call(which)) for _ in range(CALLS_PER_ROUND) for which in ("plain", "scaled")]
            ctx.sync()
            for which in ms:
                ms[which].append([a.elapsed_time(b) for k, (a, b) in pairs if k == which])
        med, spread = {}, {}
        for which in ("plain", "scaled"):
            t = np.array(ms[which])
            per_round = np.median(t, axis=1)
            med[which], spread[which] = float(np.median(t)), float(per_round.max() - per_round.min())
            print(f"  m = {m:2d} {which:6s} {t.size} calls of {STEPS} steps: median {med[which]:8.3f} ms  (min {t.min():8.3f}, max {t.max():8.3f}; "
                  f"per-round medians spread {spread[which]:6.3f} ms)")
        extra, band = med["scaled"] - med["plain"], max(spread.values())
        booked = 24.0 * n + 16.0 * n * m + 8.0 * n + 8.0 * n * (STEPS - 1)
        wait = max(0.0, query - 24.0 * n / triad * 1e3)
        expected = booked / triad * 1e3 + wait
        verdict = "within the band of the expectation" if extra - expected <= band else "MORE than the expectation by more than the band"
        print(f"  m = {m:2d} triad {triad / 1e9:.0f} GB/s; a bound query {query:.3f} ms wall, of which host wait {wait:.3f} ms")
        print(f"  m = {m:2d} scaled - plain = {extra:+.3f} ms ({extra / med['plain']:+.1%}); expected {booked / 1e6:.0f} MB at the triad rate "
              f"+ one host wait = {expected:.3f} ms; band {band:.3f} ms: {verdict}")
        # where the difference sits: the library's own event pair around every launch (DLA_OPT_PROFILE), 20 calls of each callback
        ctx.set_option(capi.OPT_PROFILE, 1)
        ctx.reset_stats()
        for _ in range(20):
            for which in ("plain", "scaled"):
                ctx._chk(ctx.lib.dla_call_precnd(ctx.h, fns[which], n, m, 0.0, x.ptr, px.ptr))
        ctx.sync()
        ks = ctx.kernel_stats()
        ctx.set_option(capi.OPT_PROFILE, 0)
        for name, k in sorted(ks.items()):
            if k["launches"] > 0 and "cheb" in name:
                us = k["ms"] / k["launches"] * 1e3
                print(f"  m = {m:2d} {name:30s} {k['launches']:4d} launches, {us:8.1f} us each, {k['alg_bytes'] / k['launches'] / us / 1e3:6.0f} GB/s over its booked bytes")
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
    for name, steps in (("dla_spmm_precnd", 0), ("dla_spmm_precnd_cheb", 8), ("dla_spmm_precnd_cheb_jacobi", 8), ("dla_spmm_precnd_cheb_jacobi", 12)):
        ctx.spmm_cheb_config(steps, F)
        pc = capi.fn_address(name)
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
        label = f"{'scaled' if name.endswith('jacobi') else 'plain'} Chebyshev, {steps:2d} steps" if steps else "diagonal (dla_spmm_precnd)"
        state = "converged" if ok else f"NOT converged at {max_iter}"
        print(f"  {label:30s} {state:24s} {info['iters']:5d} iterations  {launches:7d} launches  {sec:8.3f} s   eig[0] = {eig[0]:.10e}", flush=True)
    ctx.spmm_cheb_config(0, F)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        kind, which, side, rounds, max_iter = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        leg_step(side, rounds, which) if kind == "step" else leg_solve(side, max_iter, which)
        return 0
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1448
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    max_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    record = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "cheb_jacobi.txt")
    assert rounds * CALLS_PER_ROUND >= 50, "at least 50 calls per callback"
    text = [f"tools/cheb_jacobi_ab.py {side} {rounds} {max_iter}: dla_spmm_precnd_cheb_jacobi against dla_spmm_precnd_cheb on diffusion({side}, {CONTRAST:g})"]
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
