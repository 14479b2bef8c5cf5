#!/usr/bin/env python3
"""The Chebyshev preconditioner on the scaled pencil (dla_spmm_precnd_cheb_pencil) at a user's size: the stiffness / mass pair of
tests/cheb_pencil_ref.py -- the five-point -div(kappa grad) with contrast 1e3 and the mass matrix on its pattern -- on a side x side
grid (side 1448: n = 2 096 704), m = 8, 8 steps, one GPU.

1. One call of the pencil form in its three ways to run a step,
     (a) fused    both matrices ELLPACK, one row loop with two gathers (ell_cheb_pencil_step_kernel),
     (b) panel    B u through the metric's own product into a panel, then A's step kernel with the pencil epilogue.  No knob selects
                  this for two ELLPACK matrices: it is what every other pair of formats takes, so the comparand is the SAME metric
                  stored as sliced ELLPACK (five entries in every row: the same 12 w n bytes, no tail) on a second context,
     (c) un-fused knob 7 = 30: both products and one combining sweep,
   and beside them a call of dla_spmm_precnd_cheb_jacobi on A alone and a call of dla_spmm_precnd_pencil, alternating call by call
   in one process after a warm-up.  A refused set-up of A (n = 0) is what binds the thread's callbacks to the other context; it
   also invalidates that context's row sums, so an un-timed bound query follows it before the timed call.  The time of a call is
   taken by device events on the context's stream, so the call's host wait is inside it.  Reported per variant: median, and the
   spread of the per-round medians (the run-to-run band).  Then, with DLA_OPT_PROFILE, every kernel of the three ways by the
   library's own event pairs, with its rate over its booked bytes.
2. For the record: gen_david_driver (max_dav 20) and lobpcg_driver (gen_eig), 8 roots, n_max 13, tol 1e-8, with the pencil Chebyshev
   and with dla_spmm_precnd_pencil: ok, iterations, launches and wall time per solve, each from the same guess, capped at max_iter.

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/cheb_pencil_ab.py [side] [rounds] [max_iter] [record]     (defaults 1448, 10, 1000, profiles/cheb_pencil.txt)
"""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

from tools.cheb_jacobi_ab import diffusion  # noqa: E402

STEPS, F, CALLS_PER_ROUND, M, FAC = 8, 0.02, 5, 8, -0.3
LEGS = [("step all", 420), ("solve davidson", 600), ("solve lobpcg", 600)]
PENCIL, SCALED, DIAG = "dla_spmm_precnd_cheb_pencil", "dla_spmm_precnd_cheb_jacobi", "dla_spmm_precnd_pencil"


def mass(order):
    """the pattern of diffusion(order): diagonal rho(i, j) = 1 + 0.5 sin(0.7 i) cos(1.1 j), every edge a tenth of the harmonic mean of
    its two rho"""
    i, j = np.meshgrid(np.arange(order), np.arange(order), indexing="ij")
    rho = 1.0 + 0.5 * np.sin(0.7 * i) * np.cos(1.1 * j)
    idx = i * order + j
    n = order * order
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [rho.ravel()]
    for di, dj in ((1, 0), (0, 1)):
        r1, r2 = rho[:order - di, :order - dj], rho[di:, dj:]
        w = (2.0 * r1 * r2 / (r1 + r2)).ravel() / 10.0
        p, q = idx[:order - di, :order - dj].ravel(), idx[di:, dj:].ravel()
        rows += [p, q]; cols += [q, p]; vals += [w, w]
    b = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    b.sort_indices()
    return b


def own_context(capi):
    """a context beside the thread's default one"""
    h = C.c_void_p()
    assert capi.load().dla_create(C.byref(h), 0) == 0
    c = capi.Context.__new__(capi.Context)
    c.lib, c.h, c._keep, c.sync_python_callbacks = capi.load(), h, [], True
    return c


def leg_step(side, rounds):
    import torch
    from diaglib_amd import capi
    a, b = diffusion(side), mass(side)
    n, m = a.shape[0], M
    ctxs = {"ell": capi.Context(), "sell": own_context(capi)}
    for fmt_b, ctx in ctxs.items():
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
        ctx.spmm_setup(a, "ell")
        ctx.spmm_setup_metric(b, fmt_b)
        ctx.spmm_cheb_config(STEPS, F)
        ia, ib = ctx.spmm_info(), ctx.spmm_metric_info()
        assert ia["format"] == "ell" and ib["format"] == fmt_b, (ia, ib)
        print(f"context with the metric as {fmt_b}: n = {n}, stored entries per row A {ia['stored'] / n:.2f}, B {ib['stored'] / n:.2f}, "
              f"long rows of B {ib['long_rows']}, hi({FAC:+.1f}) = {ctx.spmm_cheb_pencil_upper(FAC):.6f}")
    # variant -> (context, callback, knob 7)
    variants = {"(a) fused": ("ell", PENCIL, 0), "(b) panel": ("sell", PENCIL, 0), "(c) un-fused": ("ell", PENCIL, 30),
                "scaled, A alone": ("ell", SCALED, 0), "diagonal of the pencil": ("ell", DIAG, 0)}
    fns = {name: capi.fn_address(name) for name in (PENCIL, SCALED, DIAG)}
    streams = {k: torch.cuda.ExternalStream(c.lib.dla_stream(c.h)) for k, c in ctxs.items()}
    panels = {}
    for k, c in ctxs.items():
        panels[k] = (c.panel(n, m), c.panel(n, m))
        c.random_fill(panels[k][0])
    bound = {"to": None}

    def call(variant):
        which, name, knob = variants[variant]
        ctx, stream, (x, px) = ctxs[which], streams[which], panels[which]
        if bound["to"] != which:                      # (a refused set-up of A binds the thread's callbacks to this context ...)
            sync()                                         # (the two contexts have a stream each: no call overlaps the other context's)
            assert ctx.lib.dla_spmm_setup_csr(ctx.h, 0, None, None, None) == capi.ERR_ARG
            bound["to"] = which
            ctx.spmm_cheb_pencil_upper(FAC)                # (... and invalidates its row sums: formed again here, outside the timed call)
        ctx.set_option(107, knob)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx._chk(ctx.lib.dla_call_precnd(ctx.h, fns[name], n, m, FAC, x.ptr, px.ptr))
        e1.record(stream)
        ctx.set_option(107, 0)
        return e0, e1

    def sync():
        for c in ctxs.values():
            c.sync()

    # the three ways give the same bits at this size too
    outs = {}
    for v in ("(a) fused", "(b) panel", "(c) un-fused"):
        call(v)
        sync()
        outs[v] = panels[variants[v][0]][1].download()
    x0, x1 = panels["ell"][0].download(), panels["sell"][0].download()
    same_x = np.array_equal(x0, x1)
    print(f"  (a) and (c) bit-identical: {np.array_equal(outs['(a) fused'].view(np.uint64), outs['(c) un-fused'].view(np.uint64))}"
          + (f"; (a) and (b): {np.array_equal(outs['(a) fused'].view(np.uint64), outs['(b) panel'].view(np.uint64))}" if same_x else
             "; (b) runs on a panel of its own context (other random numbers), compared in tests/test_spmm_cheb_pencil_gpu.py"))
    for _ in range(3):                                     # warm-up: code objects, work panels, the bounds
        for v in variants:
            call(v)
    sync()
    ms = {v: [] for v in variants}
    for _ in range(rounds):
        pairs = [(v, call(v)) for _ in range(CALLS_PER_ROUND) for v in variants]
        sync()
        for v in ms:
            ms[v].append([e0.elapsed_time(e1) for k, (e0, e1) in pairs if k == v])
    med, spread = {}, {}
    for v in variants:
        t = np.array(ms[v])
        per_round = np.median(t, axis=1)
        med[v], spread[v] = float(np.median(t)), float(per_round.max() - per_round.min())
        print(f"  m = {m} {v:24s} {t.size} calls: median {med[v]:8.3f} ms  (min {t.min():8.3f}, max {t.max():8.3f}; per-round medians spread {spread[v]:6.3f} ms)")
    band = max(spread["(a) fused"], spread["(b) panel"])
    gain = med["(b) panel"] - med["(a) fused"]
    verdict = "(a) is faster than (b) beyond the band: the fused kernel ships" if gain > band else \
              "(a) is NOT faster than (b) beyond the band: ship (b) for two ELLPACK matrices as well"
    print(f"  (b) - (a) = {gain:+.3f} ms ({gain / med['(b) panel']:+.1%} of (b)); (c) - (a) = {med['(c) un-fused'] - med['(a) fused']:+.3f} ms; "
          f"band {band:.3f} ms: {verdict}")
    print(f"  pencil (a) against the scaled form on A alone: {med['(a) fused'] / med['scaled, A alone']:.2f} x; against the diagonal of the pencil: "
          f"{med['(a) fused'] / med['diagonal of the pencil']:.1f} x")
    # where the time sits: the library's own event pair around every launch (DLA_OPT_PROFILE), 20 calls of each way
    for v in ("(a) fused", "(b) panel", "(c) un-fused"):
        ctx = ctxs[variants[v][0]]
        call(v); sync()
        ctx.set_option(capi.OPT_PROFILE, 1)
        ctx.reset_stats()
        for _ in range(20):
            call(v)
        sync()
        ks, st = ctx.kernel_stats(), ctx.stats()
        ctx.set_option(capi.OPT_PROFILE, 0)
        for name, k in sorted(ks.items()):
            if k["launches"] > 0 and k["ms"] > 0:
                us = k["ms"] / k["launches"] * 1e3
                rate = k["alg_bytes"] / k["launches"] / us / 1e3
                print(f"  {v:12s} {name:36s} {k['launches']:4d} launches, {us:8.1f} us each, {rate:6.0f} GB/s over its booked bytes ({rate / 8000:.0%} of 8 TB/s)")
        print(f"  {v:12s} product launches (matvec class): {st['matvec']['launches']}")
    for c in ctxs.values():
        c.spmm_cheb_config(0, F)
    ctxs["sell"].destroy()


def leg_solve(side, max_iter, driver):
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    a, b = diffusion(side), mass(side)
    n = a.shape[0]
    ctx.spmm_setup(a, "ell")
    ctx.spmm_setup_metric(b, "ell")
    n_targ, n_max, tol = 8, 13, 1e-8
    guess = np.zeros((n, n_max), order="F")
    for j in range(n_max):                                # evec[i, j] = [i = 7 j] + 1e-3 cos(0.7 (i + 1)(j + 1))
        guess[:, j] = 1e-3 * np.cos(0.7 * (np.arange(n) + 1.0) * (j + 1.0))
        guess[7 * j, j] += 1.0
    mv, bv = capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_bvec")
    print(f"{driver}: n = {n}, {n_targ} roots, n_max {n_max}, tol {tol:g}, max_iter {max_iter}, both matrices ELLPACK")
    for name, steps in ((DIAG, 0), (PENCIL, STEPS)):
        ctx.spmm_cheb_config(steps, F)
        pc = capi.fn_address(name)
        for cap in (3, max_iter):                         # (three iterations to warm up, then the solve that is timed)
            ev = ctx.panel(guess)
            ctx.reset_stats(); ctx.sync()
            t0 = time.perf_counter()
            if driver == "davidson":
                eig, _, ok, info = ctx.gen_david_driver(n, n_targ, n_max, cap, tol, 20, 0.0, mv, pc, bv, ev)
            else:
                eig, _, ok, info = ctx.lobpcg_driver(n, n_targ, n_max, cap, tol, 0.0, mv, pc, ev, bvec=bv)
            ctx.sync()
            sec, st = time.perf_counter() - t0, ctx.stats()
            ev.free()
        launches = sum(st[c]["launches"] for c in capi.OP_NAMES)
        label = f"pencil Chebyshev, {steps} steps" if steps else "diagonal (dla_spmm_precnd_pencil)"
        state = "converged" if ok else f"NOT converged at {max_iter}"
        print(f"  {label:34s} {state:24s} {info['iters']:5d} iterations  {launches:7d} launches  {sec:8.3f} s   eig[0] = {eig[0]:.10e}", flush=True)
    ctx.spmm_cheb_config(0, F)
    ctx.spmm_drop_metric()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        kind, which, side, rounds, max_iter = sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        leg_step(side, rounds) if kind == "step" else leg_solve(side, max_iter, which)
        return 0
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1448
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    max_iter = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    record = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "cheb_pencil.txt")
    assert rounds * CALLS_PER_ROUND >= 50, "at least 50 calls per variant"
    text = [f"tools/cheb_pencil_ab.py {side} {rounds} {max_iter}: dla_spmm_precnd_cheb_pencil on (diffusion({side}, 1000), mass({side})), m = {M}, {STEPS} steps, fac = {FAC}"]
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
