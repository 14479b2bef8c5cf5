#!/usr/bin/env python3
"""The dense device operator (dla_dense_matvec: dense_mfma_kernel, and dense_combine_kernel where the contraction is split) at
users' sizes, beside torch.matmul and the triad rate of the same process.

1. The product Y = A X at n = 2048, 8192 and 32768 (a leg each), m = 1, 8, 13 and 37.  A is a random matrix made on the device and
   handed over with dla_dense_setup_dev; torch.matmul multiplies the SAME device arrays (the caller's column-major A, the
   library's X panel).  The two alternate call by call on the context's stream after a warm-up; a call is timed by device events
   around it.  Reported per shape: the medians, the spread of the per-round medians, the product's rate over its booked bytes
   8 n^2 + 16 n m beside the rate dla_stream_triad measures in this process, k_chunks, and the ratio to torch.matmul.  No threshold:
   shapes where the kernel loses are printed like the others.
2. The reference harness' solve (main.f90:311-317, davidson_driver, 8 roots, n_max 13, tol 1e-9, max_dav 20) at n = 2000 in host mode
   (the oracle's orc_dense_matvec / orc_dense_precnd through host callbacks) and in device mode (dla_dense_matvec / dla_dense_precnd):
   wall time per solve, iterations, eigenvalue difference.

3. With --lr, the dense linear-response parts instead (record: profiles/dense_lr_operator.txt): one caslr_eff_driver solve and one
   caslr_driver solve of the reference harness' linear-response problem (orc_lr_setup; 4 roots, n_max 8, tol 1e-9, max_dav 20, unit
   guess) at n = 2000 in device mode (dla_dense_apbmul .. smdmul, dla_dense_lrprec2 / 1) and the same solves through host callbacks
   (the oracle's orc_lr_* routines); and the pair set-up dla_dense_setup_lr_pair_dev at n = 8192 -- wall time of the synchronous
   call, in ms and in GB/s of its 16 n^2 + 16 n_pad^2 bytes (two sources read, two copies written), beside the triad rate of the
   process.  Recorded figures, no thresholds.

4. With --transpose, the transposed product instead (record: profiles/dense_operator_t.txt): dla_dense_matvec_t beside
   dla_dense_matvec on the SAME stored matrix at n = 2048, 8192 and 32768, m = 8, 13 and 37, alternating call by call as in 1. --
   medians, spreads, TB/s of the booked bytes and the ratio transposed / forward -- and one nonsym_driver solve (side c, 4 roots,
   n_max 8, tol 1e-9, max_dav 10) of the matrix of examples/fortran_nonsym_caller at n = 2000 in device mode (dla_dense_matvec,
   dla_dense_matvec_t, dla_dense_precnd) beside host callbacks (numpy products with a and its transposed copy).

5. With --sym, the symmetric storage instead (record: profiles/dense_sym_operator.txt): the product on the triangular copy
   (dla_dense_setup_sym, here in the metric slot: dense_sym_mfma_kernel and dense_sym_combine_kernel) beside dla_dense_matvec on the
   full copy of the SAME symmetric matrix in the same process at n = 2048, 8192 and 32768, m = 8, 13 and 37, alternating call by
   call as in 1. -- medians, spreads, the device bytes of both copies, the full product's rate over its booked bytes beside the
   triad rate, the plan of the symmetric pass and the ratio symmetric / full -- and the harness solve of 2. at n = 2000 in device
   mode with the operator stored in full and as a triangle.

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/dense_operator_bench.py [rounds] [record]          (defaults 10, profiles/dense_operator.txt)
    python tools/dense_operator_bench.py --lr [rounds] [record]     (defaults 10, profiles/dense_lr_operator.txt)
    python tools/dense_operator_bench.py --transpose [rounds] [record]   (defaults 10, profiles/dense_operator_t.txt)
    python tools/dense_operator_bench.py --sym [rounds] [record]         (defaults 10, profiles/dense_sym_operator.txt)
"""
import os
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CALLS_PER_ROUND, WIDTHS = 5, (1, 8, 13, 37)
LEGS = [("product 2048", 300), ("product 8192", 300), ("product 32768", 420), ("solve 2000", 420)]
LR_LEGS = [("lrsolve 2000", 420), ("lrpair 8192", 300)]
T_LEGS = [("tproduct 2048", 300), ("tproduct 8192", 300), ("tproduct 32768", 420), ("nsolve 2000", 420)]
T_WIDTHS = (8, 13, 37)
S_LEGS = [("sproduct 2048", 300), ("sproduct 8192", 300), ("sproduct 32768", 420), ("ssolve 2000", 420)]


def leg_product(n, rounds):
    import torch
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen).T      # column-major: a(i, k) at i + k n
    ctx.dense_setup(a)
    triad = ctx.stream_triad(max(1 << 24, n * n // 4))
    fn = capi.fn_address("dla_dense_matvec")
    print(f"n = {n}: stored copy {ctx.dense_info()['device_bytes'] / 1e6:.0f} MB, triad {triad:.0f} GB/s")
    for m in WIDTHS:
        x, y = ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)
        xt = ctx._dev_tensor(x.ptr, n, m)
        yt = torch.empty((n, m), dtype=torch.float64, device="cuda")                 # (torch's own preferred layout for its result)

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if which == "dense":
                ctx._chk(ctx.lib.dla_call_matvec(ctx.h, fn, n, m, x.ptr, y.ptr))
            else:
                with torch.cuda.stream(stream):
                    torch.matmul(a, xt, out=yt)
            e1.record(stream)
            return e0, e1

        for which in ("dense", "torch") * 3:
            call(which)
        ctx.sync()
        diff = float((ctx._dev_tensor(y.ptr, n, m) - yt).abs().max())
        ms = {"dense": [], "torch": []}
        for _ in range(rounds):
            pairs = [(which, call(which)) for _ in range(CALLS_PER_ROUND) for which in ("dense", "torch")]
            ctx.sync()
            for which in ms:
                ms[which].append([e0.elapsed_time(e1) for k, (e0, e1) in pairs if k == which])
        med, spread = {}, {}
        for which in ms:
            t = np.array(ms[which])
            per_round = np.median(t, axis=1)
            med[which], spread[which] = float(np.median(t)), float(per_round.max() - per_round.min())
        rate = (8.0 * n * n + 16.0 * n * m) / (med["dense"] * 1e-3) / 1e9
        print(f"  m = {m:2d}  k_chunks {ctx.dense_info()['k_chunks']:2d}  dense {med['dense']:8.4f} ms (spread {spread['dense']:.4f})  {rate:6.0f} GB/s = "
              f"{rate / triad:5.2f} of the triad rate   torch.matmul {med['torch']:8.4f} ms (spread {spread['torch']:.4f})   dense / torch = "
              f"{med['dense'] / med['torch']:5.2f}   max |difference| {diff:.2e}", flush=True)
        x.free(); y.free()
    print(f"  triad after the products {ctx.stream_triad(max(1 << 24, n * n // 4)):.0f} GB/s")
    ctx.dense_drop()


def leg_tproduct(n, rounds):
    import torch
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen).T      # column-major: a(i, k) at i + k n
    ctx.dense_setup(a)
    triad = ctx.stream_triad(max(1 << 24, n * n // 4))
    fns = {"forward": capi.fn_address("dla_dense_matvec"), "transposed": capi.fn_address("dla_dense_matvec_t")}
    print(f"n = {n}: stored copy {ctx.dense_info()['device_bytes'] / 1e6:.0f} MB, triad {triad:.0f} GB/s")
    for m in T_WIDTHS:
        x, y = ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)
        xt = ctx._dev_tensor(x.ptr, n, m)

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx._chk(ctx.lib.dla_call_matvec(ctx.h, fns[which], n, m, x.ptr, y.ptr))
            e1.record(stream)
            return e0, e1

        for which in ("forward", "transposed") * 3:
            call(which)
        ctx.sync()
        with torch.cuda.stream(stream):
            want = torch.matmul(a.T, xt)
        stream.synchronize()
        diff = float((ctx._dev_tensor(y.ptr, n, m) - want).abs().max())      # (y holds the last call's result: the transposed one)
        ms = {"forward": [], "transposed": []}
        for _ in range(rounds):
            pairs = [(which, call(which)) for _ in range(CALLS_PER_ROUND) for which in ("forward", "transposed")]
            ctx.sync()
            for which in ms:
                ms[which].append([e0.elapsed_time(e1) for k, (e0, e1) in pairs if k == which])
        med, spread = {}, {}
        for which in ms:
            t = np.array(ms[which])
            per_round = np.median(t, axis=1)
            med[which], spread[which] = float(np.median(t)), float(per_round.max() - per_round.min())
        rate = {w: (8.0 * n * n + 16.0 * n * m) / (med[w] * 1e-3) / 1e12 for w in med}
        print(f"  m = {m:2d}  forward {med['forward']:8.4f} ms (spread {spread['forward']:.4f}) {rate['forward']:5.2f} TB/s   transposed "
              f"{med['transposed']:8.4f} ms (spread {spread['transposed']:.4f}) {rate['transposed']:5.2f} TB/s   transposed / forward = "
              f"{med['transposed'] / med['forward']:5.2f}   max |A^T x - torch| {diff:.2e}", flush=True)
        x.free(); y.free()
    print(f"  triad after the products {ctx.stream_triad(max(1 << 24, n * n // 4)):.0f} GB/s")
    ctx.dense_drop()


def leg_sproduct(n, rounds):
    import torch
    from diaglib_amd import capi
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen)
    a = torch.tril(a) + torch.tril(a, -1).T                                          # exactly symmetric (and so column-major as it is)
    ctx.dense_setup(a.T)                                                             # slot 0: the full copy
    ctx.dense_setup(a.T, metric=True, sym="L")                                       # slot 1: one triangle of the same matrix
    full, tri = ctx.dense_info()["device_bytes"], ctx.dense_info(True)["device_bytes"]
    triad = ctx.stream_triad(max(1 << 24, n * n // 4))
    fns = {"full": capi.fn_address("dla_dense_matvec"), "symmetric": capi.fn_address("dla_dense_bvec")}
    print(f"n = {n}: full copy {full / 1e6:.0f} MB, triangular copy {tri / 1e6:.0f} MB ({(full - tri) / 1e6:.0f} MB saved, {tri / full:.3f} of the full copy), "
          f"triad {triad:.0f} GB/s")
    for m in T_WIDTHS:
        x, y, ys = ctx.panel(n, m), ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)
        out = {"full": y, "symmetric": ys}

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx._chk(ctx.lib.dla_call_matvec(ctx.h, fns[which], n, m, x.ptr, out[which].ptr))
            e1.record(stream)
            return e0, e1

        for which in ("full", "symmetric") * 3:
            call(which)
        ctx.sync()
        diff = float((ctx._dev_tensor(y.ptr, n, m) - ctx._dev_tensor(ys.ptr, n, m)).abs().max())
        ms = {"full": [], "symmetric": []}
        for _ in range(rounds):
            pairs = [(which, call(which)) for _ in range(CALLS_PER_ROUND) for which in ("full", "symmetric")]
            ctx.sync()
            for which in ms:
                ms[which].append([e0.elapsed_time(e1) for k, (e0, e1) in pairs if k == which])
        med, spread = {}, {}
        for which in ms:
            t = np.array(ms[which])
            per_round = np.median(t, axis=1)
            med[which], spread[which] = float(np.median(t)), float(per_round.max() - per_round.min())
        rate = (8.0 * n * n + 16.0 * n * m) / (med["full"] * 1e-3) / 1e9
        plan, ws = ctx.dense_sym_info(True), ctx.dense_info(True)["workspace_bytes"]
        print(f"  m = {m:2d}  full {med['full']:8.4f} ms (spread {spread['full']:.4f}) {rate:6.0f} GB/s = {rate / triad:5.2f} of the triad rate   symmetric "
              f"{med['symmetric']:8.4f} ms (spread {spread['symmetric']:.4f}; {plan['panels']} panels, chunks of {plan['chunk_blocks']} blocks, at most "
              f"{plan['max_partials']} partials per element, workspace {ws / 1e6:.1f} MB)   symmetric / full = {med['symmetric'] / med['full']:5.2f}   "
              f"max |difference| {diff:.2e}", flush=True)
        x.free(); y.free(); ys.free()
    print(f"  triad after the products {ctx.stream_triad(max(1 << 24, n * n // 4)):.0f} GB/s")
    ctx.dense_drop()
    ctx.dense_drop(True)


def leg_ssolve(n):
    from diaglib_amd import capi
    ctx = capi.Context()
    t, m, tol, max_dav = 8, 13, 1e-9, 20
    idx = np.arange(1, n + 1.0)
    a = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a, idx + 1.0)
    g = np.zeros((n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    mv, pc = capi.fn_address("dla_dense_matvec"), capi.fn_address("dla_dense_precnd")
    times, out = {"stored in full": [], "stored as a triangle": []}, {}
    for _ in range(5):                                       # (the two storages alternate solve by solve; the first pair is the warm-up)
        for mode, sym in (("stored in full", None), ("stored as a triangle", "L")):
            ctx.dense_setup(a, sym=sym)
            ctx.sync()
            t0 = time.perf_counter()
            eig, _, ok, info = ctx.davidson_driver(n, t, m, 300, tol, max_dav, 0.0, mv, pc, g)
            times[mode].append((time.perf_counter() - t0) * 1e3)
            out[mode] = (eig[:t].copy(), ok, info["iters"], ctx.dense_info()["device_bytes"])
    for mode, ts in times.items():
        eig, ok, iters, nbytes = out[mode]
        print(f"n = {n} davidson_driver, device callbacks, operator {mode} ({nbytes / 1e6:.1f} MB): median {np.median(ts[1:]):8.2f} ms per solve "
              f"(min {min(ts[1:]):.2f}), {iters} iterations, ok = {ok}", flush=True)
    e0, e1 = (v[0] for v in out.values())
    print(f"  largest relative eigenvalue difference between the two storages: {float(np.abs(e0 / e1 - 1.0).max()):.2e}")
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.dense_drop()


def leg_nsolve(n):
    from diaglib_amd import capi
    ctx = capi.Context()
    t, m, tol, max_dav = 4, 8, 1e-9, 10
    # the matrix of examples/fortran_nonsym_caller: exp(-T) A0 exp(T), T = alpha u v^T of Frobenius norm 0.01
    idx = np.arange(1, n + 1.0)
    a0 = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a0, idx + 1.0)
    u, v = np.sin(1.3 * idx), np.cos(0.7 * idx)
    alpha = 0.01 / (np.linalg.norm(u) * np.linalg.norm(v))
    s = alpha * (v @ u)
    a = (np.eye(n) - alpha * np.expm1(-s) / -s * np.outer(u, v)) @ a0 @ (np.eye(n) + alpha * np.expm1(s) / s * np.outer(u, v))
    a, at, diag = np.asfortranarray(a), np.asfortranarray(a.T), np.diag(a).copy()

    def mprec(fac, x):
        d = diag + fac
        safe = np.abs(d) > 1.0e-5
        return np.where(safe[:, None], x / np.where(safe, d, 1.0)[:, None], x)

    g = np.zeros((n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    ctx.dense_setup(a)
    out = {}
    for mode, device, fns in (("host callbacks (numpy, a and its transposed copy)", 0, (lambda x: a @ x, lambda x: at @ x, mprec)),
                              ("device callbacks (dla_dense_matvec, dla_dense_matvec_t)", 1,
                               tuple(capi.fn_address(f) for f in ("dla_dense_matvec", "dla_dense_matvec_t", "dla_dense_precnd")))):
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, device)
        times = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            eig, _, _, ok, info = ctx.nonsym_driver(n, t, m, 200, tol, max_dav, 0.0, *fns, g, g, "c")
            times.append((time.perf_counter() - t0) * 1e3)
        out[mode] = eig[:t].copy()
        print(f"n = {n} nonsym_driver side c, {mode}: median {np.median(times[1:]):8.2f} ms per solve (min {min(times[1:]):.2f}), {info['iters']} iterations, "
              f"{info['matvec_cols']} matvec columns, ok = {ok}", flush=True)
    e0, e1 = out.values()
    print(f"  largest relative eigenvalue difference between the two modes: {float(np.abs(e0 / e1 - 1.0).max()):.2e}")
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.dense_drop()


def leg_solve(n):
    from diaglib_amd import capi
    from oracle.pyoracle import Oracle      # (tools/ is measurement infrastructure, like tools/host_mode_probe.py)
    ctx, o = capi.Context(), Oracle()
    t, m, tol, max_dav = 8, 13, 1e-9, 20
    idx = np.arange(1, n + 1.0)
    a = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a, idx + 1.0)
    g = np.zeros((n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    o.dense_setup(n)
    ctx.dense_setup(a)
    out = {}
    for mode, device, mv, pc in (("host callbacks (orc_dense_matvec)", 0, o.fn("orc_dense_matvec"), o.fn("orc_dense_precnd")),
                                 ("device callbacks (dla_dense_matvec)", 1, capi.fn_address("dla_dense_matvec"), capi.fn_address("dla_dense_precnd"))):
        ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, device)
        times = []
        for _ in range(5):
            ctx.sync()
            t0 = time.perf_counter()
            eig, _, ok, info = ctx.davidson_driver(n, t, m, 300, tol, max_dav, 0.0, mv, pc, g)
            times.append((time.perf_counter() - t0) * 1e3)
        out[mode] = eig[:t].copy()
        print(f"n = {n} davidson_driver, {mode}: median {np.median(times[1:]):8.2f} ms per solve (min {min(times[1:]):.2f}), {info['iters']} iterations, ok = {ok}", flush=True)
    e0, e1 = out.values()
    print(f"  largest relative eigenvalue difference between the two modes: {float(np.abs(e0 / e1 - 1.0).max()):.2e}")
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.dense_drop()


def leg_lr_solve(n):
    from diaglib_amd import capi
    from oracle.pyoracle import Oracle
    ctx, o = capi.Context(), Oracle()
    t, m, tol, max_dav = 4, 8, 1e-9, 20
    parts = ("apb", "amb", "spd", "smd")
    for part, a in zip(parts, o.lr_setup(n)):
        ctx.dense_setup_lr(part, a)
    g = np.zeros((2 * n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    for driver, trad in (("caslr_eff_driver", False), ("caslr_driver", True)):
        out = {}
        host = [o.fn(k) for k in ("orc_lr_apb", "orc_lr_amb", "orc_lr_spd", "orc_lr_smd", "orc_lr_prec1" if trad else "orc_lr_prec")]
        device = [capi.fn_address(f"dla_dense_{p}mul") for p in parts] + [capi.fn_address("dla_dense_lrprec1" if trad else "dla_dense_lrprec2")]
        for mode, on_device, fns in (("host callbacks (orc_lr_*)", 0, host), ("device callbacks (dla_dense_*)", 1, device)):
            ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, on_device)
            solve = ctx.caslr_driver if trad else ctx.caslr_eff_driver
            times = []
            for _ in range(5):
                ctx.sync()
                t0 = time.perf_counter()
                eig, _, ok, info = solve(n, t, m, 200, tol, max_dav, *fns, g)
                times.append((time.perf_counter() - t0) * 1e3)
            out[mode] = eig[:t].copy()
            print(f"n = {n} {driver}, {mode}: median {np.median(times[1:]):8.2f} ms per solve (min {min(times[1:]):.2f}), {info['iters']} iterations, ok = {ok}", flush=True)
        e0, e1 = out.values()
        print(f"  largest relative eigenvalue difference between the two modes: {float(np.abs(e0 / e1 - 1.0).max()):.2e}")
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.dense_drop_lr()


def leg_lr_pair(n, rounds):
    import torch
    from diaglib_amd import capi
    ctx = capi.Context()
    gen = torch.Generator(device="cuda").manual_seed(n)
    p, q = (torch.rand((n, n), dtype=torch.float64, device="cuda", generator=gen).T for _ in range(2))      # column-major
    torch.cuda.synchronize()
    triad = ctx.stream_triad(max(1 << 24, n * n // 4))
    ctx._chk(ctx.lib.dla_dense_setup_lr_pair_dev(ctx.h, 0, n, p.data_ptr(), n, q.data_ptr(), n))      # (the blocks are allocated here)
    n_pad = ctx.dense_lr_info("apb")["n_pad"]
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        ctx._chk(ctx.lib.dla_dense_setup_lr_pair_dev(ctx.h, 0, n, p.data_ptr(), n, q.data_ptr(), n))
        times.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(times))
    moved = 16.0 * n * n + 16.0 * n_pad * n_pad
    print(f"n = {n} dla_dense_setup_lr_pair_dev (synchronous call, blocks in place): median {med:8.3f} ms (min {min(times):.3f}, max {max(times):.3f}) over "
          f"{rounds} calls, {moved / 1e9:.2f} GB moved = {moved / (med * 1e-3) / 1e9:6.0f} GB/s = {moved / (med * 1e-3) / 1e9 / triad:5.2f} of the triad rate "
          f"({triad:.0f} GB/s)", flush=True)
    ctx.dense_drop_lr()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        kind, n, rounds = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        {"product": lambda: leg_product(n, rounds), "solve": lambda: leg_solve(n), "lrsolve": lambda: leg_lr_solve(n),
         "lrpair": lambda: leg_lr_pair(n, rounds), "tproduct": lambda: leg_tproduct(n, rounds), "nsolve": lambda: leg_nsolve(n),
         "sproduct": lambda: leg_sproduct(n, rounds), "ssolve": lambda: leg_ssolve(n)}[kind]()
        return 0
    args = [a for a in sys.argv[1:] if a not in ("--lr", "--transpose", "--sym")]
    lr, tr, sy = "--lr" in sys.argv[1:], "--transpose" in sys.argv[1:], "--sym" in sys.argv[1:]
    rounds = int(args[0]) if args else 10
    record = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "dense_sym_operator.txt" if sy else "dense_operator_t.txt" if tr else "dense_lr_operator.txt" if lr else "dense_operator.txt")
    if sy:
        text = [f"tools/dense_operator_bench.py --sym {rounds}: the product on the triangular copy (dla_dense_setup_sym) beside dla_dense_matvec on the full "
                f"copy of the same symmetric matrix, {rounds * CALLS_PER_ROUND} timed calls each per shape; davidson_driver in device mode on both storages "
                f"(4 timed solves each)"]
    elif tr:
        text = [f"tools/dense_operator_bench.py --transpose {rounds}: dla_dense_matvec_t beside dla_dense_matvec on the same stored matrix, "
                f"{rounds * CALLS_PER_ROUND} timed calls each per shape; nonsym_driver in device mode beside host callbacks (4 timed solves each)"]
    elif lr:
        text = [f"tools/dense_operator_bench.py --lr {rounds}: the linear-response drivers on dense parts in device mode beside host callbacks (4 timed solves "
                f"each), and the pair set-up ({rounds} timed calls) beside the triad rate"]
    else:
        text = [f"tools/dense_operator_bench.py {rounds}: dla_dense_matvec beside torch.matmul and the triad rate; {rounds * CALLS_PER_ROUND} timed calls each per shape"]
    for leg, limit in (S_LEGS if sy else T_LEGS if tr else LR_LEGS if lr else LEGS):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg"] + leg.split() + [str(rounds)]
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
