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

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/dense_operator_bench.py [rounds] [record]     (defaults 10, profiles/dense_operator.txt)
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


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        kind, n, rounds = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        leg_product(n, rounds) if kind == "product" else leg_solve(n)
        return 0
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    record = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dense_operator.txt")
    text = [f"tools/dense_operator_bench.py {rounds}: dla_dense_matvec beside torch.matmul and the triad rate; {rounds * CALLS_PER_ROUND} timed calls each per shape"]
    for leg, limit in LEGS:
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
