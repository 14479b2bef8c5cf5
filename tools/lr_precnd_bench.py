#!/usr/bin/env python3
"""lr_precnd_kernel (dla_spmm_lrprec1 / 2: lrprec_1 / lrprec_2 on the stored diagonals of the sparse linear-response parts) beside
synth_lrprec_kernel (dla_synth_lrprec1 / 2: the same job on the diagonals of the built-in sample operators), interleaved in one
process, with the triad rate of the same process as the yardstick.  HIP-event time from the engine's own statistics
(OPT_PROFILE); bytes are the algorithmic ones: 32 n m for the four blocks + 24 n (three stored diagonals) or 8 n (wsq).

    python tools/lr_precnd_bench.py [n] [m] [rounds] [reps]        (defaults 2 000 000, 13, 7, 20; the text of profiles/spmm_lr.txt)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
from diaglib_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 13
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20

ctx = capi.Context()
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
ctx.set_option(capi.OPT_PROFILE, 1)
ctx.synth_setup(n, 0, n)
i = np.arange(1.0, n + 1.0)
for part, diag in (("apb", i + 5.0), ("amb", i + 2.0), ("spd", 1.0 + 0.5 / (1.0 + (np.arange(1, n + 1) % 7)))):
    ctx.spmm_setup_lr(part, sp.diags(diag).tocsr())
xp, xm, yp, ym = (ctx.panel(n, m) for _ in range(4))
ctx.random_fill(xp); ctx.random_fill(xm)


def call(name, fac):
    ctx._chk(ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(name), n, m, fac, xp.ptr, xm.ptr, yp.ptr, ym.ptr))


CASES = [("lr_precnd_kernel<2>  lrprec1", "dla_spmm_lrprec1", 0.37, 32.0 * n * m + 24.0 * n),
         ("synth_lrprec_kernel  lrprec1", "dla_synth_lrprec1", 0.37, 32.0 * n * m + 8.0 * n),
         ("lr_precnd_kernel<2>  lrprec2", "dla_spmm_lrprec2", 2.5, 32.0 * n * m + 24.0 * n),
         ("synth_lrprec_kernel  lrprec2", "dla_synth_lrprec2", 2.5, 32.0 * n * m + 8.0 * n)]
for _, name, fac, _ in CASES:                 # warm-up: code objects, first launches
    for _ in range(3):
        call(name, fac)
ctx.sync()
times = {c[0]: [] for c in CASES}
triad = []
for _ in range(rounds):
    triad.append(ctx.stream_triad(n * m, 5))
    for label, name, fac, _ in CASES:
        ctx.reset_stats()
        for _ in range(reps):
            call(name, fac)
        ctx.sync()
        st = ctx.stats()["precnd"]
        assert st["launches"] >= reps, st
        times[label].append(st["ms"] / reps)
tri = float(np.median(triad))
print(f"backend {ctx.backend}; n = {n}, m = {m}; {rounds} rounds x {reps} calls per kernel, alternating; HIP-event time per call")
print(f"triad rate of this process (n m doubles per stream): median {tri:.0f} GB/s (min {min(triad):.0f}, max {max(triad):.0f})")
for label, _, _, nbytes in CASES:
    t = np.array(times[label])
    med = float(np.median(t))
    print(f"{label:30s} median {med * 1e3:8.1f} us  (min {t.min() * 1e3:8.1f}, max {t.max() * 1e3:8.1f})  "
          f"{nbytes / med / 1e6:7.0f} GB/s = {nbytes / med / 1e6 / tri:5.2f} of the triad rate")
