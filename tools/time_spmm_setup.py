#!/usr/bin/env python3
"""Wall time of the three ways a sparse matrix reaches the device operator, in one process, interleaved round by round:

  host     dla_spmm_setup_csr_fmt on host arrays (one host thread checks, sorts and scatters; 12 bytes per stored entry uploaded)
  device   dla_spmm_setup_csr_dev on the same arrays in device memory (row pointers to the host, entries by kernels)
  refresh  dla_spmm_refresh_values_dev: new values for the stored pattern

on (a) the 5-point Laplacian in ELLPACK and (b) the skewed matrix of tests/spmm_cases.py (power-law rows, one dense row) in the
sliced format.  Not a test, no threshold.  Per matrix one line with the medians, the run-to-run band of each, device / host,
refresh / device, and the share of the device set-up that is still host work (row-pointer download, checks on them and
dla::sell_layout; the library reports it under $DIAGLIB_AMD_HOSTTIME, which this tool switches on for itself): that share says
whether moving the layout to the device would be worth a later change.  The products of the three are compared bit for bit.

python tools/time_spmm_setup.py [n] [rounds] >> profiles/spmm_setup.txt"""
import os
import platform
import re
import sys
import tempfile
import time

os.environ["DIAGLIB_AMD_HOSTTIME"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
from diaglib_amd import capi  # noqa: E402
from spmm_cases import skewed_csr  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
M = 4
ctx = capi.Context()
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
MV = capi.fn_address("dla_spmm_matvec")
x, ax = ctx.panel(n, M), ctx.panel(n, M)
ctx.random_fill(x)


def product():
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, MV, n, M, x.ptr, ax.ptr))
    return ax.download()


def wall(f):
    ctx.sync()
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)          # (all three calls are synchronous)


def leg(name, csr, fmt):
    rp, ci, va = csr
    va2 = va * (1.0 + 0.5 * np.sin(np.arange(va.size)))
    d = [torch.from_numpy(a).cuda() for a in (rp, ci, va, va2)]
    torch.cuda.synchronize()
    f = capi.SPMM_FORMATS[fmt]
    ms = {"host": [], "device": [], "refresh": []}
    same = True
    for _ in range(rounds):
        ms["host"].append(wall(lambda: ctx._chk(ctx.lib.dla_spmm_setup_csr_fmt(ctx.h, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, f))))
        want = product()
        ms["device"].append(wall(lambda: ctx._chk(ctx.lib.dla_spmm_setup_csr_dev(ctx.h, 0, n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), f))))
        same &= np.array_equal(product().view(np.uint64), want.view(np.uint64))
        ms["refresh"].append(wall(lambda: ctx._chk(ctx.lib.dla_spmm_refresh_values_dev(ctx.h, 0, n, d[0].data_ptr(), d[1].data_ptr(), d[3].data_ptr()))))
        got = product()
        ctx._chk(ctx.lib.dla_spmm_setup_csr_fmt(ctx.h, n, rp.ctypes.data, ci.ctypes.data, va2.ctypes.data, f))
        same &= np.array_equal(got.view(np.uint64), product().view(np.uint64))
    info = ctx.spmm_info()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    band = {k: 100.0 * (max(v) - min(v)) / med[k] for k, v in ms.items()}
    return name, info, med, band, same


def host_parts():
    """the library's own account of the host part of the device set-ups, printed when the context goes: {format: ms per call}"""
    keep = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        os.dup2(tmp.fileno(), 2)
        try:
            ctx.destroy()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    out = {}
    for fmt, total, calls in re.findall(r"spmm_setup_csr_dev host part, (\w+)\s+([0-9.]+) ms\s+(\d+) calls", text):
        out[fmt] = float(total) / int(calls)
    return out


print(f"# tools/time_spmm_setup.py n={n} rounds={rounds} backend={ctx.backend} host={platform.processor() or platform.machine()} "
      f"cpus={os.cpu_count()} torch={torch.__version__}")
nx = 2000
t = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])  # noqa: E731
lap = (sp.kron(sp.identity(n // nx), t(nx)) + sp.kron(t(n // nx), sp.identity(nx))).tocsr() if n % nx == 0 and n > nx else t(n).tocsr()
legs = [leg("5-point laplacian", (np.ascontiguousarray(lap.indptr, np.int64), np.ascontiguousarray(lap.indices, np.int32),
                                  np.ascontiguousarray(lap.data, np.float64)), "ell"),
        leg("skewed seed 7", skewed_csr(np.random.default_rng(7), n), "sell")]
x.free(); ax.free()
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
parts = host_parts()
for name, info, med, band, same in legs:
    part = parts.get(info["format"])
    share = f"{100.0 * part / med['device']:5.1f} % ({part:.1f} ms)" if part is not None else "not reported"
    print(f"{name:18s} {info['format']:4s} nnz {info['nnz']:10d} stored {info['stored'] + info['long_entries']:10d} | host {med['host']:9.1f} ms (band {band['host']:4.1f} %)  "
          f"device {med['device']:8.1f} ms (band {band['device']:4.1f} %)  refresh {med['refresh']:8.1f} ms (band {band['refresh']:4.1f} %) | "
          f"device / host {med['device'] / med['host']:6.3f}  refresh / device {med['refresh'] / med['device']:6.3f}  host share of device set-up {share}  "
          f"same bits {same}", flush=True)
