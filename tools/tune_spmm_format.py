#!/usr/bin/env python3
"""A/B of the two storage formats of the sparse operator (dla_spmm_setup_csr_fmt: ELLPACK against sliced ELLPACK with a CSR
tail) in one process, alternating the formats round by round, timed by the engine's HIP events (DLA_OPT_PROFILE), with a
comparison of the two results.

  (a) the matrices ELLPACK was built for: a 5-point Laplacian and a band of half-width 6
  (b) ragged matrices whose ELLPACK padding w n / nnz is 1.1, 1.25, 1.5, 2 and 4 (w = 16, rows capped so that ELLPACK fits):
      where the two curves cross is where DLA_SPMM_AUTO should change its mind
  (c) the skewed matrices of tests/spmm_cases.py (power-law rows, one dense row), sliced format only: the tail as the layout
      cut it (long_rows, long_segments of long_segment_entries entries, multi_segments = partial sums per right-hand side) and
      one product as (12 (stored + long_entries) + 4 n + 16 n m) / time beside the STREAM triad of the same run.  This is the
      leg to repeat when dla::SELL_LONG_SEG is tuned: build with each candidate and compare the lines (legs = c)

python tools/tune_spmm_format.py [n] [m] [rounds] [legs = abc] >> profiles/spmm_formats.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
from diaglib_amd import capi  # noqa: E402
from spmm_cases import skewed_csr  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2_000_000
m = int(sys.argv[2]) if len(sys.argv) > 2 else 13
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
legs = sys.argv[4] if len(sys.argv) > 4 else "abc"
REPS = 20
ctx = capi.Context()
ctx.set_option(capi.OPT_PROFILE, 1)
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
MV = capi.fn_address("dla_spmm_matvec")
x, ax = ctx.panel(n, m), ctx.panel(n, m)
ctx.random_fill(x)


def setup(csr, fmt):
    rp, ci, va = csr
    ctx._chk(ctx.lib.dla_spmm_setup_csr_fmt(ctx.h, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, capi.SPMM_FORMATS[fmt]))
    return ctx.spmm_info()


def product_ms():
    """event time of one product in ms (mean of REPS after two warm-up calls), and the result"""
    for _ in range(2):
        ctx._chk(ctx.lib.dla_call_matvec(ctx.h, MV, n, m, x.ptr, ax.ptr))
    ctx.reset_stats()
    for _ in range(REPS):
        ctx._chk(ctx.lib.dla_call_matvec(ctx.h, MV, n, m, x.ptr, ax.ptr))
    ctx.sync()
    s = ctx.stats()["matvec"]
    assert s["launches"] == REPS, s
    return s["ms"] / REPS


def sell_bytes(info):
    return 12.0 * (info["stored"] + info["long_entries"]) + 4.0 * n + 16.0 * n * m


def raw(a):
    a = a.tocsr()
    return np.ascontiguousarray(a.indptr, np.int64), np.ascontiguousarray(a.indices, np.int32), np.ascontiguousarray(a.data, np.float64)


def ab(name, csr):
    """alternate ELL and SELL; medians, the run-to-run band of each, SELL / ELL and the difference of the results"""
    ms = {"ell": [], "sell": []}
    out, info = {}, {}
    for _ in range(rounds):
        for fmt in ("ell", "sell"):
            info[fmt] = setup(csr, fmt)
            ms[fmt].append(product_ms())
            out[fmt] = ax.download()
    same = np.array_equal(out["ell"], out["sell"])
    med = {f: float(np.median(v)) for f, v in ms.items()}
    band = {f: (max(v) - min(v)) / med[f] for f, v in ms.items()}
    nnz = info["ell"]["nnz"]
    print(f"{name:28s} nnz {nnz:10d}  padding ell {info['ell']['stored'] / nnz:5.2f} sell {(info['sell']['stored'] + info['sell']['long_entries']) / nnz:5.2f} | "
          f"ell {med['ell']:7.3f} ms (band {100 * band['ell']:4.1f} %)  sell {med['sell']:7.3f} ms (band {100 * band['sell']:4.1f} %)  "
          f"sell / ell {med['sell'] / med['ell']:5.3f}  same bits {same}", flush=True)


def two_lengths(rng, w, short, padding):
    """a share of the rows has w entries, the others `short`, in random order, so that w n / nnz = padding; columns within 512 rows
    of the diagonal (the gathers cost both formats the same)"""
    share = (w / padding - short) / (w - short)
    lens = np.where(rng.random(n) < share, w, short).astype(np.int64)
    lens[0] = w
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    cols = np.clip(rows + rng.integers(-512, 513, rows.size), 0, n - 1).astype(np.int32)
    return indptr, cols, rng.standard_normal(rows.size)


print(f"# tools/tune_spmm_format.py n={n} m={m} rounds={rounds} reps={REPS} backend={ctx.backend}")
triad = ctx.stream_triad(32 * 1024 * 1024, 5)
print(f"# STREAM triad of this run: {triad:.0f} GB/s")
rng = np.random.default_rng(3)
if "a" in legs:
    print("# (a) stencil and band")
    nx = 2000
    t = lambda k: sp.diags([-np.ones(k - 1), 2 * np.ones(k), -np.ones(k - 1)], [-1, 0, 1])  # noqa: E731
    ab("5-point laplacian", raw(sp.kron(sp.identity(n // nx), t(nx)) + sp.kron(t(n // nx), sp.identity(nx))) if n % nx == 0 else raw(t(n)))
    half = 6
    band = sp.diags([rng.standard_normal(n - k) for k in range(1, half + 1)], list(range(1, half + 1)), shape=(n, n))
    ab("band, half-width 6", raw(band + band.T + sp.diags(np.arange(1.0, n + 1.0))))
if "b" in legs:
    print("# (b) ragged: rows of 16 or 2 entries in random order")
    for padding in (1.1, 1.25, 1.5, 2.0, 4.0):
        ab(f"ragged, ell padding {padding:4.2f}", two_lengths(rng, 16, 2, padding))
if "c" in legs:
    print("# (c) skewed (power-law rows, one dense row): sliced format only")
    for seed in (7, 8, 9):
        info = setup(skewed_csr(np.random.default_rng(seed), n), "sell")
        ms = [product_ms() for _ in range(rounds)]
        med = float(np.median(ms))
        gbs = sell_bytes(info) / med / 1e6
        print(f"skewed seed {seed}: nnz {info['nnz']}  stored + long {(info['stored'] + info['long_entries']) / info['nnz']:.3f} x nnz  long rows {info['long_rows']}  "
              f"long segments {info['long_segments']} of {info['long_segment_entries']}  multi segments {info['multi_segments']}  "
              f"device {info['device_bytes'] / 2 ** 20:.0f} MiB | m = {m}: {med:7.3f} ms (min {min(ms):7.3f} max {max(ms):7.3f}, band {100 * (max(ms) - min(ms)) / med:4.1f} %)  "
              f"{gbs:6.0f} GB/s algorithmic = {gbs / triad:.3f} x triad", flush=True)
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
ctx.set_option(capi.OPT_PROFILE, 0)
