#!/usr/bin/env python3
"""The transposed product of the stored sparse operator (dla_spmm_matvec_t: ell_spmm_t_kernel / sell_spmm_t_kernel /
csr_long_segments_t_kernel through the transposed index) beside the two things a caller could do instead.

Per matrix and block width m = 8, 13, 37, alternating call by call on the context's stream after a warm-up, a call timed by device
events around it (the protocol of tools/dense_operator_bench.py --transpose):

  transposed  dla_spmm_matvec_t on slot A            (A^T x through the index: 8 bytes per entry of index, the value gathered)
  forward     dla_spmm_matvec on the same slot A     (A x: what the stored matrix costs in its own direction)
  copy        dla_spmm_bvec on slot B                (A^T x from an explicitly transposed copy in the index's format: 12 bytes per entry)

Reported: the medians, the spread of the per-round medians, the ratios transposed / forward and transposed / copy, the rate of the
transposed product over its booked bytes (include/diaglib_amd.h, Statistics), the device bytes of the index against those of the copy,
and the wall time of dla_spmm_transpose_prepare behind a host and behind a device set-up of A.  Recorded figures, no thresholds.

Matrices: the five-point Laplacian on a 1448 x 1448 grid (the matrix of profiles/cheb_precnd.txt; ELLPACK both ways), and a skewed
matrix with tail rows AND tail columns: skewed_csr of tests/spmm_cases.py (power-law rows, one dense row) with the entries of its own
transpose appended row by row.

Every leg is a process of its own under `timeout`; the first leg that fails ends the run.

    python tools/spmm_transpose_bench.py [rounds] [record]          (defaults 10, profiles/spmm_matvec_t.txt)
"""
import os
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CALLS_PER_ROUND, WIDTHS = 5, (8, 13, 37)
LEGS = [("stencil 1448", 420), ("skewed 200000", 420)]


def stencil(g):
    import scipy.sparse as sp
    t = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(g, g))
    a = (sp.kron(sp.identity(g), t) + sp.kron(t, sp.identity(g))).tocsr()
    return a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def stable_transpose(n, indptr, indices, data):
    order = np.argsort(indices, kind="stable")
    tptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n), out=tptr[1:])
    return tptr, np.ascontiguousarray(rows_of(indptr)[order], dtype=np.int32), np.ascontiguousarray(data[order])


def skewed(n):
    from spmm_cases import skewed_csr
    rng = np.random.default_rng(n)
    indptr, indices, data = skewed_csr(rng, n)
    tptr, tcol, _ = stable_transpose(n, indptr, indices, data)
    # row i: its own entries, then those of column i (new values: the matrix is not symmetric)
    rows = np.concatenate([rows_of(indptr), rows_of(tptr)])
    cols = np.concatenate([indices, tcol])
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return n, ptr, np.ascontiguousarray(cols[order], dtype=np.int32), rng.standard_normal(len(cols))


def leg(kind, size, rounds):
    import torch
    from diaglib_amd import capi
    from spmm_slots import setup
    n, indptr, indices, data = stencil(size) if kind == "stencil" else skewed(size)
    nnz = len(indices)
    ctx = capi.Context()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    stream = torch.cuda.ExternalStream(ctx.lib.dla_stream(ctx.h))
    prepare = {}
    for where in ("device", "host"):
        setup(ctx, "A", n, indptr, indices, data, "auto", where)
        times = []
        for _ in range(4):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.spmm_transpose_prepare("auto")
            times.append((time.perf_counter() - t0) * 1e3)
        prepare[where] = float(np.median(times[1:]))
    ia, it = ctx.spmm_info(), ctx.spmm_transpose_info()
    setup(ctx, "B", n, *stable_transpose(n, indptr, indices, data), it["format"])
    ib = ctx.spmm_metric_info()
    triad = ctx.stream_triad(1 << 25)
    print(f"{kind} n = {n}, nnz = {nnz}: A {ia['format']} ({ia['long_rows']} tail rows), index {it['format']} ({it['long_rows']} tail columns, "
          f"{it['multi_segments']} partial sums); device bytes: index {it['device_bytes'] / 1e6:.1f} MB, transposed copy {ib['device_bytes'] / 1e6:.1f} MB, "
          f"A itself {ia['device_bytes'] / 1e6:.1f} MB; dla_spmm_transpose_prepare {prepare['host']:.2f} ms behind a host set-up, {prepare['device']:.2f} ms "
          f"behind a device set-up; triad {triad:.0f} GB/s", flush=True)
    fns = {"transposed": capi.fn_address("dla_spmm_matvec_t"), "forward": capi.fn_address("dla_spmm_matvec"), "copy": capi.fn_address("dla_spmm_bvec")}
    for m in WIDTHS:
        x, y = ctx.panel(n, m), ctx.panel(n, m)
        ctx.random_fill(x)

        def call(which):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx._chk(ctx.lib.dla_call_matvec(ctx.h, fns[which], n, m, x.ptr, y.ptr))
            e1.record(stream)
            return e0, e1

        for which in tuple(fns) * 3:
            call(which)
        ctx.sync()
        ctx.reset_stats()
        call("transposed")
        ctx.sync()
        booked = ctx.stats()["matvec"]["alg_bytes"]
        ms = {w: [] for w in fns}
        for _ in range(rounds):
            pairs = [(which, call(which)) for _ in range(CALLS_PER_ROUND) for which in fns]
            ctx.sync()
            for which in ms:
                ms[which].append([e0.elapsed_time(e1) for k, (e0, e1) in pairs if k == which])
        med, spread = {}, {}
        for which in ms:
            t = np.array(ms[which])
            per_round = np.median(t, axis=1)
            med[which], spread[which] = float(np.median(t)), float(per_round.max() - per_round.min())
        print(f"  m = {m:2d}  " + "  ".join(f"{w} {med[w]:8.4f} ms (spread {spread[w]:.4f})" for w in fns) +
              f"   transposed / forward = {med['transposed'] / med['forward']:5.2f}   transposed / copy = {med['transposed'] / med['copy']:5.2f}   "
              f"transposed: {booked / 1e6:.1f} MB booked = {booked / (med['transposed'] * 1e-3) / 1e12:5.2f} TB/s", flush=True)
        x.free(); y.free()
    ctx.spmm_drop_transpose()
    ctx.spmm_drop_metric()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return 0
    args = sys.argv[1:]
    rounds = int(args[0]) if args else 10
    record = args[1] if len(args) > 1 else os.path.join(ROOT, "profiles", "spmm_matvec_t.txt")
    text = [f"tools/spmm_transpose_bench.py {rounds}: dla_spmm_matvec_t beside dla_spmm_matvec on the same stored matrix and dla_spmm_bvec on an explicitly "
            f"transposed copy, {rounds * CALLS_PER_ROUND} timed calls each per shape, alternating call by call"]
    for name, limit in LEGS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg"] + name.split() + [str(rounds)]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:                             # (as it comes: a long leg is not silent)
            print(line, end="", flush=True)
            text.append(line.rstrip())
        if p.wait() != 0:
            print(f"leg '{name}' ended with status {p.returncode}: stopping here", flush=True)
            return p.returncode
    with open(record, "w") as f:
        f.write("\n".join(text) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
