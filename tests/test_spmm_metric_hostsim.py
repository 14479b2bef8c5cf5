"""CPU: the sparse metric's entry points on the host-memory engine (tests/hostsim.py over oracle/hostsim_engine.cpp).  That engine
stores one sparse matrix, a row-sharded operator, and overrides the product of that matrix alone: the default bodies of the slot
interface answer DLA_ERR_ARG for the product of every other slot and for every set-up, info and drop.  The sparse operator the engine does
implement goes on working, and the callbacks fail through the trampolines' status with their name.
(A process of its own: the library a process has loaded cannot be exchanged.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import ctypes as C, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import scipy.sparse as sp
import hostsim
from diaglib_amd import capi
capi.load(hostsim.build())
ctx = capi.Context()
assert ctx.backend.startswith("hostsim")
n, m = 300, 3
i = np.arange(n, dtype=np.float64)
a = (sp.diags([0.1 * np.cos(i[:-1]), 2.0 + i / 50.0, 0.1 * np.cos(i[:-1])], [-1, 0, 1])).tocsr()
rp, ci, va = a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)
ctx.spmm_setup_sharded(a, 0, n)              # (the only sparse setup this engine has)
for fmt in (capi.SPMM_ELL, capi.SPMM_SELL, capi.SPMM_AUTO):
    assert ctx.lib.dla_spmm_setup_metric_csr(ctx.h, n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, fmt) == capi.ERR_ARG
assert ctx.lib.dla_spmm_metric_info(ctx.h, C.byref(capi.SpmmInfo())) == capi.ERR_ARG
assert ctx.lib.dla_spmm_drop_metric(ctx.h) == capi.ERR_ARG
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
x = np.asfortranarray(np.random.default_rng(1).standard_normal((n, m)))
px, py = ctx.panel(x), ctx.panel(n, m)
st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_spmm_bvec"), n, m, px.ptr, py.ptr)
assert st == capi.ERR_ARG and "dla_spmm_bvec" in ctx.lib.dla_last_error(ctx.h).decode()
st = ctx.lib.dla_call_precnd(ctx.h, capi.fn_address("dla_spmm_precnd_pencil"), n, m, -1.25, px.ptr, py.ptr)
assert st == capi.ERR_ARG and "dla_spmm_precnd_pencil" in ctx.lib.dla_last_error(ctx.h).decode()
# the operator this engine does hold is where it was
ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_spmm_matvec"), n, m, px.ptr, py.ptr))
assert np.abs(py.download() - a @ x).max() < 1e-13
print("metric on the host engine: refused, ok")
"""


def test_the_host_engine_refuses_the_metric_through_the_defaulted_virtuals(tmp_path):
    script = tmp_path / "metric_worker.py"
    script.write_text(WORKER.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "refused, ok" in p.stdout
