"""CPU: the dense linear-response entry points on the host-memory engine (tests/hostsim.py over oracle/hostsim_engine.cpp, which
compiles and links unchanged).  That engine stores no dense matrix: the defaulted bodies of Engine::dense_setup .. dense_lrprec
answer DLA_ERR_ARG for the six set-up, info and drop entries, and the six callbacks fail through the status of dla_call_matvec /
dla_call_lrprec with their names in the message -- before any set-up has bound a context, and after the (refused) set-ups as well:
the whole text of dla_last_error is held.
(A process of its own: the library a process has loaded cannot be exchanged.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import ctypes as C, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import hostsim
from diaglib_amd import capi
capi.load(hostsim.build())
ctx = capi.Context()
assert ctx.backend.startswith("hostsim")
n, m = 40, 3
rng = np.random.default_rng(2)
a, b = (np.asfortranarray(rng.standard_normal((n, n))) for _ in range(2))
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
x = np.asfortranarray(np.random.default_rng(1).standard_normal((n, m)))
px, pxm = ctx.panel(x), ctx.panel(x)
py, pym = (ctx.panel(np.full((n, m), -7.25, order="F")) for _ in range(2))
before = py.download()
assert np.all(before == -7.25)
err = lambda: ctx.lib.dla_last_error(ctx.h).decode()
# what each callback says before any set-up has bound a context (host_logic.cpp)
UNBOUND = {{"dla_dense_apbmul": "dla_dense_apbmul before dla_dense_setup_lr: no dense part apb (A+B) has been set up",
           "dla_dense_ambmul": "dla_dense_ambmul before dla_dense_setup_lr: no dense part amb (A-B) has been set up",
           "dla_dense_spdmul": "dla_dense_spdmul before dla_dense_setup_lr: no dense part spd (S+D) has been set up",
           "dla_dense_smdmul": "dla_dense_smdmul before dla_dense_setup_lr: no dense part smd (S-D) has been set up",
           "dla_dense_lrprec1": "dla_dense_lrprec1 before dla_dense_setup_lr: no dense part has been set up",
           "dla_dense_lrprec2": "dla_dense_lrprec2 before dla_dense_setup_lr: no dense part has been set up"}}


def callbacks_fail():
    for name in ("dla_dense_apbmul", "dla_dense_ambmul", "dla_dense_spdmul", "dla_dense_smdmul"):
        st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, px.ptr, py.ptr)
        assert st == capi.ERR_ARG and name in err() and err() == UNBOUND[name], (name, st, err())
    for name in ("dla_dense_lrprec1", "dla_dense_lrprec2"):
        st = ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(name), n, m, -1.25, px.ptr, pxm.ptr, py.ptr, pym.ptr)
        assert st == capi.ERR_ARG and name in err() and err() == UNBOUND[name], (name, st, err())
    assert np.array_equal(py.download(), before) and np.array_equal(pym.download(), before)    # a refused call writes nothing


def refused(st):
    assert st == capi.ERR_ARG and "dense" in err() and err() == "this engine stores no dense matrix", (st, err())


callbacks_fail()                                          # no set-up has bound a context
for part in range(4):
    refused(ctx.lib.dla_dense_setup_lr(ctx.h, part, n, a.ctypes.data, n))
    refused(ctx.lib.dla_dense_setup_lr_dev(ctx.h, part, n, px.ptr, n))
    refused(ctx.lib.dla_dense_lr_info(ctx.h, part, C.byref(capi.DenseInfo())))
for pair in range(2):
    refused(ctx.lib.dla_dense_setup_lr_pair(ctx.h, pair, n, a.ctypes.data, n, b.ctypes.data, n))
    refused(ctx.lib.dla_dense_setup_lr_pair_dev(ctx.h, pair, n, px.ptr, n, pxm.ptr, n))
refused(ctx.lib.dla_dense_drop_lr(ctx.h))
callbacks_fail()
print("dense linear-response parts on the host engine: refused, ok")
"""


def test_the_host_engine_refuses_the_dense_lr_entries_through_the_defaulted_virtuals(tmp_path):
    script = tmp_path / "dense_lr_worker.py"
    script.write_text(WORKER.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "refused, ok" in p.stdout
