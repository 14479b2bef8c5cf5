"""CPU: the dense operator's entry points on the host-memory engine (tests/hostsim.py over oracle/hostsim_engine.cpp, which compiles
and links unchanged).  That engine stores no dense matrix: the defaulted bodies of Engine::dense_* answer DLA_ERR_ARG for the four
entries, and the four callbacks fail through the status of dla_call_matvec / dla_call_precnd with their names in the message --
before any set-up has bound a context, and after a (refused) set-up as well: the whole text of dla_last_error is held.
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
a = np.asfortranarray(np.random.default_rng(2).standard_normal((n, n)))
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
x = np.asfortranarray(np.random.default_rng(1).standard_normal((n, m)))
px, py = ctx.panel(x), ctx.panel(np.full((n, m), -7.25, order="F"))
before = py.download()
assert np.all(before == -7.25)
# what each callback says before any set-up has bound a context (host_logic.cpp)
UNBOUND = {{"dla_dense_matvec": "dla_dense_matvec before dla_dense_setup: no dense operator has been set up",
           "dla_dense_bvec": "dla_dense_bvec before dla_dense_setup: no dense metric has been set up",
           "dla_dense_precnd": "dla_dense_precnd before dla_dense_setup: no dense operator has been set up",
           "dla_dense_precnd_pencil": "dla_dense_precnd_pencil before dla_dense_setup: no dense operator has been set up"}}
err = lambda: ctx.lib.dla_last_error(ctx.h).decode()


def callbacks_fail():
    for name in ("dla_dense_matvec", "dla_dense_bvec"):
        st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, px.ptr, py.ptr)
        assert st == capi.ERR_ARG and name in err() and err() == UNBOUND[name], (name, st, err())
    for name in ("dla_dense_precnd", "dla_dense_precnd_pencil"):
        st = ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, -1.25, px.ptr, py.ptr)
        assert st == capi.ERR_ARG and name in err() and err() == UNBOUND[name], (name, st, err())
    assert np.array_equal(py.download(), before)          # a refused call writes nothing


callbacks_fail()                                          # no set-up has bound a context
for which in (0, 1):
    assert ctx.lib.dla_dense_setup(ctx.h, which, n, a.ctypes.data, n) == capi.ERR_ARG
    assert ctx.lib.dla_dense_setup_dev(ctx.h, which, n, px.ptr, n) == capi.ERR_ARG
    assert ctx.lib.dla_dense_info(ctx.h, which, C.byref(capi.DenseInfo())) == capi.ERR_ARG
    assert ctx.lib.dla_dense_drop(ctx.h, which) == capi.ERR_ARG
    assert "dense" in err() and err() == "this engine stores no dense matrix", err()
callbacks_fail()
print("dense operator on the host engine: refused, ok")
"""


def test_the_host_engine_refuses_the_dense_entries_through_the_defaulted_virtuals(tmp_path):
    script = tmp_path / "dense_worker.py"
    script.write_text(WORKER.format(root=ROOT))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "refused, ok" in p.stdout
