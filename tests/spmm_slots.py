"""Test helper: one spelling of the plumbing of the sparse GPU tests.  A context stores six sparse matrices -- the operator A, the
metric B and the four parts of a linear-response pencil -- and every one of them is set up, refreshed, asked about and multiplied by
through the same few calls; the helpers here take the slot they act on.

A slot is "A", "B" or a part name ("apb", "amb", "spd", "smd").  The public numbering is accepted too: 0 / 1 are the `which` of the
device-array entries (A / B), ("which", k) and ("part", k) pass a raw number through -- the way to reach an out-of-range one."""
import contextlib
import ctypes as C

import numpy as np

from diaglib_amd import capi
from spmm_lr_cases import MUL, PARTS
from test_operators_gpu import Guarded, call_matvec, call_precnd

FMT = capi.SPMM_FORMATS
SLOTS = ("A", "B") + PARTS
CALL = dict({"A": "dla_spmm_matvec", "B": "dla_spmm_bvec"}, **MUL)
# family -> the device set-up, the refresh and the info entry (the host set-ups have one entry per slot of "main": host_entry)
_ENTRIES = {"main": ("dla_spmm_setup_csr_dev", "dla_spmm_refresh_values_dev", None),
            "part": ("dla_spmm_setup_lr_csr_dev", "dla_spmm_refresh_lr_values_dev", "dla_spmm_lr_info")}


def slot_number(slot):
    """(family, number): ("main", which) or ("part", part)"""
    if isinstance(slot, tuple):
        return {"which": "main", "part": "part"}[slot[0]], int(slot[1])
    if isinstance(slot, str) and slot in PARTS:
        return "part", capi.SPMM_LR_PARTS[slot]
    return "main", {"A": 0, "B": 1, 0: 0, 1: 1}[slot]


def slot_name(slot):
    family, k = slot_number(slot)
    return PARTS[k] if family == "part" else "AB"[k]


def _fmt(fmt):
    return FMT[fmt] if isinstance(fmt, str) else fmt


def _address(a):
    return a if isinstance(a, int) else a.ctypes.data


def host_entry(slot, fmt):
    """name and leading arguments of the host set-up of a slot; fmt None: dla_spmm_setup_csr, the entry without a format (A only)"""
    family, k = slot_number(slot)
    if family == "part":
        return "dla_spmm_setup_lr_csr", (k,)
    return ("dla_spmm_setup_metric_csr" if k else "dla_spmm_setup_csr" if fmt is None else "dla_spmm_setup_csr_fmt"), ()


def setup_status(ctx, slot, n, indptr, indices, data, fmt, where="host"):
    """status of one set-up.  host: numpy arrays, or addresses (0: a null array).  device: numpy arrays, which travel to the device and
    are poisoned the moment the call has returned, or device addresses"""
    if where == "host":
        entry, lead = host_entry(slot, fmt)
        tail = () if fmt is None else (_fmt(fmt),)
        return getattr(ctx.lib, entry)(ctx.h, *lead, n, _address(indptr), _address(indices), _address(data), *tail)
    assert where == "device", where
    family, k = slot_number(slot)
    return _device_call(ctx, _ENTRIES[family][0], k, n, (indptr, indices, data), (_fmt(fmt),))


def refresh_status(ctx, slot, n, indptr, indices, data):
    family, k = slot_number(slot)
    return _device_call(ctx, _ENTRIES[family][1], k, n, (indptr, indices, data), ())


def _device_call(ctx, entry, k, n, arrays, tail):
    if all(isinstance(a, int) for a in arrays):
        return getattr(ctx.lib, entry)(ctx.h, k, n, *arrays, *tail)
    t = to_device(*arrays)
    st = getattr(ctx.lib, entry)(ctx.h, k, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), *tail)
    poison(t)
    return st


def setup(ctx, slot, n, indptr, indices, data, fmt, where="host"):
    """one slot from raw CSR arrays (unsorted columns, duplicates: scipy would clean them)"""
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
    ctx._chk(setup_status(ctx, slot, n, indptr, indices, data, fmt, where))


def refresh(ctx, slot, n, indptr, indices, data):
    """new values for the pattern a slot holds, from device arrays"""
    ctx._chk(refresh_status(ctx, slot, n, indptr, indices, data))


def info_status(ctx, slot, out):
    family, k = slot_number(slot)
    if family == "part":
        return ctx.lib.dla_spmm_lr_info(ctx.h, k, C.byref(out))
    return (ctx.lib.dla_spmm_metric_info if k else ctx.lib.dla_spmm_info)(ctx.h, C.byref(out))


def info(ctx, slot):
    family, k = slot_number(slot)
    return ctx.spmm_lr_info(k) if family == "part" else ctx.spmm_metric_info() if k else ctx.spmm_info()


def last_error(ctx):
    return ctx.lib.dla_last_error(ctx.h).decode()


def product(ctx, slot_or_name, x):
    """one product of a slot (or of the named callback) on x, between sentinel columns; the input must come back unchanged"""
    name = slot_or_name if str(slot_or_name).startswith("dla_") else CALL[slot_name(slot_or_name)]
    n, m = x.shape
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    call_matvec(ctx, name, n, m, gx.ptr, gy.ptr)
    got = gy.body().copy()
    gx.assert_unchanged()
    gx.free(); gy.free()
    return got


def precnd(ctx, name, x, fac=-1.25):
    n, m = x.shape
    gx, gy = Guarded(ctx, n, m, x), Guarded(ctx, n, m)
    call_precnd(ctx, name, n, m, fac, gx.ptr, gy.ptr)
    got = gy.body().copy()
    gx.free(); gy.free()
    return got


def to_device(indptr, indices, data):
    import torch
    t = (torch.from_numpy(np.ascontiguousarray(indptr, np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(indices, np.int32)).cuda(),
         torch.from_numpy(np.ascontiguousarray(data, np.float64)).cuda())
    torch.cuda.synchronize()            # the caller's producer has finished
    return t


def poison(tensors):
    """what a caller may do the moment the call has returned"""
    import torch
    crow, col, val = tensors
    crow.fill_(-1); col.fill_(2 ** 31 - 1); val.fill_(float("nan"))
    torch.cuda.synchronize()


def within_scipy_bound(got, a, x):
    """the dot-product bound 64 eps |A| |x| around scipy's product"""
    return np.all(np.abs(got - a @ x) <= 64 * np.finfo(np.float64).eps * (abs(a) @ np.abs(x)) + 1e-300)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def raw(a):
    a = a.tocsr()
    return a.shape[0], a.indptr.astype(np.int64), a.indices.astype(np.int32), a.data.astype(np.float64)


@contextlib.contextmanager
def fresh_context():
    lib = capi.load()
    h = C.c_void_p()
    assert lib.dla_create(C.byref(h), 0) == 0
    c = capi.Context.__new__(capi.Context)
    c.lib, c.h, c._keep, c.sync_python_callbacks = lib, h, [], True
    try:
        c.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
        yield c
    finally:
        c.destroy()
