"""GPU: the complete text of dla_last_error and the status of every refused call on the stored sparse matrices -- the operator A, the
metric B, one part of the linear-response pencil (amb) and out-of-range slot numbers -- through the eight set-up and refresh entries,
the three info entries and the product / preconditioner callbacks.  The other sparse tests hold these messages by loose patterns only.

The matrix is 8 x 8 and tridiagonal; every call under test is refused before a product kernel runs.  After every refused call the
info and a product with m = 2 of the slots A, B and amb have the bits they had before (where nothing is stored: the same refusal).
The irregular wording -- the doubled prefix for B and the parts, no slot name in the device entries for B -- is what callers read
today and is held as it is."""
import numpy as np
import pytest

from diaglib_amd import capi
from spmm_slots import (CALL, fresh_context, info_status, last_error, refresh_status, setup, setup_status, to_device)
from test_operators_gpu import Guarded, setup_csr_one_shard

pytestmark = pytest.mark.gpu
N, M, NNZ = 8, 2, 22
THREE = ("A", "B", "amb")
X = np.asfortranarray(np.random.default_rng(5).standard_normal((N, M)))
PART_RANGE = "part must be 0 (A+B), 1 (A-B), 2 (S+D) or 3 (S-D)"
WHICH_RANGE = "which must be 0 (the operator) or 1 (the metric)"
SHARDED_B = "the operator of this context is row-sharded, and a row-sharded metric is not supported"
SHARDED_LR = "the operator of this context is row-sharded, and row-sharded linear-response parts are not supported"


def tridiagonal(scale=1.0):
    lens = np.array([2] + [3] * (N - 2) + [2])
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate([np.arange(max(0, i - 1), min(N, i + 2)) for i in range(N)]).astype(np.int32)
    data = scale * (1.0 + np.arange(NNZ, dtype=np.float64) / 8.0)
    assert indptr[-1] == NNZ == indices.size
    return indptr, indices, data


MAT = {"A": tridiagonal(1.0), "B": tridiagonal(-2.0), "amb": tridiagonal(0.5)}


@pytest.fixture()
def c():
    """a context of its own with nothing stored, which the thread's callbacks act on: a REFUSED set-up of A binds it as well"""
    with fresh_context() as ctx:
        assert ctx.lib.dla_spmm_setup_csr(ctx.h, 0, 0, 0, 0) == capi.ERR_ARG and last_error(ctx) == "spmm_setup_csr: bad arguments"
        yield ctx


def fill(ctx, fmt="ell", slots=THREE):
    """(every accepted set-up binds the thread's callbacks to ctx)"""
    for s in slots:
        setup(ctx, s, N, *MAT[s], fmt)


def refused_callback(ctx, trampoline, name, n, fac=None, blocks=2):
    """(status, message) of a callback through its trampoline on blocks of n x M; a refused callback has written nothing"""
    g = [Guarded(ctx, n, M, np.ones((n, M))) for _ in range(blocks // 2)] + [Guarded(ctx, n, M) for _ in range(blocks // 2)]
    args = (n, M) + (() if fac is None else (fac,)) + tuple(b.ptr for b in g)
    st = getattr(ctx.lib, trampoline)(ctx.h, capi.fn_address(name), *args)
    msg = last_error(ctx)
    outputs = [b.body().copy() for b in g[blocks // 2:]]
    for b in g:
        b.free()
    return st, msg, outputs


def state(ctx, slot):
    """info and product of a slot: their bits, or status and message of the refusal"""
    out = capi.SpmmInfo()
    st = info_status(ctx, slot, out)
    inf = bytes(out) if st == 0 else (st, last_error(ctx))
    gx, gy = Guarded(ctx, N, M, X), Guarded(ctx, N, M)
    st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(CALL[slot]), N, M, gx.ptr, gy.ptr)
    y = gy.body().copy()
    prod = y.tobytes() if st == 0 else (st, last_error(ctx), y.tobytes())
    gx.free(); gy.free()
    return inf, prod


def states(ctx):
    return {s: state(ctx, s) for s in THREE}


def assert_refused(ctx, st, text, before=None):
    msg = last_error(ctx)
    assert (st, msg) == (capi.ERR_ARG, text), (st, msg, text)
    if before is not None:
        assert states(ctx) == before, "a refused call changed a slot"


# ------------------------------------------------------------------------------------------------------------------ set-ups
# id: (slot, where, takes a format, the message around the defect's words)
SETUPS = {
    "setup_csr": ("A", "host", False, "spmm_setup_csr: {}"),
    "setup_csr_fmt": ("A", "host", True, "spmm_setup_csr_fmt: {}"),
    "setup_metric_csr": ("B", "host", True, "spmm_setup_metric_csr: spmm_setup_csr_fmt: {}"),
    "setup_lr_csr": ("amb", "host", True, "spmm_setup_lr_csr, part amb (A-B): spmm_setup_csr_fmt: {}"),
    "setup_csr_dev_0": ("A", "device", True, "spmm_setup_csr_dev: {}"),
    "setup_csr_dev_1": ("B", "device", True, "spmm_setup_csr_dev: {}"),
    "setup_lr_csr_dev": ("amb", "device", True, "spmm_setup_lr_csr_dev, part amb (A-B): spmm_setup_csr_dev: {}"),
}


def test_the_column_messages_of_the_issue():
    want = {"setup_csr": "spmm_setup_csr: column index out of range",
            "setup_csr_fmt": "spmm_setup_csr_fmt: column index out of range",
            "setup_metric_csr": "spmm_setup_metric_csr: spmm_setup_csr_fmt: column index out of range",
            "setup_lr_csr": "spmm_setup_lr_csr, part amb (A-B): spmm_setup_csr_fmt: column index out of range",
            "setup_csr_dev_0": "spmm_setup_csr_dev: column index out of range", "setup_csr_dev_1": "spmm_setup_csr_dev: column index out of range",
            "setup_lr_csr_dev": "spmm_setup_lr_csr_dev, part amb (A-B): spmm_setup_csr_dev: column index out of range"}
    assert {k: v[3].format("column index out of range") for k, v in SETUPS.items()} == want


def setup_defects(where, with_format):
    """(what, n, three arrays or addresses, format, the defect's words)"""
    indptr, indices, data = MAT["A"]
    down = indptr.copy(); down[4] = down[3] - 1
    high = indices.copy(); high[9] = N
    low = indices.copy(); low[9] = -1
    out = [("n = 0", 0, (indptr, indices, data), "ell", "bad arguments"),
           ("descending row pointers", N, (down, indices, data), "ell", "row pointers not ascending"),
           ("empty matrix", N, (np.zeros(N + 1, np.int64), indices, data), "ell", "empty matrix"),
           ("column n", N, (indptr, high, data), "ell", "column index out of range"),
           ("column n, sell", N, (indptr, high, data), "sell", "column index out of range"),
           ("column -1", N, (indptr, low, data), "auto", "column index out of range")]
    if with_format:
        out.append(("unknown format", N, (indptr, indices, data), 3, "unknown format"))
    keep = to_device(indptr, indices, data) if where == "device" else None
    ptrs = [t.data_ptr() for t in keep] if keep else [a.ctypes.data for a in (indptr, indices, data)]
    for k in range(3):
        out.append((f"null array {k}", N, tuple(0 if j == k else ptrs[j] for j in range(3)), "ell", "bad arguments"))
    return out, keep


@pytest.mark.parametrize("stored", [None, "ell", "sell"], ids=["nothing stored", "ell stored", "sell stored"])
@pytest.mark.parametrize("entry", list(SETUPS))
def test_refused_setups(c, entry, stored):
    slot, where, with_format, text = SETUPS[entry]
    if stored:
        fill(c, stored)
    before = states(c)
    defects, keep = setup_defects(where, with_format)
    for what, n, arrays, fmt, words in defects:
        st = setup_status(c, slot, n, *arrays, fmt if with_format else None, where)
        assert_refused(c, st, text.format(words), before)
    del keep


# ------------------------------------------------------------------------------------------------------------------ refreshes
REFRESHES = {"A": "spmm_refresh_values_dev: {}", "B": "spmm_refresh_values_dev: {}",
             "amb": "spmm_refresh_lr_values_dev, part amb (A-B): spmm_refresh_values_dev: {}"}
NOT_SET_UP = {"A": "spmm_refresh_values_dev: no operator has been set up", "B": "spmm_refresh_values_dev: no metric has been set up",
              "amb": "spmm_refresh_lr_values_dev: part amb (A-B) has not been set up"}


@pytest.mark.parametrize("slot", THREE)
def test_refresh_before_any_setup(c, slot):
    before = states(c)
    assert_refused(c, refresh_status(c, slot, N, *MAT[slot]), NOT_SET_UP[slot], before)
    assert_refused(c, refresh_status(c, slot, N, 0, 0, 0), NOT_SET_UP[slot], before)      # (asked before the arrays are looked at)
    fill(c, "sell", [s for s in THREE if s != slot])
    before = states(c)
    assert_refused(c, refresh_status(c, slot, N, *MAT[slot]), NOT_SET_UP[slot], before)


@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("slot", THREE)
def test_refused_refreshes(c, slot, fmt):
    fill(c, fmt)
    before = states(c)
    indptr, indices, data = MAT[slot]
    text = REFRESHES[slot]
    keep = to_device(indptr, indices, data)
    ptrs = [t.data_ptr() for t in keep]
    for k in range(3):
        assert_refused(c, refresh_status(c, slot, N, *(0 if j == k else ptrs[j] for j in range(3))), text.format("bad arguments"), before)
    assert_refused(c, refresh_status(c, slot, 0, *ptrs), text.format("bad arguments"), before)
    longer = np.append(indptr, indptr[-1])
    assert_refused(c, refresh_status(c, slot, N + 1, longer, indices, data), text.format("n = 9 differs from the stored 8"), before)
    more = indptr.copy(); more[-1] += 1
    assert_refused(c, refresh_status(c, slot, N, more, np.append(indices, 0).astype(np.int32), np.append(data, 1.0)),
                   text.format("23 entries, the stored matrix has 22"), before)
    swapped = indptr.copy(); swapped[1] = 3            # (rows 0 and 1: 3 and 2 entries)
    assert_refused(c, refresh_status(c, slot, N, swapped, indices, data), text.format("the row pointers are not the stored pattern's"), before)
    other = indices.copy(); other[9] = (other[9] + 3) % N
    assert_refused(c, refresh_status(c, slot, N, indptr, other, data), text.format("the columns are not the stored pattern's"), before)
    del keep


# ------------------------------------------------------------------------------------------------------------------ slot numbers
@pytest.mark.parametrize("bad", [4, -1])
def test_a_part_out_of_range(c, bad):
    fill(c)
    before = states(c)
    indptr, indices, data = MAT["amb"]
    slot = ("part", bad)
    assert_refused(c, setup_status(c, slot, N, indptr, indices, data, "ell"), "spmm_setup_lr_csr: " + PART_RANGE, before)
    assert_refused(c, setup_status(c, slot, N, 8, 8, 8, "ell", "device"), "spmm_setup_lr_csr_dev: " + PART_RANGE, before)      # (no pointer is used)
    assert_refused(c, refresh_status(c, slot, N, 8, 8, 8), "spmm_refresh_lr_values_dev: " + PART_RANGE, before)
    assert_refused(c, info_status(c, slot, capi.SpmmInfo()), "spmm_lr_info: " + PART_RANGE, before)


@pytest.mark.parametrize("bad", [2, -1])
def test_a_which_out_of_range(c, bad):
    fill(c)
    before = states(c)
    slot = ("which", bad)
    assert_refused(c, setup_status(c, slot, N, 8, 8, 8, "ell", "device"), "spmm_setup_csr_dev: " + WHICH_RANGE, before)
    assert_refused(c, refresh_status(c, slot, N, 8, 8, 8), "spmm_refresh_values_dev: " + WHICH_RANGE, before)


# ------------------------------------------------------------------------------------------------------------------ info, products, preconditioners
MATVEC, PRECND, LRPREC = "dla_call_matvec", "dla_call_precnd", "dla_call_lrprec"
NO_A, NO_B = "no operator has been set up", "no metric has been set up (dla_spmm_setup_metric_csr)"
NO_AMB, NO_APB = ("part amb (A-B) has not been set up (dla_spmm_setup_lr_csr)", "part apb (A+B) has not been set up (dla_spmm_setup_lr_csr)")


def test_info_and_callbacks_before_any_setup(c):
    out = capi.SpmmInfo()
    assert_refused(c, info_status(c, "A", out), "spmm_info: no operator has been set up")
    assert_refused(c, info_status(c, "B", out), "spmm_metric_info: no metric has been set up")
    assert_refused(c, info_status(c, "amb", out), "spmm_lr_info: part amb (A-B) has not been set up")
    assert c.lib.dla_spmm_drop_metric(c.h) == 0 and c.lib.dla_spmm_drop_lr(c.h) == 0          # (nothing to drop: no error)
    for tramp, name, fac, blocks, text in [
            (MATVEC, "dla_spmm_matvec", None, 2, "spmm_matvec failed: spmm_matvec: n differs from setup"),
            (MATVEC, "dla_spmm_bvec", None, 2, "dla_spmm_bvec failed: spmm_bvec: " + NO_B),
            (MATVEC, "dla_spmm_ambmul", None, 2, "dla_spmm_ambmul failed: spmm_ambmul: " + NO_AMB),
            (PRECND, "dla_spmm_precnd", 0.3, 2, "spmm_precnd failed: spmm_precnd: n differs from setup"),
            (PRECND, "dla_spmm_precnd_pencil", 0.3, 2, "dla_spmm_precnd_pencil failed: spmm_precnd_pencil: " + NO_A),
            (LRPREC, "dla_spmm_lrprec1", 0.3, 4, "dla_spmm_lrprec1 failed: spmm_lrprec1: " + NO_APB),
            (LRPREC, "dla_spmm_lrprec2", 0.3, 4, "dla_spmm_lrprec2 failed: spmm_lrprec2: " + NO_APB)]:
        st, msg, outputs = refused_callback(c, tramp, name, N, fac, blocks)
        assert (st, msg) == (capi.ERR_ARG, text), (name, st, msg)
        assert all(np.all(y == 7.0) for y in outputs), name
    fill(c, "ell", ["A"])
    st, msg, _ = refused_callback(c, PRECND, "dla_spmm_precnd_pencil", N, 0.3)
    assert (st, msg) == (capi.ERR_ARG, "dla_spmm_precnd_pencil failed: spmm_precnd_pencil: " + NO_B)


@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_callbacks_with_one_row_more(c, fmt):
    fill(c, fmt)
    for p in ("apb", "spd"):
        setup(c, p, N, *MAT["amb"], fmt)
    before = states(c)
    for tramp, name, fac, blocks, text in [
            (MATVEC, "dla_spmm_matvec", None, 2, "spmm_matvec failed: spmm_matvec: n differs from setup"),
            (MATVEC, "dla_spmm_bvec", None, 2, "dla_spmm_bvec failed: spmm_bvec: n differs from the metric's"),
            (MATVEC, "dla_spmm_ambmul", None, 2, "dla_spmm_ambmul failed: spmm_ambmul: n = 9 differs from the 8 rows of part amb (A-B)"),
            (PRECND, "dla_spmm_precnd", 0.3, 2, "spmm_precnd failed: spmm_precnd: n differs from setup"),
            (PRECND, "dla_spmm_precnd_pencil", 0.3, 2, "dla_spmm_precnd_pencil failed: spmm_precnd_pencil: n differs from setup"),
            (LRPREC, "dla_spmm_lrprec1", 0.3, 4, "dla_spmm_lrprec1 failed: spmm_lrprec1: n = 9 differs from the 8 rows of part apb (A+B)"),
            (LRPREC, "dla_spmm_lrprec2", 0.3, 4, "dla_spmm_lrprec2 failed: spmm_lrprec2: n = 9 differs from the 8 rows of part apb (A+B)")]:
        st, msg, outputs = refused_callback(c, tramp, name, N + 1, fac, blocks)
        assert (st, msg) == (capi.ERR_ARG, text), (name, st, msg)
        assert all(np.all(y == 7.0) for y in outputs), name
        assert states(c) == before


# ------------------------------------------------------------------------------------------------------------------ a row-sharded A
def shard(ctx):
    indptr, indices, data = MAT["A"]
    gi = np.ascontiguousarray(indices, dtype=np.int64)
    return ctx.lib.dla_spmm_setup_csr_sharded(ctx.h, N, 0, N, indptr.ctypes.data, gi.ctypes.data, data.ctypes.data)


def test_b_and_the_parts_beside_a_sharded_operator(c):
    setup_csr_one_shard(c, N, *MAT["A"])
    before = states(c)
    assert isinstance(before["A"][1], bytes), before["A"]
    assert_refused(c, setup_status(c, "B", N, *MAT["B"], "ell"), "spmm_setup_metric_csr: " + SHARDED_B, before)
    assert_refused(c, setup_status(c, "B", N, *MAT["B"], "ell", "device"), "spmm_setup_csr_dev: " + SHARDED_B, before)
    assert_refused(c, setup_status(c, "amb", N, *MAT["amb"], "ell"), "spmm_setup_lr_csr: " + SHARDED_LR, before)
    assert_refused(c, setup_status(c, "amb", N, *MAT["amb"], "ell", "device"), "spmm_setup_lr_csr_dev: " + SHARDED_LR, before)
    assert_refused(c, refresh_status(c, "A", N, *MAT["A"]), "spmm_refresh_values_dev: the operator of this context is row-sharded", before)
    assert_refused(c, refresh_status(c, "B", N, *MAT["B"]), NOT_SET_UP["B"], before)
    assert_refused(c, refresh_status(c, "amb", N, *MAT["amb"]), "spmm_refresh_lr_values_dev: " + SHARDED_LR, before)
    # a refused set-up of A leaves it sharded, an accepted one through any other entry makes it whole
    assert_refused(c, setup_status(c, "A", 0, *MAT["A"], "ell"), "spmm_setup_csr_fmt: bad arguments", before)
    assert_refused(c, setup_status(c, "B", N, *MAT["B"], "ell"), "spmm_setup_metric_csr: " + SHARDED_B, before)
    for where, fmt in (("host", None), ("host", "sell"), ("device", "ell")):
        assert shard(c) == 0
        assert setup_status(c, "A", N, *MAT["A"], fmt, where) == 0
        assert setup_status(c, "B", N, *MAT["B"], "ell") == 0 and c.lib.dla_spmm_drop_metric(c.h) == 0


def test_the_sharded_setup_beside_b_or_a_part(c):
    held_b = ("spmm_setup_csr_sharded: this context holds a metric (dla_spmm_setup_metric_csr), and a row-sharded metric is not supported; "
              "drop it first")
    held_lr = ("spmm_setup_csr_sharded: this context holds linear-response parts (dla_spmm_setup_lr_csr), and row-sharded parts are not "
               "supported; drop them first (dla_spmm_drop_lr)")
    fill(c, "ell", ["A", "B"])
    before = states(c)
    assert_refused(c, shard(c), held_b, before)
    setup(c, "amb", N, *MAT["amb"], "sell")
    before = states(c)
    assert_refused(c, shard(c), held_lr, before)
    assert c.lib.dla_spmm_drop_metric(c.h) == 0
    before = states(c)
    assert_refused(c, shard(c), held_lr, before)
    assert c.lib.dla_spmm_drop_lr(c.h) == 0 and shard(c) == 0


# ------------------------------------------------------------------------------------------------------------------ the thread's context
def test_which_setups_bind_the_threads_context(c):
    """the callbacks act on the context bound last: every set-up of A binds its context even when it is refused, a set-up of B or of
    a part only when it is accepted; info, refresh and drop never do"""
    fill(c)
    ok = "A product of the first context"
    with fresh_context() as d:
        def reaches_c():
            gx, gy = Guarded(c, N, M, X), Guarded(c, N, M)
            st = c.lib.dla_call_matvec(c.h, capi.fn_address("dla_spmm_matvec"), N, M, gx.ptr, gy.ptr)
            gx.free(); gy.free()
            return st == 0
        assert reaches_c(), ok
        down = MAT["B"][0].copy(); down[4] = 0
        for slot, where in (("B", "host"), ("amb", "host"), ("B", "device"), ("amb", "device")):
            assert setup_status(d, slot, N, down, *MAT["B"][1:], "ell", where) == capi.ERR_ARG
            assert reaches_c(), (slot, where)
        assert info_status(d, "A", capi.SpmmInfo()) == capi.ERR_ARG and refresh_status(d, "A", N, *MAT["A"]) == capi.ERR_ARG
        assert d.lib.dla_spmm_drop_metric(d.h) == 0 and d.lib.dla_spmm_drop_lr(d.h) == 0 and reaches_c()
        for slot, where in (("B", "host"), ("amb", "device")):
            assert setup_status(d, slot, N, *MAT["B"], "ell", where) == 0
            assert not reaches_c(), (slot, where)
            assert c.lib.dla_spmm_setup_csr(c.h, 0, 0, 0, 0) == capi.ERR_ARG and reaches_c()
        for refused_a in (lambda: setup_status(d, "A", N, down, *MAT["A"][1:], None), lambda: setup_status(d, "A", N, down, *MAT["A"][1:], "sell"),
                          lambda: setup_status(d, "A", N, down, *MAT["A"][1:], "ell", "device"),
                          lambda: d.lib.dla_spmm_setup_csr_sharded(d.h, 0, 0, N, 0, 0, 0)):
            assert refused_a() == capi.ERR_ARG
            assert not reaches_c()
            assert c.lib.dla_spmm_setup_csr(c.h, 0, 0, 0, 0) == capi.ERR_ARG and reaches_c()
        assert c.lib.dla_spmm_setup_csr(c.h, 0, 0, 0, 0) == capi.ERR_ARG      # (d goes away: the callbacks act on c again)
