"""GPU: the complete text of dla_last_error and the status of every refused call on the stored dense matrices -- the operator A, the
metric B and the four parts of the linear-response pencil -- through the six set-up entries, the two info entries, dla_dense_drop and
the ten product / preconditioner callbacks.  The other dense tests hold these messages by loose patterns only.

The matrices are 8 x 8 (n_pad = 16), random and not symmetric; every call under test is refused before a product kernel runs.  After
every refused call dla_dense_info of both slots, dla_dense_lr_info of the four parts and a product with m = 2 of the operator, the
metric and amb have the bits they had before (where nothing is stored: the same refusal), and a refused callback has written nothing.
The irregular wording -- the set-up entry in parentheses behind a callback's refusal but not behind an info's, "(dla_dense_setup
with which = 1)" from the pencil preconditioner -- is what callers read today and is held as it is."""
import ctypes as C

import numpy as np
import pytest

from diaglib_amd import capi
from spmm_slots import fresh_context, last_error
from test_operators_gpu import SENT, Guarded

pytestmark = pytest.mark.gpu
N, M = 8, 2
PARTS = ("apb", "amb", "spd", "smd")
SLOTS = ("A", "B") + PARTS
THREE = ("A", "B", "amb")
_RNG = np.random.default_rng(11)
MAT = {s: np.asfortranarray(_RNG.standard_normal((N, N))) for s in SLOTS}
X = np.asfortranarray(_RNG.standard_normal((N, M)))
CALL = dict({"A": "dla_dense_matvec", "B": "dla_dense_bvec"}, **{p: f"dla_dense_{p}mul" for p in PARTS})
NOUN = {"A": "dense operator", "B": "dense metric", "apb": "dense part apb (A+B)", "amb": "dense part amb (A-B)",
        "spd": "dense part spd (S+D)", "smd": "dense part smd (S-D)"}
WHICH_RANGE = "which must be 0 (the operator) or 1 (the metric)"
PART_RANGE = "part must be 0 (A+B), 1 (A-B), 2 (S+D) or 3 (S-D)"
PAIR_RANGE = "pair must be 0 (A and B: fills A+B, A-B) or 1 (S and D: fills S+D, S-D)"
MATVEC, PRECND, LRPREC = "dla_call_matvec", "dla_call_precnd", "dla_call_lrprec"


def number(slot):
    """(is a part, the public number of the slot)"""
    return (True, PARTS.index(slot)) if slot in PARTS else (False, "AB".index(slot))


def set_up(ctx, slot, a=None):
    a = MAT[slot] if a is None else a
    part, k = number(slot)
    ctx._chk((ctx.lib.dla_dense_setup_lr if part else ctx.lib.dla_dense_setup)(ctx.h, k, a.shape[0], a.ctypes.data, a.shape[0]))


def fill(ctx, slots=SLOTS):
    """(every accepted set-up binds the thread's dense callbacks to ctx)"""
    for s in slots:
        set_up(ctx, s)


@pytest.fixture()
def c():
    """a context of its own with nothing stored, which the thread's dense callbacks act on: only an ACCEPTED set-up binds it, and a
    drop leaves the binding alone"""
    with fresh_context() as ctx:
        set_up(ctx, "A")
        assert ctx.lib.dla_dense_drop(ctx.h, 0) == 0
        yield ctx


def info_status(ctx, slot, out):
    part, k = number(slot)
    return (ctx.lib.dla_dense_lr_info if part else ctx.lib.dla_dense_info)(ctx.h, k, out)


def states(ctx):
    """the product of the operator, the metric and amb first (an info describes the most recent product), then the info of all six
    slots: their bits, or status and message of the refusal"""
    got = {}
    for s in THREE:
        gx, gy = Guarded(ctx, N, M, X), Guarded(ctx, N, M)
        st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(CALL[s]), N, M, gx.ptr, gy.ptr)
        y = gy.body().copy()
        got["product", s] = y.tobytes() if st == 0 else (st, last_error(ctx), y.tobytes())
        gx.free(); gy.free()
    for s in SLOTS:
        out = capi.DenseInfo()
        st = info_status(ctx, s, C.byref(out))
        got["info", s] = bytes(out) if st == 0 else (st, last_error(ctx))
    return got


def assert_refused(ctx, st, text, before):
    msg = last_error(ctx)
    assert (st, msg) == (capi.ERR_ARG, text), (st, msg, text)
    assert states(ctx) == before, "a refused call changed a slot"


def refused_callback(ctx, trampoline, name, n, fac=None, blocks=2):
    """(status, message) of a callback through its trampoline on blocks of n x M; a refused callback has written nothing"""
    g = [Guarded(ctx, n, M, np.ones((n, M))) for _ in range(blocks // 2)] + [Guarded(ctx, n, M) for _ in range(blocks // 2)]
    args = (n, M) + (() if fac is None else (fac,)) + tuple(b.ptr for b in g)
    st = getattr(ctx.lib, trampoline)(ctx.h, capi.fn_address(name), *args)
    msg = last_error(ctx)
    for b in g[:blocks // 2]:
        b.assert_unchanged()
    assert all(np.all(b.body() == SENT) for b in g[blocks // 2:]), name + ": a refused callback wrote"
    for b in g:
        b.free()
    return st, msg


# ------------------------------------------------------------------------------------------------------------------ set-ups
@pytest.fixture(params=["nothing stored", "all six stored"])
def stored(request, c):
    if request.param == "all six stored":
        fill(c)
    return c


@pytest.mark.parametrize("entry", ["dla_dense_setup", "dla_dense_setup_dev", "dla_dense_setup_lr", "dla_dense_setup_lr_dev"])
def test_refused_set_ups_of_one_matrix(stored, entry):
    c = stored
    range_rule, numbers, bad_numbers = (PART_RANGE, (0, 1, 2, 3), (4, -1)) if "_lr" in entry else (WHICH_RANGE, (0, 1), (2, -1))
    before = states(c)
    other = np.asfortranarray(np.random.default_rng(12).standard_normal((N, N)))
    dev = c.panel(other)
    ptr = dev.ptr if entry.endswith("_dev") else other.ctypes.data
    f = getattr(c.lib, entry)
    for k in numbers:
        assert_refused(c, f(c.h, k, N, None, N), entry + ": the matrix is a null pointer", before)
        assert_refused(c, f(c.h, k, 0, ptr, N), entry + ": n must be positive", before)
        assert_refused(c, f(c.h, k, -3, ptr, N), entry + ": n must be positive", before)
        assert_refused(c, f(c.h, k, N, ptr, N - 1), entry + ": lda = 7 is below n = 8", before)
        assert_refused(c, f(c.h, k, 0, None, -1), entry + ": the matrix is a null pointer", before)       # (the order of the checks)
        assert_refused(c, f(c.h, k, 0, ptr, -1), entry + ": n must be positive", before)
    for k in bad_numbers:
        assert_refused(c, f(c.h, k, N, ptr, N), entry + ": " + range_rule, before)
        assert_refused(c, f(c.h, k, 0, None, 0), entry + ": " + range_rule, before)                        # (asked before the array is looked at)
    dev.free()


@pytest.mark.parametrize("entry", ["dla_dense_setup_lr_pair", "dla_dense_setup_lr_pair_dev"])
def test_refused_set_ups_of_a_pair(stored, entry):
    c = stored
    before = states(c)
    rng = np.random.default_rng(13)
    hp, hq = (np.asfortranarray(rng.standard_normal((N, N))) for _ in range(2))
    dp, dq = c.panel(hp), c.panel(hq)
    p, q = (dp.ptr, dq.ptr) if entry.endswith("_dev") else (hp.ctypes.data, hq.ctypes.data)
    f = getattr(c.lib, entry)
    for pair in (0, 1):
        assert_refused(c, f(c.h, pair, N, None, N, q, N), entry + ": the first matrix (p) is a null pointer", before)
        assert_refused(c, f(c.h, pair, N, p, N, None, N), entry + ": the second matrix (q) is a null pointer", before)
        assert_refused(c, f(c.h, pair, N, None, N, None, N), entry + ": the first matrix (p) is a null pointer", before)
        assert_refused(c, f(c.h, pair, 0, p, N, q, N), entry + ": n must be positive", before)
        assert_refused(c, f(c.h, pair, -3, p, N, q, N), entry + ": n must be positive", before)
        assert_refused(c, f(c.h, pair, N, p, N - 1, q, N + 2), entry + ": ldp = 7 is below n = 8", before)
        assert_refused(c, f(c.h, pair, N, p, N + 2, q, N - 1), entry + ": ldq = 7 is below n = 8", before)
        assert_refused(c, f(c.h, pair, N, p, N - 1, q, N - 2), entry + ": ldp = 7 is below n = 8", before)  # (p is looked at first)
        assert_refused(c, f(c.h, pair, N, p, N - 1, None, N), entry + ": ldp = 7 is below n = 8", before)
    for pair in (2, -1):
        assert_refused(c, f(c.h, pair, N, p, N, q, N), entry + ": " + PAIR_RANGE, before)
        assert_refused(c, f(c.h, pair, 0, None, 0, None, 0), entry + ": " + PAIR_RANGE, before)
    dp.free(); dq.free()


# ------------------------------------------------------------------------------------------------------------------ info and drop
def test_info_and_drop_of_a_number_out_of_range_and_a_null_out(stored):
    c = stored
    before = states(c)
    out = capi.DenseInfo()
    for bad in (2, -1):
        assert_refused(c, c.lib.dla_dense_info(c.h, bad, C.byref(out)), "dla_dense_info: " + WHICH_RANGE, before)
        assert_refused(c, c.lib.dla_dense_info(c.h, bad, None), "dla_dense_info: " + WHICH_RANGE, before)
        assert_refused(c, c.lib.dla_dense_drop(c.h, bad), "dla_dense_drop: " + WHICH_RANGE, before)
    for bad in (4, -1):
        assert_refused(c, c.lib.dla_dense_lr_info(c.h, bad, C.byref(out)), "dla_dense_lr_info: " + PART_RANGE, before)
        assert_refused(c, c.lib.dla_dense_lr_info(c.h, bad, None), "dla_dense_lr_info: " + PART_RANGE, before)
    for which in (0, 1):
        assert_refused(c, c.lib.dla_dense_info(c.h, which, None), "dla_dense_info: out is a null pointer", before)
    for part in range(4):
        assert_refused(c, c.lib.dla_dense_lr_info(c.h, part, None), "dla_dense_lr_info: out is a null pointer", before)


def test_info_of_an_empty_slot(c):
    out = capi.DenseInfo()
    for stored in ((), ("B", "apb", "spd"), ("A", "amb", "smd")):
        fill(c, stored)
        before = states(c)
        for s in SLOTS:
            if s not in stored:
                entry = "dla_dense_lr_info" if s in PARTS else "dla_dense_info"
                assert_refused(c, info_status(c, s, C.byref(out)), f"{entry}: no {NOUN[s]} has been set up", before)
                assert before["info", s] == (capi.ERR_ARG, f"{entry}: no {NOUN[s]} has been set up")
        assert c.lib.dla_dense_drop(c.h, 0) == 0 and c.lib.dla_dense_drop(c.h, 1) == 0 and c.lib.dla_dense_drop_lr(c.h) == 0
    assert c.lib.dla_dense_drop(c.h, 0) == 0 and c.lib.dla_dense_drop(c.h, 1) == 0 and c.lib.dla_dense_drop_lr(c.h) == 0   # (nothing to drop: no error)


# ------------------------------------------------------------------------------------------------------------------ the callbacks
def empty(slot, callback):
    hint = "dla_dense_setup_lr" if slot in PARTS else "dla_dense_setup"
    return f"dla_{callback} failed: {callback}: no {NOUN[slot]} has been set up ({hint})"


def other_n(slot, callback):
    return f"dla_{callback} failed: {callback}: n = 9 differs from the 8 rows of the {NOUN[slot]}"


def test_callbacks_on_empty_slots(c):
    before = states(c)
    for s in SLOTS:
        name = CALL[s]
        assert refused_callback(c, MATVEC, name, N) == (capi.ERR_ARG, empty(s, name[4:])), name
        if s in THREE:
            assert before["product", s] == (capi.ERR_ARG, empty(s, name[4:]), np.full((N, M), SENT, order="F").tobytes())
    for name in ("dense_precnd", "dense_precnd_pencil"):
        assert refused_callback(c, PRECND, "dla_" + name, N, 0.3) == (capi.ERR_ARG, empty("A", name)), name
    for name in ("dense_lrprec1", "dense_lrprec2"):
        assert refused_callback(c, LRPREC, "dla_" + name, N, 0.3, 4) == (capi.ERR_ARG, empty("apb", name)), name
    assert states(c) == before


def test_the_pencil_preconditioner_without_a_metric_and_with_one_of_another_size(c):
    pencil = "dla_dense_precnd_pencil failed: dense_precnd_pencil: "
    set_up(c, "B")
    before = states(c)
    assert refused_callback(c, PRECND, "dla_dense_precnd_pencil", N, 0.3) == (capi.ERR_ARG, empty("A", "dense_precnd_pencil"))
    assert states(c) == before
    c._chk(c.lib.dla_dense_drop(c.h, 1))
    set_up(c, "A")
    before = states(c)
    assert refused_callback(c, PRECND, "dla_dense_precnd_pencil", N, 0.3) == (
        capi.ERR_ARG, pencil + "no dense metric has been set up (dla_dense_setup with which = 1)")
    assert states(c) == before
    set_up(c, "B", np.asfortranarray(np.random.default_rng(14).standard_normal((5, 5))))
    before = states(c)
    assert before["product", "B"][:2] == (capi.ERR_ARG, "dla_dense_bvec failed: dense_bvec: n = 8 differs from the 5 rows of the dense metric")
    assert refused_callback(c, PRECND, "dla_dense_precnd_pencil", N, 0.3) == (capi.ERR_ARG, pencil + "the operator has 8 rows and the metric 5")
    # (the operator's own n is asked about first)
    assert refused_callback(c, PRECND, "dla_dense_precnd_pencil", 5, 0.3) == (
        capi.ERR_ARG, pencil + "n = 5 differs from the 8 rows of the dense operator")
    assert states(c) == before


def test_the_lr_preconditioners_need_apb_amb_and_spd_and_not_smd(c):
    for have in ((), ("smd",), ("smd", "apb"), ("smd", "apb", "amb"), ("apb", "spd"), ("amb", "spd", "smd")):
        fill(c, have)
        before = states(c)
        missing = next(p for p in ("apb", "amb", "spd") if p not in have)
        for name in ("dense_lrprec1", "dense_lrprec2"):
            assert refused_callback(c, LRPREC, "dla_" + name, N, 0.3, 4) == (capi.ERR_ARG, empty(missing, name)), (have, name)
        assert states(c) == before
        c._chk(c.lib.dla_dense_drop_lr(c.h))
    # parts of unequal n: the first that differs from the call's n is named
    fill(c, ("apb", "spd"))
    set_up(c, "amb", np.asfortranarray(np.random.default_rng(15).standard_normal((9, 9))))
    for name in ("dense_lrprec1", "dense_lrprec2"):
        assert refused_callback(c, LRPREC, "dla_" + name, N, 0.3, 4) == (
            capi.ERR_ARG, f"dla_{name} failed: {name}: n = 8 differs from the 9 rows of the dense part amb (A-B)")
        assert refused_callback(c, LRPREC, "dla_" + name, N + 1, 0.3, 4) == (capi.ERR_ARG, other_n("apb", name))
    # ... and without S-D all three are there: accepted
    set_up(c, "amb")
    g = [Guarded(c, N, M, X), Guarded(c, N, M, X), Guarded(c, N, M), Guarded(c, N, M)]
    assert c.lib.dla_call_lrprec(c.h, capi.fn_address("dla_dense_lrprec1"), N, M, 0.3, *(b.ptr for b in g)) == 0
    for b in g:
        b.free()


def test_callbacks_with_one_row_more(c):
    fill(c)
    before = states(c)
    for s in SLOTS:
        name = CALL[s]
        assert refused_callback(c, MATVEC, name, N + 1) == (capi.ERR_ARG, other_n(s, name[4:])), name
    for name in ("dense_precnd", "dense_precnd_pencil"):
        assert refused_callback(c, PRECND, "dla_" + name, N + 1, 0.3) == (capi.ERR_ARG, other_n("A", name)), name
    for name in ("dense_lrprec1", "dense_lrprec2"):
        assert refused_callback(c, LRPREC, "dla_" + name, N + 1, 0.3, 4) == (capi.ERR_ARG, other_n("apb", name)), name
    assert states(c) == before
    assert all(isinstance(before["product", s], bytes) for s in THREE) and all(isinstance(before["info", s], bytes) for s in SLOTS)
    assert len({before["product", s] for s in THREE}) == 3
