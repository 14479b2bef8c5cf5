"""GPU: the four dense parts of a linear-response pencil (include/diaglib_amd.h, dla_dense_setup_lr): the products dla_dense_apbmul /
ambmul / spdmul / smdmul on the kernels of the dense operator, the pair set-ups dla_dense_setup_lr_pair / _pair_dev
(dense_pack_pair_kernel), the preconditioners dla_dense_lrprec1 / 2 (lr_precnd_kernel on the stored dense diagonals), the slots'
independence and refusals, and whole caslr_eff_driver / caslr_driver solves of the reference harness' dense problem in device mode
against the golden fixtures of the unmodified reference.

Oracles: the dense operator slot for the bits of the products (the same kernels and plan on another instance of the storage), numpy
for exact integer products and for the preconditioner (lrprec_numpy: the same expression in the same order of operations),
dla_dense_setup_lr of numpy's p + q and p - q for the pair set-ups.  Outputs sit between sentinel columns and inputs between NaN
columns: nothing outside the n x m result is written, the input is unchanged."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi
from spmm_lr_cases import PARTS, lrprec_numpy
from spmm_slots import info as sparse_info, product as sparse_product, same_bits
from test_operators_gpu import Guarded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.25e77
PART = capi.SPMM_LR_PARTS
MUL = {p: f"dla_dense_{p}mul" for p in PARTS}
SIZES = [1, 15, 17, 65, 130]
WIDTHS = [1, 3, 16, 17, 49]


@pytest.fixture()
def dev(ctx):
    """device callbacks on; the session's context is handed back without dense matrices and without sparse parts or metric"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.dense_drop_lr()
    yield ctx
    ctx.dense_drop_lr()
    ctx.dense_drop(False)
    ctx.dense_drop(True)
    ctx.spmm_drop_lr()
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)


def held(a, lda):
    """a in the leading n rows of an lda x n column-major array whose other rows are NaN"""
    n = a.shape[0]
    h = np.full((lda, n), np.nan, order="F")
    h[:n, :] = a
    return h


def setup_host(ctx, part, a, lda):
    h = held(a, lda)
    ctx._chk(ctx.lib.dla_dense_setup_lr(ctx.h, PART[part], a.shape[0], h.ctypes.data, lda))


def setup_device(ctx, part, a, lda):
    """... from device memory; the array is overwritten and freed before anything is multiplied"""
    p = ctx.panel(held(a, lda))
    ctx._chk(ctx.lib.dla_dense_setup_lr_dev(ctx.h, PART[part], a.shape[0], p.ptr, lda))
    p.zero()
    ctx.sync()
    p.free()


def product(ctx, name, x):
    """one product of the named callback on x between NaN columns, the result between sentinel columns"""
    n, m = x.shape
    xin = np.full((n, m + 2), np.nan, order="F")
    xin[:, 1:m + 1] = x
    px, py = ctx.panel(xin), ctx.panel(np.full((n, m + 2), SENTINEL, order="F"))
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, px.col(1, m).ptr, py.col(1, m).ptr))
    out, xafter = py.download(), px.download()
    px.free(); py.free()
    assert np.all(out[:, 0] == SENTINEL) and np.all(out[:, m + 1] == SENTINEL), "the columns beside the result were written"
    assert np.array_equal(xafter[:, 1:m + 1], x) and np.all(np.isnan(xafter[:, [0, m + 1]])), "the input was changed"
    return out[:, 1:m + 1]


def last_error(ctx):
    return ctx.lib.dla_last_error(ctx.h).decode()


# ------------------------------------------------------------------ 1. the bits of the operator slot
@pytest.mark.parametrize("n", SIZES)
def test_part_products_are_the_bits_of_the_dense_operator_slot(dev, n):
    """n = 130 with m <= 3 is the smallest split pass (k_chunks = 2), m = 49 the smallest second pass"""
    rng = np.random.default_rng(6000 + n)
    a = rng.standard_normal((n, n))                                       # not symmetric
    xs = {m: rng.standard_normal((n, m)) for m in WIDTHS}
    dev.dense_setup(a)
    want, chunks = {}, {}
    for m in WIDTHS:
        want[m] = product(dev, "dla_dense_matvec", xs[m])
        chunks[m] = dev.dense_info()
    if n == 130:
        assert chunks[1]["k_chunks"] == 2 and chunks[3]["k_chunks"] == 2, chunks
    for k, part in enumerate(PARTS):
        (setup_device if k % 2 else setup_host)(dev, part, a, n + 3 * (k // 2))
        info = dev.dense_lr_info(part)
        assert info["n"] == n and info["n_pad"] == -(-n // 16) * 16 and info["device_bytes"] == 8 * info["n_pad"] ** 2 + 8 * n
        for m in WIDTHS:
            got = product(dev, MUL[part], xs[m])
            assert same_bits(got, want[m]), (n, m, part)
            assert dev.dense_lr_info(part) == chunks[m], (n, m, part)     # the first pass of that part's most recent product
    assert dev.dense_info() == chunks[WIDTHS[-1]]


def test_one_launch_per_pass_booked_as_a_dense_pass(dev):
    n, m = 130, 3
    rng = np.random.default_rng(7)
    setup_host(dev, "smd", rng.standard_normal((n, n)), n)
    x, y = dev.panel(rng.standard_normal((n, m))), dev.panel(n, m)
    dev.reset_stats()
    dev._chk(dev.lib.dla_call_matvec(dev.h, capi.fn_address("dla_dense_smdmul"), n, m, x.ptr, y.ptr))
    dev.sync()
    ks = {k: v["launches"] for k, v in dev.kernel_stats().items() if v["launches"]}
    assert ks == {"dense_mfma_kernel<1>": 1, "dense_combine_kernel": 1}, ks
    mv = dev.stats()["matvec"]
    assert mv["alg_bytes"] == 8.0 * n * n + 16.0 * n * m and mv["flops"] == 2.0 * n * n * m and mv["launches"] == 2, mv
    assert dev.dense_lr_info("smd")["workspace_bytes"] == 8 * 2 * n * m
    x.free(); y.free()


# ------------------------------------------------------------------ 2. no symmetry assumed
def test_a_non_symmetric_s_plus_d_and_s_minus_d(dev):
    """small integers: every order of summation is exact, so (S + D) x and (S - D) x equal numpy's bit for bit -- and each other's
    transposed product does not"""
    n, m = 37, 5
    rng = np.random.default_rng(37)
    s = rng.integers(-4, 5, (n, n)).astype(np.float64)
    s = s + s.T
    d = np.triu(rng.integers(1, 5, (n, n)), 1).astype(np.float64)
    d = d - d.T
    x = rng.integers(-8, 9, (n, m)).astype(np.float64)
    setup_host(dev, "spd", s + d, n + 1)
    setup_device(dev, "smd", s - d, n)
    got_p, got_m = product(dev, "dla_dense_spdmul", x), product(dev, "dla_dense_smdmul", x)
    assert np.array_equal(got_p, (s + d) @ x) and np.array_equal(got_m, (s - d) @ x)
    assert not np.array_equal(got_p, (s - d) @ x)


# ------------------------------------------------------------------ 3. the pair set-ups
def _state(ctx, part, x):
    """(info, product bits); the product first: info describes the most recent product"""
    y = product(ctx, MUL[part], x)
    return ctx.dense_lr_info(part), y


@pytest.mark.parametrize("n", [17, 130])
@pytest.mark.parametrize("pair", [0, 1], ids=["ab", "sd"])
def test_pair_set_ups_store_what_setup_lr_stores_for_the_sum_and_the_difference(dev, n, pair):
    rng = np.random.default_rng(700 + n + pair)
    p, q = rng.standard_normal((n, n)), rng.standard_normal((n, n)) * 1e-3      # (p + q rounds: the sum is not exact)
    q[0, 0], q[n - 1, 0] = p[0, 0], -p[n - 1, 0]                                 # exact zeros in the difference and in the sum
    x = rng.standard_normal((n, 3))
    plus, minus = PARTS[2 * pair], PARTS[2 * pair + 1]
    setup_host(dev, plus, np.asfortranarray(p + q), n)
    setup_host(dev, minus, np.asfortranarray(p - q), n)
    want = {part: _state(dev, part, x) for part in (plus, minus)}
    assert not same_bits(want[plus][1], want[minus][1])
    ldp, ldq = n + 3, n + 5
    hp, hq = held(p, ldp), held(q, ldq)

    def check(tag):
        for part in (plus, minus):
            got = _state(dev, part, x)
            assert got[0] == want[part][0] and same_bits(got[1], want[part][1]), (tag, part)

    dev.dense_drop_lr()
    dev._chk(dev.lib.dla_dense_setup_lr_pair(dev.h, pair, n, hp.ctypes.data, ldp, hq.ctypes.data, ldq))
    check("host")
    assert np.array_equal(hp[:n], p) and np.array_equal(hq[:n], q), "the sources are only read"
    dev.dense_drop_lr()
    dp, dq = dev.panel(hp), dev.panel(hq)
    dev._chk(dev.lib.dla_dense_setup_lr_pair_dev(dev.h, pair, n, dp.ptr, ldp, dq.ptr, ldq))
    assert same_bits(dp.download()[:n], p) and same_bits(dq.download()[:n], q), "the sources are only read"
    dp.zero(); dq.zero()
    dev.sync()
    dp.free(); dq.free()
    check("device")
    # over a larger matrix in both slots (the blocks only grow; the padding of the smaller copy must be written all the same)
    big = rng.standard_normal((n + 40, n + 40))
    setup_host(dev, plus, big, n + 40)
    setup_device(dev, minus, big, n + 40)
    dev.dense_setup_lr_pair(pair, p, q)                                          # the wrapper, NumPy arrays (C-ordered)
    check("wrapper")
    for other in PARTS:
        if other not in (plus, minus):
            with pytest.raises(capi.DlaError, match="dla_dense_lr_info"):
                dev.dense_lr_info(other)


def test_pair_and_part_set_up_from_column_major_torch_views(dev):
    import torch
    n, ldp, ldq = 17, 20, 24
    rng = np.random.default_rng(5)
    p, q = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    x = rng.standard_normal((n, 3))
    setup_host(dev, "spd", np.asfortranarray(p + q), n)
    setup_host(dev, "smd", np.asfortranarray(p - q), n)
    want = {part: _state(dev, part, x) for part in ("spd", "smd")}
    dev.dense_drop_lr()
    bp, bq = np.zeros((n, ldp)), np.zeros((n, ldq))
    bp[:, :n], bq[:, :n] = p.T, q.T                              # b[k, i] = a(i, k): a(ld, n) column-major
    tp, tq = torch.from_numpy(bp).cuda(), torch.from_numpy(bq).cuda()
    dev.dense_setup_lr_pair("sd", tp.T[:n, :], tq.T[:n, :])
    for part in ("spd", "smd"):
        got = _state(dev, part, x)
        assert got[0] == want[part][0] and same_bits(got[1], want[part][1]), part
    dev.dense_setup_lr("apb", tp.T[:n, :])
    dev.dense_setup(p)
    assert same_bits(product(dev, "dla_dense_apbmul", x), product(dev, "dla_dense_matvec", x))
    for bad in ((tp[:, :n], tq.T[:n, :]), (tp.T[:n, :], q), (tp.T[:n, :], tq.T[:n, :].float()), (p, q[:5, :5])):
        with pytest.raises(ValueError, match="dense_setup_lr_pair"):
            dev.dense_setup_lr_pair("sd", *bad)
    with pytest.raises(ValueError, match="dense_setup_lr_pair"):
        dev.dense_setup_lr_pair("ba", p, q)
    with pytest.raises(ValueError, match="dense_setup_lr"):
        dev.dense_setup_lr("bpa", p)
    for part in ("spd", "smd"):
        assert same_bits(product(dev, MUL[part], x), want[part][1])


# ------------------------------------------------------------------ 4. independence
def _banded(n, k, scale):
    i = np.arange(n, dtype=np.float64)
    return sp.diags([scale * np.cos(i[:-k] + k), 2.0 + scale + i / 50.0, scale * np.sin(i[:-k] + k)], [-k, 0, k]).tocsr()


def test_dense_parts_and_all_other_slots_keep_their_bits_while_the_others_change(dev):
    """a sparse A, the four sparse parts, a dense A and a dense B beside the four dense parts: setting, replacing and dropping a dense
    part leaves every other slot's info and product bits alone, and the reverse"""
    n, m = 130, 5
    rng = np.random.default_rng(9)
    x = np.asfortranarray(rng.standard_normal((n, m)))
    dense = {name: rng.standard_normal((n, n)) for name in ("A", "B") + PARTS}
    sparse = {name: _banded(n, 1 + k, 0.1 * (1 + k)) for k, name in enumerate(("A",) + PARTS)}

    def set_sparse(name, mat):
        dev.spmm_setup(mat) if name == "A" else dev.spmm_setup_lr(name, mat)

    def set_dense(name, a, device=False):
        if name in PARTS:
            (setup_device if device else setup_host)(dev, name, a, a.shape[0] + (2 if device else 0))
        else:
            dev.dense_setup(a, metric=name == "B")

    def state(kind, name):
        if kind == "sparse":
            return sparse_info(dev, name), sparse_product(dev, name, x)
        if name in PARTS:
            return _state(dev, name, x)
        y = product(dev, "dla_dense_bvec" if name == "B" else "dla_dense_matvec", x)
        return dev.dense_info(name == "B"), y

    slots = [("sparse", s) for s in sparse] + [("dense", d) for d in dense]
    for name, mat in sparse.items():
        set_sparse(name, mat)
    for name, a in dense.items():
        set_dense(name, a)
    before = {slot: state(*slot) for slot in slots}
    assert len({v[1].tobytes() for v in before.values()}) == len(slots)

    def unchanged(but=()):
        for slot in slots:
            if slot not in but:
                got = state(*slot)
                assert got[0] == before[slot][0] and same_bits(got[1], before[slot][1]), f"slot {slot} changed"

    # every dense part in turn: replaced by a matrix of another size (from device memory), put back, dropped with the other parts
    for part in PARTS:
        setup_device(dev, part, rng.standard_normal((63, 63)), 65)
        assert dev.dense_lr_info(part)["n"] == 63
        unchanged(but=[("dense", part)])
        set_dense(part, dense[part], device=True)
        unchanged()
    dev.dense_drop_lr()
    unchanged(but=[("dense", p) for p in PARTS])
    for part in PARTS:
        with pytest.raises(capi.DlaError, match="dla_dense_lr_info.*" + part):
            dev.dense_lr_info(part)
    dev.dense_drop_lr()                                        # (nothing to drop: no error)
    dev.dense_setup_lr_pair("ab", dense["apb"], dense["amb"])  # a pair fills its two slots and no other
    unchanged(but=[("dense", p) for p in PARTS])
    for part in ("spd", "smd"):
        with pytest.raises(capi.DlaError, match="dla_dense_lr_info.*" + part):
            dev.dense_lr_info(part)
    for part in PARTS:
        set_dense(part, dense[part])
    unchanged()
    # the reverse: every other slot replaced, put back and dropped in turn
    for name in ("A", "B"):
        set_dense(name, rng.standard_normal((63, 63)))
        unchanged(but=[("dense", name)])
        dev.dense_drop(name == "B")
        unchanged(but=[("dense", name)])
        set_dense(name, dense[name])
        unchanged()
    for name in sparse:
        set_sparse(name, _banded(n, 3, 0.7))
        unchanged(but=[("sparse", name)])
        set_sparse(name, sparse[name])
        unchanged()
    dev.spmm_drop_lr()
    unchanged(but=[("sparse", p) for p in PARTS])


# ------------------------------------------------------------------ 5. refusals
def test_refused_set_ups_replace_nothing_and_callbacks_name_themselves_and_the_part(dev):
    n, m = 65, 3
    rng = np.random.default_rng(10)
    mats = {part: rng.standard_normal((n, n)) for part in PARTS}
    x = rng.standard_normal((n, m))
    px, pxm = dev.panel(x), dev.panel(x)
    py, pym = (dev.panel(np.full((n + 1, m), SENTINEL, order="F")) for _ in range(2))

    def refused(call, *words):
        st = call()
        assert st == capi.ERR_ARG, st
        assert all(w in last_error(dev) for w in words), (last_error(dev), words)
        assert np.all(py.download() == SENTINEL) and np.all(pym.download() == SENTINEL), "a refused call wrote"

    mv = lambda name, rows=n: dev.lib.dla_call_matvec(dev.h, capi.fn_address(name), rows, m, px.ptr, py.ptr)
    pc = lambda name, rows=n: dev.lib.dla_call_lrprec(dev.h, capi.fn_address(name), rows, m, 0.3, px.ptr, pxm.ptr, py.ptr, pym.ptr)
    # nothing is stored
    for part in PARTS:
        refused(lambda: mv(MUL[part]), MUL[part], part)
        refused(lambda: dev.lib.dla_dense_lr_info(dev.h, PART[part], C.byref(capi.DenseInfo())), "dla_dense_lr_info", part)
    # a preconditioner needs A+B, A-B and S+D -- and not S-D
    setup_host(dev, "smd", mats["smd"], n)
    for needs in ("apb", "amb", "spd"):
        for name in ("dla_dense_lrprec1", "dla_dense_lrprec2"):
            refused(lambda: pc(name), name, needs)
        setup_host(dev, needs, mats[needs], n)
    dev.dense_drop_lr()
    for part in ("apb", "amb", "spd"):
        setup_device(dev, part, mats[part], n + 1)
    guarded = [Guarded(dev, n, m, x), Guarded(dev, n, m, x), Guarded(dev, n, m), Guarded(dev, n, m)]
    dev._chk(dev.lib.dla_call_lrprec(dev.h, capi.fn_address("dla_dense_lrprec1"), n, m, 0.3, *(g.ptr for g in guarded)))
    assert np.all(np.isfinite(guarded[2].body())) and np.all(np.isfinite(guarded[3].body()))      # accepted without S-D
    for g in guarded:
        g.free()
    refused(lambda: mv("dla_dense_smdmul"), "dla_dense_smdmul", "smd")
    setup_host(dev, "smd", mats["smd"], n)
    before = {part: _state(dev, part, x) for part in PARTS}

    def unchanged():
        for part in PARTS:
            got = _state(dev, part, x)
            assert got[0] == before[part][0] and same_bits(got[1], before[part][1]), part

    # refused set-ups of a part, host and device entry: lda < n, a null pointer, n <= 0, a part outside 0 .. 3
    other = np.asfortranarray(rng.standard_normal((n, n)))
    dother, dother2 = dev.panel(other), dev.panel(other)
    for entry, ptr in (("dla_dense_setup_lr", other.ctypes.data), ("dla_dense_setup_lr_dev", dother.ptr)):
        f = getattr(dev.lib, entry)
        for part in range(4):
            refused(lambda: f(dev.h, part, n, ptr, n - 1), entry + ":", "lda")
            refused(lambda: f(dev.h, part, n, None, n), entry + ":", "null")
            refused(lambda: f(dev.h, part, 0, ptr, n), entry + ":", "n must be positive")
        for bad in (4, -1):
            refused(lambda: f(dev.h, bad, n, ptr, n), entry + ":", "part")
        unchanged()
    for bad in (4, -1):
        refused(lambda: dev.lib.dla_dense_lr_info(dev.h, bad, C.byref(capi.DenseInfo())), "dla_dense_lr_info:", "part")
    # ... and of a pair: either array null, n <= 0, ldp < n, ldq < n, a pair outside 0 and 1 -- both slots stay
    for entry, p, q in (("dla_dense_setup_lr_pair", other.ctypes.data, other.ctypes.data), ("dla_dense_setup_lr_pair_dev", dother.ptr, dother2.ptr)):
        f = getattr(dev.lib, entry)
        for pair in (0, 1):
            refused(lambda: f(dev.h, pair, n, None, n, q, n), entry + ":", "null")
            refused(lambda: f(dev.h, pair, n, p, n, None, n), entry + ":", "null")
            refused(lambda: f(dev.h, pair, 0, p, n, q, n), entry + ":", "n must be positive")
            refused(lambda: f(dev.h, pair, n, p, n - 1, q, n + 2), entry + ":", "ldp")
            refused(lambda: f(dev.h, pair, n, p, n + 2, q, n - 1), entry + ":", "ldq")
        for bad in (2, -1):
            refused(lambda: f(dev.h, bad, n, p, n, q, n), entry + ":", "pair")
        unchanged()
    # the entries of the operator and the metric refuse the part numbers as before
    refused(lambda: dev.lib.dla_dense_setup(dev.h, 2, n, other.ctypes.data, n), "dla_dense_setup:", "which")
    unchanged()
    # another n
    for part in PARTS:
        refused(lambda: mv(MUL[part], n + 1), MUL[part], part, str(n + 1), str(n))
    for name in ("dla_dense_lrprec1", "dla_dense_lrprec2"):
        refused(lambda: pc(name, n + 1), name, str(n + 1), str(n))
    # parts of unequal n
    setup_host(dev, "amb", rng.standard_normal((63, 63)), 63)
    for name in ("dla_dense_lrprec1", "dla_dense_lrprec2"):
        refused(lambda: pc(name), name, "amb", "63", str(n))
    for p_ in (px, pxm, py, pym, dother, dother2):
        p_.free()


# ------------------------------------------------------------------ 6. the preconditioners
def _lrprec(ctx, variant, n, m, fac, xp, xm):
    g = [Guarded(ctx, n, m, xp), Guarded(ctx, n, m, xm), Guarded(ctx, n, m), Guarded(ctx, n, m)]
    ctx._chk(ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(f"dla_dense_lrprec{variant}"), n, m, fac, *(b.ptr for b in g)))
    yp, ym = g[2].body().copy(), g[3].body().copy()
    g[0].assert_unchanged(); g[1].assert_unchanged()
    for b in g:
        b.free()
    return yp, ym


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("n", [1, 130])
def test_lrprec_against_numpy_bit_for_bit(dev, n, m):
    """lr_precnd_kernel on the stored dense diagonals against lrprec_numpy (tests/spmm_lr_cases.py), both variants, fac of both signs.
    The diagonals' ranges keep both denominators away from zero for fac = 0.3 and -1.7 (tests/test_spmm_lr_gpu.py, _diagonal_parts:
    aa in [2, 3], sg in [0.1, 0.4]); the off-diagonal elements are random and must not reach the result; S - D is not stored.

    The issue also asks for one n above a single stride trip of lr_precnd_kernel.  One trip covers 8 x 256 rows per compute unit,
    524 288 rows on 256 of them, and a dense part of that many rows is 8 n^2 = 2.2 TB: no such part can be stored, so that case
    cannot be run on the dense diagonals.  The kernel's second trip is held on the same kernel by
    tests/test_spmm_lr_gpu.py::test_lrprec_takes_a_second_stride_trip."""
    rng = np.random.default_rng(800 + n + m)
    d = {"apb": rng.uniform(2.5, 3.5, n), "amb": rng.uniform(1.5, 2.5, n), "spd": rng.uniform(0.1, 0.4, n)}
    for k, (part, diag) in enumerate(d.items()):
        a = rng.standard_normal((n, n))
        np.fill_diagonal(a, diag)
        (setup_device if k == 1 else setup_host)(dev, part, a, n + k)
    xp, xm = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
    dev.reset_stats()
    launches = dev.stats()["precnd"]["launches"]
    for variant in (1, 2):
        for fac in (0.3, -1.7):
            yp, ym = _lrprec(dev, variant, n, m, fac, xp, xm)
            wp, wm = lrprec_numpy(variant, fac, d["apb"], d["amb"], d["spd"], xp, xm)
            assert same_bits(yp, wp), f"lrprec{variant} fac={fac}: yp differs in {int((yp != wp).sum())} places, max {np.abs(yp - wp).max():.3e}"
            assert same_bits(ym, wm), f"lrprec{variant} fac={fac}: ym differs in {int((ym != wm).sum())} places, max {np.abs(ym - wm).max():.3e}"
    assert dev.stats()["precnd"]["launches"] == launches + 4
    # booked as spmm_lrprec books its launches: under no kernel name, 32 n m + 24 n bytes and 8 n m flops each
    pc = dev.stats()["precnd"]
    assert (pc["launches"], pc["alg_bytes"], pc["flops"]) == (4, 4 * (32.0 * n * m + 24.0 * n), 4 * 8.0 * n * m), pc
    assert not any(v["launches"] for v in dev.kernel_stats().values()), dev.kernel_stats()


def test_lrprec_on_the_diagonals_a_pair_set_up_formed(dev):
    """the diagonals of the pair kernel (dense_diag_pair_kernel) are the rounded sums and differences numpy forms"""
    n, m = 130, 5
    rng = np.random.default_rng(81)
    a, b, s, dd = (rng.standard_normal((n, n)) for _ in range(4))
    np.fill_diagonal(a, rng.uniform(2.0, 3.0, n)); np.fill_diagonal(b, rng.uniform(0.1, 0.5, n))
    np.fill_diagonal(s, rng.uniform(0.1, 0.4, n)); np.fill_diagonal(dd, rng.uniform(-1e-3, 1e-3, n))
    pa, pb, ps, pd = (dev.panel(np.asfortranarray(v)) for v in (a, b, s, dd))
    dev._chk(dev.lib.dla_dense_setup_lr_pair_dev(dev.h, 0, n, pa.ptr, n, pb.ptr, n))
    dev._chk(dev.lib.dla_dense_setup_lr_pair_dev(dev.h, 1, n, ps.ptr, n, pd.ptr, n))
    for p_ in (pa, pb, ps, pd):
        p_.free()
    xp, xm = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
    for variant in (1, 2):
        yp, ym = _lrprec(dev, variant, n, m, -1.7, xp, xm)
        wp, wm = lrprec_numpy(variant, -1.7, np.diag(a) + np.diag(b), np.diag(a) - np.diag(b), np.diag(s) + np.diag(dd), xp, xm)
        assert same_bits(yp, wp) and same_bits(ym, wm), variant


# ------------------------------------------------------------------ 7. whole solves on the reference harness' problem
GOLDEN = ["lr_n300_unit", "lr_n300_rand", "lr_n500_rand", "lrt_n300_unit", "lrt_n300_rand"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_lr_fixtures.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_reference_lr_problem_solved_in_device_mode_matches_the_golden_results(dev, oracle, gold, name):
    """The dense parts of orc_lr_setup in HBM, caslr_eff_driver with dla_dense_lrprec2 and caslr_driver with dla_dense_lrprec1.
    Eigenvalues against the unmodified reference's at rtol = 1e-9 (the figure tests/test_fortran_caller_gpu.py holds these fixtures
    to); iterations within max(1, it_ref // 10) (the MFMA product sums in another order than the reference's dgemm, so equality is
    not asked; the host engine in host-callback mode reproduces the counts exactly); run-ahead on and off agree to 1e-10."""
    spec = json.loads(str(gold[name + "_spec"]))
    n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
    trad = spec.get("driver") == "caslr"
    for part, a in zip(PARTS, oracle.lr_setup(n)):
        dev.dense_setup_lr(part, a)
    if spec["guess"] == "unit":
        guess = np.zeros((2 * n, m), order="F")
        guess[np.arange(m), np.arange(m)] = 1.0
    else:
        guess = np.asfortranarray(gold[name + "_guess"])
    fns = [capi.fn_address(MUL[p]) for p in PARTS] + [capi.fn_address("dla_dense_lrprec1" if trad else "dla_dense_lrprec2")]
    solve = dev.caslr_driver if trad else dev.caslr_eff_driver
    it_ref = int(gold[name + "_tr_iters"])
    eigs = []
    for run_ahead in (1, 0):
        dev.set_option(capi.OPT_RUN_AHEAD, run_ahead)
        ev = dev.panel(guess)
        eig, _, ok, info = solve(n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], *fns, ev)
        ev.free()
        print(f"{name} run-ahead {run_ahead}: {info['iters']} iterations (reference {it_ref}), "
              f"max relative eigenvalue error {float(np.abs(eig[:t] / gold[name + '_eig'][:t] - 1.0).max()):.3e}")
        assert ok and bool(gold[name + "_ok"]), (name, run_ahead, info)
        assert np.allclose(eig[:t], gold[name + "_eig"][:t], rtol=1e-9, atol=0), (name, run_ahead, eig[:t], gold[name + "_eig"][:t])
        assert abs(info["iters"] - it_ref) <= max(1, it_ref // 10), (name, run_ahead, info, it_ref)
        eigs.append(eig[:t].copy())
    assert np.allclose(eigs[0], eigs[1], rtol=1e-10, atol=0), (name, eigs)
