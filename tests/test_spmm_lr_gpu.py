"""GPU: the four sparse parts of a linear-response pencil beside the sparse operator and the metric -- dla_spmm_setup_lr_csr,
dla_spmm_setup_lr_csr_dev, dla_spmm_refresh_lr_values_dev, dla_spmm_lr_info, dla_spmm_drop_lr, the products dla_spmm_apbmul /
ambmul / spdmul / smdmul, the preconditioners dla_spmm_lrprec1 / lrprec2 (lr_precnd_kernel) and whole caslr_eff_driver /
caslr_driver solves that stay in HBM.

Oracles: the operator slot for the bits of the products (the same kernels on another instance of the storage), numpy for the
preconditioner (the same expression in the same order of operations: bit for bit -- lr_precnd_kernel is compiled without
contraction and its disassembly has fused operations only inside the expansion of the two divisions, which is correctly rounded),
scipy.linalg.eig of the dense 2n x 2n pencil and the same driver in host-callback mode for the solves."""
import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi
from spmm_cases import csr_from_lengths
from spmm_lr_cases import (MUL, PARTS, dense_roots, lrprec_numpy, positive_definite, random_pencil, solve_device_mode, solve_host_mode,
                           tolerance)
from spmm_slots import CALL, SLOTS, info as _info, product, raw, refresh_status, same_bits, setup, setup_status, to_device, within_scipy_bound
from test_operators_gpu import Guarded, setup_csr, setup_csr_one_shard
from test_spmm_gpu import _banded

pytestmark = pytest.mark.gpu
FMT = capi.SPMM_FORMATS
PART = capi.SPMM_LR_PARTS


@pytest.fixture()
def dev(ctx):
    """device callbacks on; the session's context is handed back without parts and without a metric"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.spmm_drop_lr()
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.spmm_drop_lr()
    ctx.spmm_drop_metric()


def _part(part):
    return part if isinstance(part, str) else ("part", part)


def setup_fmt(ctx, *csr_and_format):
    setup(ctx, "A", *csr_and_format)


def setup_lr(ctx, part, *csr_and_format):
    """one part from raw CSR arrays (unsorted columns, duplicates: scipy would clean them)"""
    setup(ctx, _part(part), *csr_and_format)


# ------------------------------------------------------------------------------------------------------------------ 1. products by bits
def _ragged(n):
    """rows of 1 .. 20 entries, uniform unsorted columns: nothing like a symmetric matrix"""
    rng = np.random.default_rng(n)
    return csr_from_lengths(rng, n, rng.integers(1, 21, n))


def _two_long_rows(n=8300):
    """... and rows of 8200 and 300 entries in the CSR tail.  Segments hold 4096 entries: the row of 300 is one segment, the row of
    8200 = 2 x 4096 + 8 is three (two full ones and a ragged one); a row of 5000 is added so that a row of exactly two is there too"""
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 21, n)
    lens[4100], lens[77], lens[8000] = 8200, 300, 5000
    return csr_from_lengths(rng, n, lens)


_MATRICES = {}


def _matrix(name):
    if name not in _MATRICES:
        _MATRICES[name] = _two_long_rows() if name == "long" else _ragged(int(name))
    return _MATRICES[name]


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("name,m", [("1000", 1), ("1000", 5), ("1000", 13), ("1001", 5), ("long", 3)])
def test_part_products_are_the_bits_of_the_operator_slot(dev, part, fmt, name, m):
    mat = _matrix(name)
    n = len(mat[0]) - 1
    x = np.asfortranarray(np.random.default_rng(m).standard_normal((n, m)))
    setup_fmt(dev, n, *mat, FMT[fmt])
    setup_lr(dev, part, n, *mat, fmt)
    want = dev.spmm_info()
    assert dev.spmm_lr_info(part) == want and want["format"] == fmt
    if name == "long" and fmt == "sell":
        assert (want["long_rows"], want["long_segments"], want["multi_segments"]) == (3, 6, 5), want
    assert same_bits(product(dev, MUL[part], x), product(dev, "dla_spmm_matvec", x))


@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_a_non_symmetric_part(dev, fmt):
    """S + D of the solves' pencil in the spd slot: the product is (S + D) x, not (S + D)^T x = (S - D) x"""
    mats = random_pencil(300)
    n, m = 300, 5
    x = np.asfortranarray(np.random.default_rng(3).standard_normal((n, m)))
    dev.spmm_setup_lr("spd", mats["spd"], fmt=fmt)
    dev.spmm_setup(mats["spd"], fmt=fmt)
    got = product(dev, MUL["spd"], x)
    assert same_bits(got, product(dev, "dla_spmm_matvec", x))
    assert within_scipy_bound(got, mats["spd"], x) and not within_scipy_bound(got, mats["smd"], x)


# ------------------------------------------------------------------------------------------------------------------ 2. independence
def _set(ctx, slot, mat, fmt):
    setup(ctx, slot, len(mat[0]) - 1, *mat, fmt)


def _state(ctx, slot, x):
    return _info(ctx, slot), product(ctx, CALL[slot], x)


def _assert_unchanged(ctx, before, x, but=()):
    for s in SLOTS:
        if s not in but:
            info, y = _state(ctx, s, x)
            assert info == before[s][0] and same_bits(y, before[s][1]), f"slot {s} changed"


def _six(n):
    """six different matrices, formats mixed; the sliced ones have rows in the CSR tail (their own workspaces)"""
    rng = np.random.default_rng(99)
    out = {}
    for k, s in enumerate(SLOTS):
        lens = rng.integers(1, 8 + 3 * k, n)
        if k % 2:
            lens[10 * k], lens[500 + k] = 300 + k, 700
        out[s] = (csr_from_lengths(rng, n, lens), "sell" if k % 2 else "ell")
    return out


def test_the_six_slots_are_independent(dev):
    n, m = 1000, 5
    x = np.asfortranarray(np.random.default_rng(8).standard_normal((n, m)))
    six = _six(n)
    for s in SLOTS:
        _set(dev, s, *six[s])
    before = {s: _state(dev, s, x) for s in SLOTS}
    assert len({before[s][1].tobytes() for s in SLOTS}) == 6
    rng = np.random.default_rng(100)
    for s in SLOTS:                                   # replace one: another matrix, the other format
        mat = csr_from_lengths(rng, n, rng.integers(1, 30, n))
        _set(dev, s, mat, "ell" if six[s][1] == "sell" else "sell")
        _assert_unchanged(dev, before, x, but=(s,))
        after = _state(dev, s, x)
        assert after[0] != before[s][0] and not same_bits(after[1], before[s][1])
        before[s] = after
    dev.spmm_drop_metric()
    _assert_unchanged(dev, before, x, but=("B",))
    with pytest.raises(capi.DlaError, match="no metric"):
        dev.spmm_metric_info()
    _set(dev, "B", *six["B"])
    before["B"] = _state(dev, "B", x)
    dev.spmm_drop_lr()
    _assert_unchanged(dev, before, x, but=PARTS)
    for p in PARTS:
        with pytest.raises(capi.DlaError, match=f"spmm_lr_info.*{p}.*not been set up"):
            dev.spmm_lr_info(p)
    dev.spmm_drop_lr()                                # (nothing to drop: no error)


@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_a_refused_part_setup_replaces_nothing(dev, fmt):
    n, m = 1000, 5
    x = np.asfortranarray(np.random.default_rng(8).standard_normal((n, m)))
    six = _six(n)
    for s in SLOTS:
        _set(dev, s, six[s][0], fmt)
    before = {s: _state(dev, s, x) for s in SLOTS}
    ok, val = np.array([0, 1, 2, 3, 3, 3, 3], np.int64), np.ones(8)
    cols = np.zeros(8, np.int32)
    for part in PARTS:
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr.*" + part + ".*column index out of range"):
            setup_lr(dev, part, 6, ok, np.array([0, 6, 1, 0, 0, 0, 0, 0], np.int32), val, fmt)
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr.*" + part + ".*column index out of range"):
            setup_lr(dev, part, 6, ok, np.array([0, -1, 1, 0, 0, 0, 0, 0], np.int32), val, fmt)
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr.*" + part + ".*row pointers not ascending"):
            setup_lr(dev, part, 6, np.array([0, 1, 2, 1, 3, 3, 3], np.int64), cols, val, fmt)
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr.*" + part + ".*unknown format"):
            setup_lr(dev, part, 6, ok, cols, val, 3)
        for args in ((0, cols.ctypes.data, val.ctypes.data), (ok.ctypes.data, 0, val.ctypes.data), (ok.ctypes.data, cols.ctypes.data, 0)):
            with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr.*" + part + ".*bad arguments"):
                dev._chk(dev.lib.dla_spmm_setup_lr_csr(dev.h, PART[part], 6, *args, FMT[fmt]))
        _assert_unchanged(dev, before, x)
    for bad in (4, -1):
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr: part must be"):
            setup_lr(dev, bad, 6, ok, cols, val, fmt)
        with pytest.raises(capi.DlaError, match="spmm_lr_info: part must be"):
            dev.spmm_lr_info(bad)
    with pytest.raises(ValueError):
        dev.spmm_setup_lr("apb", sp.identity(6, format="csr"), fmt="csr")
    with pytest.raises(ValueError):
        dev.spmm_setup_lr("bpa", sp.identity(6, format="csr"))
    _assert_unchanged(dev, before, x)


# ------------------------------------------------------------------------------------------------------------------ 3. device arrays
def _dev_call(ctx, entry, part, n, arrays, fmt=None):
    """status of one call of a device-array entry; the tensors are poisoned the moment it has returned"""
    if entry == "dla_spmm_setup_lr_csr_dev":
        return setup_status(ctx, _part(part), n, *arrays, fmt, "device")
    return refresh_status(ctx, _part(part), n, *arrays)


def _dev_mat(kind):
    return _matrix("long") if kind == "sell" else _matrix("1001")


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_device_setup_and_refresh_of_a_part(dev, part, fmt):
    """set-up from torch device tensors = the host set-up, field by field and bit by bit; a refresh = a fresh set-up of the new values;
    a refresh with one column changed is refused and the old products stay (sell: rows in the slices and three rows in the tail)"""
    indptr, indices, data = _dev_mat(fmt)
    n, m = len(indptr) - 1, 5
    x = np.asfortranarray(np.random.default_rng(4).standard_normal((n, m)))
    setup_lr(dev, part, n, indptr, indices, data, fmt)
    host = _state(dev, part, x)
    dev.spmm_drop_lr()
    dev._chk(_dev_call(dev, "dla_spmm_setup_lr_csr_dev", part, n, (indptr, indices, data), fmt))
    got = _state(dev, part, x)
    assert got[0] == host[0] and same_bits(got[1], host[1])
    # new values
    data2 = np.ascontiguousarray(data * 1.5 + 0.25)
    dev._chk(_dev_call(dev, "dla_spmm_refresh_lr_values_dev", part, n, (indptr, indices, data2)))
    fresh_from = _state(dev, part, x)
    setup_lr(dev, part, n, indptr, indices, data2, fmt)
    fresh = _state(dev, part, x)
    assert fresh_from[0] == fresh[0] and same_bits(fresh_from[1], fresh[1]) and not same_bits(fresh[1], host[1])
    # one column changed (in a short row; sell: and in the second segment of the longest tail row)
    spots = [int(indptr[5])] + ([int(indptr[4100]) + 5000] if fmt == "sell" else [])
    for at in spots:
        other = indices.copy()
        other[at] = (other[at] + 1) % n
        st = _dev_call(dev, "dla_spmm_refresh_lr_values_dev", part, n, (indptr, other, data))
        msg = dev.lib.dla_last_error(dev.h).decode()
        assert st == capi.ERR_ARG and "spmm_refresh_lr_values_dev" in msg and part in msg and "columns are not the stored pattern" in msg, (st, msg)
        after = _state(dev, part, x)
        assert after[0] == fresh[0] and same_bits(after[1], fresh[1])
    # the wrappers (torch tensors of any integer width)
    import torch
    dev.spmm_setup_lr_device(part, torch.from_numpy(indptr.astype(np.int32)), torch.from_numpy(indices.astype(np.int64)), torch.from_numpy(data), fmt=fmt)
    got = _state(dev, part, x)
    assert got[0] == host[0] and same_bits(got[1], host[1])
    dev.spmm_refresh_lr_values_device(part, *to_device(indptr, indices, data2))
    assert same_bits(product(dev, MUL[part], x), fresh[1])


def test_refused_device_setups_and_refreshes_of_a_part(dev):
    indptr, indices, data = _matrix("1000")
    n, m = 1000, 3
    x = np.asfortranarray(np.random.default_rng(4).standard_normal((n, m)))
    st = _dev_call(dev, "dla_spmm_refresh_lr_values_dev", "amb", n, (indptr, indices, data))
    msg = dev.lib.dla_last_error(dev.h).decode()
    assert st == capi.ERR_ARG and "spmm_refresh_lr_values_dev" in msg and "amb" in msg and "not been set up" in msg, (st, msg)
    setup_lr(dev, "amb", n, indptr, indices, data, "sell")
    before = _state(dev, "amb", x)
    bad_col = indices.copy()
    bad_col[1234] = n
    down = indptr.copy()
    down[501] = down[500] - 1
    for entry_args, text in [((n, (indptr, bad_col, data), "sell"), "column index out of range"), ((n, (down, indices, data), "ell"), "row pointers not ascending"),
                             ((n, (indptr, indices, data), None), None)]:
        if text is None:
            st = dev.lib.dla_spmm_setup_lr_csr_dev(dev.h, 4, n, 8, 8, 8, FMT["ell"])          # (the part is checked before any pointer is used)
            text = "part must be"
        else:
            st = _dev_call(dev, "dla_spmm_setup_lr_csr_dev", "amb", *entry_args)
        msg = dev.lib.dla_last_error(dev.h).decode()
        assert st == capi.ERR_ARG and "spmm_setup_lr_csr_dev" in msg and text in msg, (st, msg)
        after = _state(dev, "amb", x)
        assert after[0] == before[0] and same_bits(after[1], before[1])
    t = to_device(indptr, indices, data)
    for args in ((0, t[1].data_ptr(), t[2].data_ptr()), (t[0].data_ptr(), 0, t[2].data_ptr()), (t[0].data_ptr(), t[1].data_ptr(), 0)):
        st = dev.lib.dla_spmm_setup_lr_csr_dev(dev.h, PART["amb"], n, *args, FMT["ell"])
        msg = dev.lib.dla_last_error(dev.h).decode()
        assert st == capi.ERR_ARG and "spmm_setup_lr_csr_dev" in msg and "bad arguments" in msg, (st, msg)
    after = _state(dev, "amb", x)
    assert after[0] == before[0] and same_bits(after[1], before[1])


# ------------------------------------------------------------------------------------------------------------------ 4. lrprec1 / lrprec2
def _diagonal_parts(ctx, n, rng):
    """three parts with random diagonals and one off-diagonal band each (the band must not reach the preconditioner); the ranges
    keep both denominators away from zero for fac = 0.3 and -1.7: aa in [2, 3] and sg in [0.1, 0.4] give
    aa^2 - fac^2 sg^2 >= 4 - 2.89 x 0.16 > 3.5 and fac^2 aa^2 - sg^2 >= 0.09 x 4 - 0.16 = 0.2"""
    d = {"apb": rng.uniform(2.5, 3.5, n), "amb": rng.uniform(1.5, 2.5, n), "spd": rng.uniform(0.1, 0.4, n)}
    for k, (p, diag) in enumerate(d.items()):
        ctx.spmm_setup_lr(p, (sp.diags(diag) + sp.diags(rng.standard_normal(n - 1 - k), 1 + k)).tocsr(), fmt="sell" if k == 1 else "ell")
    return d


def _lrprec(ctx, variant, n, m, fac, xp, xm, offsets):
    g = [Guarded(ctx, n, m, xp, offsets[0]), Guarded(ctx, n, m, xm, offsets[1]), Guarded(ctx, n, m, None, offsets[2]), Guarded(ctx, n, m, None, offsets[3])]
    ctx._chk(ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(f"dla_spmm_lrprec{variant}"), n, m, fac, *(b.ptr for b in g)))
    yp, ym = g[2].body().copy(), g[3].body().copy()
    g[0].assert_unchanged(); g[1].assert_unchanged()
    vector = n % 2 == 0 and all(b.ptr % 16 == 0 for b in g)
    for b in g:
        b.free()
    return yp, ym, vector


# (n, m, byte offsets of xp, xm, yp, ym): aligned blocks (n even: the 16-byte instance), one block 8 bytes off in turn (the scalar
# instance on even n), odd n (every second column is 8 bytes off whatever the offsets)
LRPREC_CASES = [(1000, 7, (0, 0, 0, 0)), (1000, 1, (0, 0, 0, 0)), (1000, 7, (8, 0, 0, 0)), (1000, 7, (0, 8, 0, 0)), (1000, 1, (0, 0, 8, 0)),
                (1000, 7, (0, 0, 0, 8)), (1000, 7, (8, 8, 8, 8)), (1001, 7, (0, 0, 0, 0)), (1001, 1, (0, 0, 0, 0)), (1001, 1, (8, 8, 8, 8)), (1001, 7, (0, 8, 8, 0))]


@pytest.mark.parametrize("n,m,offsets", LRPREC_CASES)
def test_lrprec_against_numpy_bit_for_bit(dev, rng, n, m, offsets):
    """The bit check holds (no fused operation outside the divisions): the componentwise bound of the issue is not needed."""
    d = _diagonal_parts(dev, n, rng)
    xp, xm = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
    aa = 0.5 * (d["apb"] + d["amb"])
    dev.reset_stats()
    for variant in (1, 2):
        for fac in (0.3, -1.7):
            pole = aa * aa - fac * fac * d["spd"] ** 2 if variant == 1 else fac * fac * aa * aa - d["spd"] ** 2
            assert np.abs(pole).min() >= 0.1
            yp, ym, vector = _lrprec(dev, variant, n, m, fac, xp, xm, offsets)
            assert vector == (n % 2 == 0 and not any(offsets))
            wp, wm = lrprec_numpy(variant, fac, d["apb"], d["amb"], d["spd"], xp, xm)
            assert same_bits(yp, wp), f"lrprec{variant} fac={fac}: yp differs in {int((yp != wp).sum())} places, max {np.abs(yp - wp).max():.3e}"
            assert same_bits(ym, wm), f"lrprec{variant} fac={fac}: ym differs in {int((ym != wm).sum())} places, max {np.abs(ym - wm).max():.3e}"
    # booked: four launches under no kernel name, 32 n m + 24 n bytes and 8 n m flops each
    pc = dev.stats()["precnd"]
    assert (pc["launches"], pc["alg_bytes"], pc["flops"]) == (4, 4 * (32.0 * n * m + 24.0 * n), 4 * 8.0 * n * m), pc
    assert not any(v["launches"] for v in dev.kernel_stats().values()), dev.kernel_stats()


def test_lrprec_takes_a_second_stride_trip(dev, rng):
    """one trip of the 16-byte instance covers 2 x 8 x 256 rows per compute unit (1 048 576 on 256): 1 400 002 rows need a second"""
    import torch
    n, m = 1_400_002, 1
    assert n > 2 * 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    try:
        d = _diagonal_parts(dev, n, rng)
        xp, xm = (np.asfortranarray(rng.standard_normal((n, m))) for _ in range(2))
        yp, ym, vector = _lrprec(dev, 1, n, m, -1.7, xp, xm, (0, 0, 0, 0))
        wp, wm = lrprec_numpy(1, -1.7, d["apb"], d["amb"], d["spd"], xp, xm)
        assert vector and same_bits(yp, wp) and same_bits(ym, wm)
    finally:
        dev.spmm_drop_lr()
        dev.trim()


# ------------------------------------------------------------------------------------------------------------------ 5. whole solves
N, T, M, MAX_DAV, TOL = 300, 3, 6, 20, 1e-9


@pytest.fixture(scope="module")
def pencil():
    mats = random_pencil(N)
    assert positive_definite(mats)
    return {"mats": mats, "dense": dense_roots(mats, T)}


@pytest.mark.parametrize("fmt", ["ell", "sell"])
@pytest.mark.parametrize("trad", [False, True], ids=["caslr_eff", "caslr"])
def test_linear_response_solve_on_the_sparse_parts(ctx, pencil, trad, fmt):
    """Panels, the four matrices and the preconditioner stay in HBM through the whole solve.  Tolerance: ten times the error of the
    same driver in host-callback mode (scipy products, numpy lrprec) against the dense solve, at most 1e-8 relative.  Measured on
    an MI355X: the host-callback solve is 2.55e-14 (caslr_eff_driver) and 2.60e-14 (caslr_driver) from scipy.linalg.eig, 7
    iterations each, which makes the allowed error 2.6e-13; the device solves are 2.55e-14 from it in both formats, 7 iterations
    (most of that distance is the dense non-symmetric solver's own error)."""
    mats, want = pencil["mats"], pencil["dense"]
    try:
        eig_h, ok_h, info_h = solve_host_mode(ctx, mats, trad, T, M, 100, TOL, MAX_DAV)
        eig_d, ok_d, info_d, vec = solve_device_mode(ctx, mats, trad, T, M, 100, TOL, MAX_DAV, fmt=fmt)
    finally:
        ctx.spmm_drop_lr()
    host_err, allowed = tolerance(eig_h, want)
    dev_err = float(np.abs(eig_d / want - 1.0).max())
    print(f"{'caslr' if trad else 'caslr_eff'} / {fmt}: host-callback error {host_err:.3e} ({info_h['iters']} iterations), "
          f"device error {dev_err:.3e} ({info_d['iters']} iterations), allowed {allowed:.3e}")
    assert ok_h and ok_d, (info_h, info_d)
    assert abs(info_h["iters"] - info_d["iters"]) <= 1, (info_h, info_d)
    assert dev_err <= allowed, (dev_err, allowed, eig_d, want)
    # residual of the pencil with the matrices themselves
    apb, amb, spd, smd = (mats[p] for p in PARTS)
    for j in range(T):
        y, z = vec[:N, j], vec[N:, j]
        lhs = np.concatenate([0.5 * (apb @ (y + z) + amb @ (y - z)), 0.5 * (apb @ (y + z) - amb @ (y - z))])
        rhs = np.concatenate([0.5 * (spd @ (y + z) + smd @ (y - z)), 0.5 * (smd @ (y - z) - spd @ (y + z))])
        assert np.linalg.norm(lhs - eig_d[j] * rhs) / np.linalg.norm(lhs) < 1e-7


# ------------------------------------------------------------------------------------------------------------------ 6. errors
def _failed_matvec(ctx, name, n, m=2):
    gx, gy = Guarded(ctx, n, m, np.ones((n, m))), Guarded(ctx, n, m)
    st = ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, gx.ptr, gy.ptr)
    msg = ctx.lib.dla_last_error(ctx.h).decode()
    assert np.all(gy.body() == 7.0), "a refused callback wrote its output block"
    gx.free(); gy.free()
    return st, msg


def _failed_lrprec(ctx, name, n, m=2):
    g = [Guarded(ctx, n, m, np.ones((n, m))), Guarded(ctx, n, m, np.ones((n, m))), Guarded(ctx, n, m), Guarded(ctx, n, m)]
    st = ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(name), n, m, 0.3, *(b.ptr for b in g))
    msg = ctx.lib.dla_last_error(ctx.h).decode()
    assert np.all(g[2].body() == 7.0) and np.all(g[3].body() == 7.0), "a refused callback wrote its output blocks"
    for b in g:
        b.free()
    return st, msg


def test_callbacks_refuse_a_missing_or_mismatched_part(dev, rng):
    n = 1000
    a = _banded(n, 3, rng)
    dev.spmm_setup_lr("apb", a)
    st, msg = _failed_matvec(dev, "dla_spmm_ambmul", n)
    assert st != 0 and "dla_spmm_ambmul" in msg and "amb" in msg and "not been set up" in msg, (st, msg)
    dev.spmm_setup_lr("amb", a, fmt="sell")
    for name in ("dla_spmm_lrprec1", "dla_spmm_lrprec2"):
        st, msg = _failed_lrprec(dev, name, n)
        assert st != 0 and name in msg and "spd" in msg and "not been set up" in msg, (st, msg)
    dev.spmm_setup_lr("spd", _banded(n - 100, 2, rng))
    st, msg = _failed_lrprec(dev, "dla_spmm_lrprec1", n)
    assert st != 0 and "dla_spmm_lrprec1" in msg and "spd" in msg and "differs" in msg, (st, msg)
    st, msg = _failed_matvec(dev, "dla_spmm_spdmul", n)
    assert st != 0 and "dla_spmm_spdmul" in msg and "spd" in msg and "differs" in msg, (st, msg)
    st, msg = _failed_matvec(dev, "dla_spmm_smdmul", n)
    assert st != 0 and "dla_spmm_smdmul" in msg and "smd" in msg, (st, msg)
    # the context goes on working
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    assert within_scipy_bound(product(dev, "dla_spmm_apbmul", x), a, x)
    assert within_scipy_bound(product(dev, "dla_spmm_ambmul", x), a, x)


def test_a_sharded_operator_and_the_parts_exclude_each_other(dev, rng):
    """row-sharded parts do not exist: a part is refused beside a sharded operator, the sharded set-up beside a part"""
    n = 600
    a = _banded(n, 3, rng)
    _, ia, ja, va = raw(a)
    x = np.asfortranarray(rng.standard_normal((n, 3)))
    dev.spmm_drop_metric()
    setup_csr_one_shard(dev, n, ia, ja, va)
    try:
        ax = product(dev, "dla_spmm_matvec", x)
        with pytest.raises(capi.DlaError, match="spmm_setup_lr_csr:.*row-sharded"):
            dev.spmm_setup_lr("apb", a)
        st = _dev_call(dev, "dla_spmm_setup_lr_csr_dev", "spd", n, (ia, ja, va), "ell")
        msg = dev.lib.dla_last_error(dev.h).decode()
        assert st == capi.ERR_ARG and "spmm_setup_lr_csr_dev:" in msg and "row-sharded" in msg, (st, msg)
        for p in PARTS:
            with pytest.raises(capi.DlaError, match="not been set up"):
                dev.spmm_lr_info(p)
        assert same_bits(product(dev, "dla_spmm_matvec", x), ax)
    finally:
        setup_csr(dev, n, ia, ja, va)
    dev.spmm_setup_lr("smd", a)
    y = product(dev, "dla_spmm_smdmul", x)
    with pytest.raises(capi.DlaError, match="spmm_setup_csr_sharded.*linear-response parts"):
        setup_csr_one_shard(dev, n, ia, ja, va)
    assert same_bits(product(dev, "dla_spmm_smdmul", x), y) and same_bits(product(dev, "dla_spmm_matvec", x), ax)
    dev.spmm_drop_lr()
    setup_csr_one_shard(dev, n, ia, ja, va)            # (without parts the sharded set-up is accepted again)
    setup_csr(dev, n, ia, ja, va)
