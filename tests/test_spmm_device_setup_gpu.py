"""GPU: the sparse operator and the metric set up from CSR arrays in DEVICE memory (dla_spmm_setup_csr_dev) and new values for a stored
pattern (dla_spmm_refresh_values_dev) -- csr_check_cols_kernel, ell_fill_kernel, sell_fill_kernel, tail_copy_kernel, csr_diag_kernel
and pattern_compare_kernel of diaglib_amd/csrc/hip_engine.hip.

The oracle is the set-up from HOST arrays (dla_spmm_setup_csr_fmt / dla_spmm_setup_metric_csr), which this work leaves as it was: the
contract is the same operator, so every comparison is of raw bytes (np.array_equal on the uint64 view, which also tells -0.0 from
0.0) and of the info dicts, never a tolerance.  The host set-up runs on a context of its own ("set up from host arrays on one context
and from device arrays on another"); the sparse callbacks act on the context the thread set up last, so a slot's products are always
taken right after its set-up, before the other context is touched.  Every device set-up of this file overwrites the caller's tensors
with NaN / out-of-range indices as soon as the call returns: all products below are taken after that, so all of them also show that
the call is synchronous."""
import ctypes as C

import numpy as np
import pytest

from diaglib_amd import capi
from spmm_cases import LONG_ROW, csr_from_lengths, skewed_csr
from spmm_slots import fresh_context, info, poison, precnd, product, refresh_status, same_bits, setup_status, to_device
from test_operators_gpu import ragged_csr, setup_csr_one_shard
from test_sell_layout_split import LONG_SEG, special_lengths
from test_spmm_gpu import _laplacian_2d

pytestmark = pytest.mark.gpu
FMT = capi.SPMM_FORMATS
A, B = 0, 1
MS = (1, 8, 9, 13)            # right-hand sides: below, at and above the chunk of 8 of sell_spmm_kernel, and a chunk with a remainder


@pytest.fixture()
def dev(ctx):
    """device callbacks on; the session's context is handed back without a metric"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.spmm_drop_metric()


@pytest.fixture(scope="module")
def other():
    """the second context: the host-array set-ups that the device-array ones are compared with"""
    with fresh_context() as c:
        yield c


# ------------------------------------------------------------------------------------------------------------------ matrices
def _special(rng, n):
    """special_lengths, with two (i, i) entries far apart in the row of 8193 entries (tail, first and second segment) and in the row
    of LONG_ROW entries (a slice row) on top of whatever the uniform columns hit"""
    lens = special_lengths(rng, n)
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    for length, places in ((2 * LONG_SEG + 1, (5, 5000)), (LONG_ROW, (3, 200))):
        for r in np.flatnonzero(lens == length):
            indices[indptr[r] + np.array(places)] = r
            data[indptr[r] + np.array(places)] = (1.75, -0.3125)
    return indptr, indices, data


def _uniform(rng, n):
    return csr_from_lengths(rng, n, np.full(n, 5))


# name -> (n, builder, formats): ELLPACK only where widest row x n stays small; "uniform" is the matrix AUTO keeps in ELLPACK
CASES = {
    "one_row": (1, lambda rng: csr_from_lengths(rng, 1, np.array([3])), ("ell", "sell", "auto")),
    "ragged63": (63, lambda rng: ragged_csr(rng, 63, 9), ("ell", "sell", "auto")),
    "ragged64": (64, lambda rng: ragged_csr(rng, 64, 9), ("ell", "sell", "auto")),
    "ragged65": (65, lambda rng: ragged_csr(rng, 65, 9), ("ell", "sell", "auto")),            # the last slice partly beyond n
    "special65": (65, lambda rng: _special(rng, 65), ("ell", "sell", "auto")),                  # ELLPACK 8193 wide: rows no thread walks alone
    "ragged4096": (4096, lambda rng: ragged_csr(rng, 4096, 33), ("ell", "sell", "auto")),
    "ragged4097": (4097, lambda rng: ragged_csr(rng, 4097, 9), ("ell", "sell", "auto")),       # the second window
    "uniform4097": (4097, lambda rng: _uniform(rng, 4097), ("ell", "sell", "auto")),
    "special4097": (4097, lambda rng: _special(rng, 4097), ("sell", "auto")),
    "skewed9000": (9000, lambda rng: skewed_csr(rng, 9000), ("sell", "auto")),                  # one dense row: three segments
    "special9000": (9000, lambda rng: _special(rng, 9000), ("sell", "auto")),
}
_MATRICES = {}


def matrix(name):
    if name not in _MATRICES:
        n, build, _ = CASES[name]
        _MATRICES[name] = (n,) + tuple(build(np.random.default_rng(sum(map(ord, name)))))
    return _MATRICES[name]


def vectors(n, m):
    return np.asfortranarray(np.random.default_rng(7 * n + m).standard_normal((n, m)))


# ------------------------------------------------------------------------------------------------------------------ plumbing
def setup_host(c, which, *csr_and_format):
    c._chk(setup_status(c, which, *csr_and_format))


def dev_call(c, entry, which, n, arrays, fmt=None):
    """status of one call of a device-array entry on (indptr, indices, data); the tensors are poisoned after it"""
    slot = which if which in (A, B) else ("which", which)
    return setup_status(c, slot, n, *arrays, fmt, "device") if entry == "dla_spmm_setup_csr_dev" else refresh_status(c, slot, n, *arrays)


def setup_dev(c, which, n, indptr, indices, data, fmt):
    c._chk(dev_call(c, "dla_spmm_setup_csr_dev", which, n, (indptr, indices, data), fmt))


def refresh_dev(c, which, n, indptr, indices, data):
    c._chk(dev_call(c, "dla_spmm_refresh_values_dev", which, n, (indptr, indices, data)))


def refused(c, entry, which, n, arrays, fmt=None):
    st = dev_call(c, entry, which, n, arrays, fmt)
    msg = c.lib.dla_last_error(c.h).decode()
    assert st == capi.ERR_ARG and entry[4:] in msg, (st, msg)
    return msg


def slot_results(c, which, n, pencil=False):
    """everything the contract names for one slot: info, products for every m of MS, the preconditioner(s)"""
    out = {"info": info(c, which)}
    for m in MS:
        out[f"product m={m}"] = product(c, "dla_spmm_bvec" if which == B else "dla_spmm_matvec", vectors(n, m))
    if which == A:
        out["precnd"] = precnd(c, "dla_spmm_precnd", vectors(n, 3))
    if pencil:
        out["precnd_pencil"] = precnd(c, "dla_spmm_precnd_pencil", vectors(n, 3))
    return out


def assert_same_results(got, want, what):
    assert got.keys() == want.keys()
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    for k in want:
        if k != "info":
            assert same_bits(got[k], want[k]), f"{what}: {k} differs from the host set-up in {int((got[k] != want[k]).sum())} places"


_HOST = {}


def host_results(other, name, fmt, which):
    """the host-array set-up's results, computed once per (matrix, format, slot)"""
    key = (name, fmt, which)
    if key not in _HOST:
        n, indptr, indices, data = matrix(name)
        setup_host(other, which, n, indptr, indices, data, fmt)
        _HOST[key] = slot_results(other, which, n)
    return _HOST[key]


PARITY = [(name, fmt) for name, (_, _, fmts) in CASES.items() for fmt in fmts]


# ------------------------------------------------------------------------------------------------------------------ 1. the same operator
@pytest.mark.parametrize("which", [A, B], ids=["A", "B"])
@pytest.mark.parametrize("name,fmt", PARITY)
def test_device_setup_is_the_host_setup(dev, other, name, fmt, which):
    n, indptr, indices, data = matrix(name)
    want = host_results(other, name, fmt, which)
    setup_dev(dev, which, n, indptr, indices, data, fmt)
    assert_same_results(slot_results(dev, which, n), want, f"{name} {fmt} slot {which}")
    lens = np.diff(indptr)
    if name.startswith("special") and n >= 4097 or name == "special65" and fmt != "ell":
        i = want["info"]
        assert i["format"] == "sell" and i["long_rows"] == int((lens > LONG_ROW).sum()) and i["multi_segments"] == 5
    if name == "uniform4097" and fmt == "auto":
        assert want["info"]["format"] == "ell"


@pytest.mark.parametrize("name,fmt_a,fmt_b", [("ragged4097", "ell", "sell"), ("special4097", "sell", "sell"), ("special65", "sell", "ell")])
def test_pencil_preconditioner_with_both_slots_from_device_arrays(dev, other, name, fmt_a, fmt_b):
    """B = the same pattern with other values (shifted by one entry), so that a_ii + fac b_ii is not a multiple of a_ii"""
    n, indptr, indices, data = matrix(name)
    data_b = np.roll(data, 1) + 0.25
    setup_host(other, A, n, indptr, indices, data, fmt_a)
    setup_host(other, B, n, indptr, indices, data_b, fmt_b)
    want = [slot_results(other, A, n, pencil=True), slot_results(other, B, n, pencil=True)]
    setup_dev(dev, A, n, indptr, indices, data, fmt_a)
    setup_dev(dev, B, n, indptr, indices, data_b, fmt_b)
    for which in (A, B):
        assert_same_results(slot_results(dev, which, n, pencil=True), want[which], f"{name} pencil slot {which}")


def test_only_long_row_has_three_segments(dev, other):
    n = 300
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 4, n)
    lens[17] = 2 * LONG_SEG + 1
    arrays = csr_from_lengths(rng, n, lens)
    setup_host(other, A, n, *arrays, "sell")
    want = slot_results(other, A, n)
    assert (want["info"]["long_rows"], want["info"]["long_segments"], want["info"]["multi_segments"]) == (1, 3, 3)
    setup_dev(dev, A, n, *arrays, "sell")
    assert_same_results(slot_results(dev, A, n), want, "one row of 8193 entries")


@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_duplicate_diagonal_entries_in_a_short_and_in_a_tail_row(dev, other, fmt):
    """values whose sum depends on the order: in the caller's order (1e16 + 1.0) + -1e16 = 0.0, in any other 1.0.  The stored diagonal
    shows through dla_spmm_precnd, x / (d + fac): with fac = 0.5 the right diagonal gives 2 x exactly, the wrong one x / 1.5"""
    n = 70
    rng = np.random.default_rng(12)
    lens = rng.integers(1, 5, n)
    lens[3], lens[40] = 6, LONG_ROW + 44
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    for r, places in ((3, (0, 2, 5)), (40, (1, 70, 299))):
        row = indices[indptr[r]:indptr[r + 1]]          # (a view)
        row[row == r] = (r + 1) % n
        row[np.array(places)] = r
        data[indptr[r] + np.array(places)] = (1e16, 1.0, -1e16)
    setup_host(other, A, n, indptr, indices, data, fmt)
    x = vectors(n, 2)
    want = precnd(other, "dla_spmm_precnd", x, fac=0.5)
    setup_dev(dev, A, n, indptr, indices, data, fmt)
    got = precnd(dev, "dla_spmm_precnd", x, fac=0.5)
    assert same_bits(got, want)
    assert np.array_equal(got[[3, 40]], 2.0 * x[[3, 40]])


@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_row_pointers_that_do_not_start_at_zero(dev, other, fmt):
    """the host entries index the entry arrays with the row pointers as they are (rowptr[0] entries in front are never read) and
    accept such a matrix; the device entry does the same"""
    n, indptr, indices, data = matrix("ragged65")
    front = 7
    ip = indptr + front
    ci = np.concatenate([np.zeros(front, np.int32), indices])
    va = np.concatenate([np.full(front, 99.0), data])
    setup_host(other, A, n, ip, ci, va, fmt)
    want = slot_results(other, A, n)
    assert want["info"]["nnz"] == len(indices)
    assert_same_results(want, host_results(other, "ragged65", fmt, A), "host entry, shifted row pointers")
    setup_dev(dev, A, n, ip, ci, va, fmt)
    assert_same_results(slot_results(dev, A, n), want, "shifted row pointers")


# ------------------------------------------------------------------------------------------------------------------ 2. refresh
def _scaled(n, indptr, indices, data):
    """D A D with d_i = 1 + 0.5 sin(i): symmetric where A is, and no two entries scaled alike"""
    d = 1.0 + 0.5 * np.sin(np.arange(n, dtype=np.float64))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    return data * d[rows] * d[indices]


@pytest.mark.parametrize("which", [A, B], ids=["A", "B"])
@pytest.mark.parametrize("name,fmt", [("ragged4097", "ell"), ("special65", "ell"), ("special4097", "sell"), ("skewed9000", "sell"), ("uniform4097", "auto")])
def test_refresh_equals_a_fresh_setup(dev, other, name, fmt, which):
    n, indptr, indices, data = matrix(name)
    new = _scaled(n, indptr, indices, data)
    assert not np.array_equal(new, data)
    setup_host(other, which, n, indptr, indices, new, fmt)
    want = slot_results(other, which, n)
    # the other slot of the refreshed context holds something else, and keeps it
    bystander = A if which == B else B
    n2, ip2, ci2, va2 = matrix("ragged4097" if n == 4097 else "ragged65")
    setup_dev(dev, bystander, n2, ip2, ci2, va2, "sell")
    before = slot_results(dev, bystander, n2)
    setup_dev(dev, which, n, indptr, indices, data, fmt)
    refresh_dev(dev, which, n, indptr, indices, new)
    assert_same_results(slot_results(dev, which, n), want, f"refreshed {name} {fmt} slot {which}")
    assert_same_results(slot_results(dev, bystander, n2), before, "the slot that was not refreshed")


def test_refresh_after_a_host_setup_and_with_shifted_row_pointers(dev, other):
    n, indptr, indices, data = matrix("special4097")
    new = _scaled(n, indptr, indices, data)
    setup_host(other, A, n, indptr, indices, new, "sell")
    want = slot_results(other, A, n)
    setup_host(dev, A, n, indptr, indices, data, "sell")
    refresh_dev(dev, A, n, indptr + 3, np.concatenate([np.zeros(3, np.int32), indices]), np.concatenate([np.zeros(3), new]))
    assert_same_results(slot_results(dev, A, n), want, "refresh of a slot that host arrays set up")


# ------------------------------------------------------------------------------------------------------------------ 3. refusals
def _unchanged(c, which, n, before):
    assert_same_results(slot_results(c, which, n), before, "after a refused call")


@pytest.mark.parametrize("which", [A, B], ids=["A", "B"])
@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_refused_setups_replace_nothing(dev, fmt, which):
    """The out-of-range columns are caught by csr_check_cols_kernel, which runs alone and is waited for before any kernel indexes
    with a column (the launch order is written down at setup_dev in hip_engine.hip): nothing here indexes out of bounds.  The
    refused matrices are LARGER than the stored one, so a set-up that grew the slot's blocks before its checks would lose them."""
    n, indptr, indices, data = matrix("ragged65")
    setup_dev(dev, which, n, indptr, indices, data, fmt)
    before = slot_results(dev, which, n)
    nb, ipb, cib, vab = matrix("ragged4097")
    mid = len(cib) // 2
    for bad_col in (nb, -1):
        ci = cib.copy()
        ci[mid] = bad_col
        assert "column index out of range" in refused(dev, "dla_spmm_setup_csr_dev", which, nb, (ipb, ci, vab), FMT[fmt])
        _unchanged(dev, which, n, before)
    ip = ipb.copy()
    ip[100] = ip[101] + 1
    assert "row pointers not ascending" in refused(dev, "dla_spmm_setup_csr_dev", which, nb, (ip, cib, vab), FMT[fmt])
    assert "unknown format" in refused(dev, "dla_spmm_setup_csr_dev", which, nb, (ipb, cib, vab), 7)
    assert "which" in refused(dev, "dla_spmm_setup_csr_dev", 2, nb, (ipb, cib, vab), FMT[fmt])
    assert "empty matrix" in refused(dev, "dla_spmm_setup_csr_dev", which, nb, (np.zeros(nb + 1, np.int64), cib, vab), FMT[fmt])
    assert "bad arguments" in refused(dev, "dla_spmm_setup_csr_dev", which, 0, (ipb, cib, vab), FMT[fmt])
    assert dev.lib.dla_spmm_setup_csr_dev(dev.h, which, nb, None, None, None, FMT[fmt]) == capi.ERR_ARG
    _unchanged(dev, which, n, before)


def test_refresh_before_any_setup_is_refused(dev):
    n, indptr, indices, data = matrix("ragged65")
    with fresh_context() as c:
        assert "no operator" in refused(c, "dla_spmm_refresh_values_dev", A, n, (indptr, indices, data))
        assert "no metric" in refused(c, "dla_spmm_refresh_values_dev", B, n, (indptr, indices, data))
        assert c.lib.dla_spmm_info(c.h, C.byref(capi.SpmmInfo())) == capi.ERR_ARG
    setup_dev(dev, A, n, indptr, indices, data, "ell")         # (the thread's operator is the session context's again)
    dev.spmm_drop_metric()
    assert "no metric" in refused(dev, "dla_spmm_refresh_values_dev", B, n, (indptr, indices, data))
    assert "which" in refused(dev, "dla_spmm_refresh_values_dev", 2, n, (indptr, indices, data))


def _swap_two_lengths(indptr):
    """two neighbouring rows of different length trade lengths: the entry count stays"""
    lens = np.diff(indptr)
    i = int(np.flatnonzero(lens[:-1] != lens[1:])[len(lens) // 3])
    lens[i], lens[i + 1] = lens[i + 1], lens[i]
    ip = np.zeros_like(indptr)
    np.cumsum(lens, out=ip[1:])
    assert ip[-1] == indptr[-1] and not np.array_equal(ip, indptr)
    return ip


@pytest.mark.parametrize("which", [A, B], ids=["A", "B"])
@pytest.mark.parametrize("name,fmt", [("special4097", "sell"), ("ragged4097", "ell")])
def test_refused_refreshes_leave_values_and_diagonal(dev, name, fmt, which):
    n, indptr, indices, data = matrix(name)
    new = _scaled(n, indptr, indices, data)
    setup_dev(dev, which, n, indptr, indices, data, fmt)
    before = slot_results(dev, which, n)
    lens = np.diff(indptr)
    # another n (one row less, the entries of the rest)
    assert "differs from the stored" in refused(dev, "dla_spmm_refresh_values_dev", which, n - 1, (indptr[:-1], indices, new))
    # another number of entries (the last row one entry longer)
    ip = indptr.copy()
    ip[-1] += 1
    assert "entries" in refused(dev, "dla_spmm_refresh_values_dev", which, n, (ip, np.append(indices, np.int32(0)), np.append(new, 1.0)))
    _unchanged(dev, which, n, before)
    # one column changed: in a row that lives in a slice (ELLPACK: any row) ...
    short = np.flatnonzero((lens >= 2) & (lens <= LONG_ROW))
    short = int(short[len(short) // 2])
    ci = indices.copy()
    ci[indptr[short] + 1] = (ci[indptr[short] + 1] + 1) % n
    assert "columns" in refused(dev, "dla_spmm_refresh_values_dev", which, n, (indptr, ci, new))
    _unchanged(dev, which, n, before)
    # ... and in a tail row, in its last segment
    if fmt == "sell":
        tail = int(np.flatnonzero(lens == 2 * LONG_SEG + 1)[0])
        ci = indices.copy()
        ci[indptr[tail + 1] - 1] = (ci[indptr[tail + 1] - 1] + 1) % n
        assert "columns" in refused(dev, "dla_spmm_refresh_values_dev", which, n, (indptr, ci, new))
        _unchanged(dev, which, n, before)
    # two row lengths swapped, the entry count unchanged
    assert "row pointers" in refused(dev, "dla_spmm_refresh_values_dev", which, n, (_swap_two_lengths(indptr), indices, new))
    _unchanged(dev, which, n, before)
    # and the slot still takes a good refresh
    refresh_dev(dev, which, n, indptr, indices, new)
    assert not same_bits(slot_results(dev, which, n)["product m=1"], before["product m=1"])


def test_sharded_operator_refuses_refresh_and_device_metric(dev):
    n, indptr, indices, data = matrix("ragged65")
    dev.spmm_drop_metric()
    setup_csr_one_shard(dev, n, indptr, indices, data)
    x = vectors(n, 3)
    ax = product(dev, "dla_spmm_matvec", x)
    assert "row-sharded" in refused(dev, "dla_spmm_refresh_values_dev", A, n, (indptr, indices, data * 2.0))
    assert same_bits(product(dev, "dla_spmm_matvec", x), ax)
    assert "row-sharded" in refused(dev, "dla_spmm_setup_csr_dev", B, n, (indptr, indices, data), FMT["ell"])
    with pytest.raises(capi.DlaError, match="no metric"):
        dev.spmm_metric_info()
    assert same_bits(product(dev, "dla_spmm_matvec", x), ax)
    # a device set-up of A makes the operator whole again, as dla_spmm_setup_csr_fmt does
    setup_dev(dev, A, n, indptr, indices, data, "ell")
    setup_dev(dev, B, n, indptr, indices, data, "ell")
    assert same_bits(product(dev, "dla_spmm_bvec", x), product(dev, "dla_spmm_matvec", x))


# ------------------------------------------------------------------------------------------------------------------ 4. use after return
@pytest.mark.parametrize("fmt", ["ell", "sell"])
def test_the_callers_arrays_may_be_overwritten_when_the_call_returns(dev, other, fmt):
    """explicitly what every set-up of this file does: NaN over the values, out-of-range numbers over the indices, then products"""
    import torch
    name = "special4097" if fmt == "sell" else "ragged4096"
    n, indptr, indices, data = matrix(name)
    want = host_results(other, name, fmt, A)
    t = to_device(indptr, indices, data)
    dev._chk(dev.lib.dla_spmm_setup_csr_dev(dev.h, A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), FMT[fmt]))
    poison(t)
    assert bool(torch.isnan(t[2]).all())
    assert_same_results(slot_results(dev, A, n), want, "after the caller's arrays were overwritten")
    new = _scaled(n, indptr, indices, data)
    t = to_device(indptr, indices, new)
    dev._chk(dev.lib.dla_spmm_refresh_values_dev(dev.h, A, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()))
    poison(t)
    del t
    got = slot_results(dev, A, n)
    setup_host(other, A, n, indptr, indices, new, fmt)
    assert_same_results(got, slot_results(other, A, n), "refresh, after the caller's arrays were overwritten")


# ------------------------------------------------------------------------------------------------------------------ 5. the Python wrapper
def _davidson(c, n, guess):
    c.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ev = c.panel(guess)
    eig, _, ok, info = c.davidson_driver(n, 4, 8, 1000, 1e-8, 20, 0.0, capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_precnd"), ev)
    vec = ev.download()
    ev.free()
    return eig, vec, ok, info


def test_torch_sparse_csr_tensor_through_the_wrapper(dev):
    """the 2-D Laplacian of tests/test_spmm_gpu.py (96 x 64, the smallest grid the suite uses) as a torch.sparse_csr_tensor with
    int64 indices: the solve reproduces the host-set-up solve bit for bit"""
    import torch
    a = _laplacian_2d(96, 64)
    n = a.shape[0]
    guess = np.asfortranarray(np.random.default_rng(5).random((n, 8)) - 0.5)
    dev.spmm_setup(a)
    info_host = dev.spmm_info()
    eig0, vec0, ok0, it0 = _davidson(dev, n, guess)
    assert ok0, it0
    t = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64)),
                                torch.from_numpy(a.data.astype(np.float64)), size=a.shape).cuda()
    assert t.col_indices().dtype == torch.int64
    dev.spmm_setup_device(t.crow_indices(), t.col_indices(), t.values())
    assert dev.spmm_info() == info_host
    eig1, vec1, ok1, it1 = _davidson(dev, n, guess)
    assert ok1 and it1 == it0, (it0, it1)
    assert same_bits(eig1, eig0) and same_bits(vec1, vec0)
    # host tensors and int32 row pointers are converted; the metric slot and a refresh through the wrapper
    x = vectors(n, 3)
    ax = product(dev, "dla_spmm_matvec", x)
    dev.spmm_setup_device(torch.from_numpy(a.indptr.astype(np.int32)), torch.from_numpy(a.indices.astype(np.int32)), torch.from_numpy(a.data), fmt="sell",
                          metric=True)
    assert dev.spmm_metric_info()["format"] == "sell" and same_bits(product(dev, "dla_spmm_bvec", x), ax)
    dev.spmm_refresh_values_device(t.crow_indices(), t.col_indices(), 2.0 * t.values(), metric=True)
    assert same_bits(product(dev, "dla_spmm_bvec", x), 2.0 * ax)
    # refused before anything reaches the library
    with pytest.raises(ValueError, match="fmt"):
        dev.spmm_setup_device(t.crow_indices(), t.col_indices(), t.values(), fmt="csr")
    with pytest.raises(ValueError, match="int32 or int64"):
        dev.spmm_setup_device(t.crow_indices().double(), t.col_indices(), t.values())
    with pytest.raises(ValueError, match="floating"):
        dev.spmm_setup_device(t.crow_indices(), t.col_indices(), t.col_indices())
    with pytest.raises(ValueError, match="32 bits"):
        dev.spmm_setup_device(t.crow_indices(), t.col_indices() + 2 ** 40, t.values())
    with pytest.raises(ValueError, match="torch tensor"):
        dev.spmm_setup_device(a.indptr, a.indices, a.data)
    with pytest.raises(ValueError, match="do not hold"):
        dev.spmm_setup_device(t.crow_indices(), t.col_indices()[:-1], t.values()[:-1])
    assert same_bits(product(dev, "dla_spmm_matvec", x), ax)
