"""CPU: the checkers of tests/dense_ref.py have teeth, and the case lists of tests/test_dense_sweeps_gpu.py leave them headroom.

HostLib is a float64 numpy emulation of the part of the C-ABI the checkers drive (allocation, transfers and the dense entries of
include/diaglib_amd.h), on host memory, behind the very wrappers of diaglib_amd/capi.py -- so the wrappers' leading dimensions and NULL
pointers are exercised here too.  The exact emulation must pass every checker; each seeded defect must fail with the message of the
check it belongs to.  Headroom: a plain float64 product is the emulation, so running every case list on it holds the inputs to
|float64 product - long-double reference| <= 1.0 x the bound on their own."""
import ctypes as C
import re

import numpy as np
import pytest

import dense_ref as D
import test_dense_sweeps_gpu as G
from diaglib_amd import capi


def dev(ptr, n, m):
    """the n x m column-major block at an address"""
    return np.frombuffer((C.c_double * (n * m)).from_address(int(ptr)), dtype=np.float64).reshape((m, n)).T if n * m else np.zeros((n, m))


def host(p, ld, cols):
    """a host block of leading dimension ld behind a ctypes pointer"""
    return dev(C.cast(p, C.c_void_p).value, ld, cols)


class HostLib:
    """defect: None (exact) or one of DEFECTS"""

    def __init__(self, defect=None):
        self.defect, self.blocks = defect, {}

    # ---- memory
    def dla_alloc(self, h, size, ref):
        buf = np.zeros(int(size) + 64, np.uint8)
        addr = (buf.ctypes.data + 15) // 16 * 16
        self.blocks[addr] = buf
        ref._obj.value = addr
        return 0

    def dla_free(self, h, ptr):
        self.blocks.pop(int(ptr), None)
        return 0

    def dla_upload(self, h, dst, src, size):
        C.memmove(int(dst), int(src), int(size))
        return 0

    dla_download = dla_upload

    def dla_last_error(self, h):
        return b"host emulation"

    # ---- how a block is stored, and the defects of a store
    def store(self, ptr, n, k, new):
        z, d = dev(ptr, n, k), self.defect
        new = np.array(new, dtype=np.float64)
        if d == "last row":
            new[n - 1] = z[n - 1]
        elif d == "last row pair" and n % 2 == 0:
            new[n - 2:] = z[n - 2:]
        elif d == "column":
            new[:, k // 2] = z[:, k // 2]
        elif d == "nan leak":
            new[n - 1, k - 1] += 0.0 * self.neighbour
        z[:] = new
        if d == "sentinel":
            dev(ptr + 8 * n * k, 1, 1)[0, 0] = 0.5

    def coeff(self, p, ld, rows, cols):
        """rows x cols of a host coefficient block; the defect reads it with the row count as leading dimension"""
        if self.defect == "ldc as l":
            return host(p, rows, cols).copy()
        return host(p, ld, cols)[:rows].copy()

    def result(self, p, ld, rows, cols, new):
        if self.defect == "ldc as l":
            ld = rows
        host(p, ld, cols)[:rows] = new

    def read(self, ptr, n, l):
        """an input panel; the defects that touch or leak it"""
        x = dev(ptr, n, l)
        self.neighbour = dev(ptr - 8, 1, 1)[0, 0]                 # the element in front of the block
        val = x.copy()
        if self.defect == "input":
            x[n // 2, 0] += 1.0
        return val

    # ---- the dense entries
    def dla_gram(self, h, n, l, x, k, u, c, ldc):
        self.result(c, ldc, l, k, self.read(x, n, l).T @ self.read(u, n, k))
        return 0

    def dla_gram_lower(self, h, n, l, x, u, c, ldc):
        return self.dla_gram(h, n, l, x, l, u, c, ldc)

    def dla_panel_gemm(self, h, n, l, x, k, c, ldc, z):
        self.store(z, n, k, self.read(x, n, l) @ self.coeff(c, ldc, l, k))
        return 0

    def dla_panel_update(self, h, n, l, x, k, c, ldc, u):
        self.store(u, n, k, dev(u, n, k) - self.read(x, n, l) @ self.coeff(c, ldc, l, k))
        return 0

    def dla_trmm_linvt(self, h, n, k, u, linv, ld):
        lm = self.coeff(linv, ld, k, k)
        self.neighbour = dev(u - 8, 1, 1)[0, 0]
        self.store(u, n, k, dev(u, n, k) @ (lm if self.defect == "upper of linv" else np.tril(lm)).T)
        return 0

    def gram_of(self, u, n, k, g, ldg):
        z = dev(u, n, k)
        low = np.tril(z.T @ z)
        self.result(g, ldg, k, k, low + np.tril(low, -1).T)
        return 0

    def dla_trmm_gram(self, h, n, k, u, w, ldw, g, ldg):
        self.neighbour = dev(u - 8, 1, 1)[0, 0]
        self.store(u, n, k, dev(u, n, k) @ self.coeff(w, ldw, k, k))
        return self.gram_of(u, n, k, g, ldg)

    def dla_update_gram(self, h, n, l, x, k, c, ldc, u, g, ldg):
        self.dla_panel_update(h, n, l, x, k, c, ldc, u)
        return self.gram_of(u, n, k, g, ldg)

    def dla_combo_gram(self, h, n, m, x, k, c, ldc, u, g, ldg):
        assert u == x + 8 * n * m
        self.store(u, n, k, self.read(x, n, m + k) @ self.coeff(c, ldc, m + k, k))
        return self.gram_of(u, n, k, g, ldg)

    def residual(self, n, m, e, t, eig, n_res, skip, rnorm):
        theta = np.ctypeslib.as_array(eig, (m,))
        sk = np.ctypeslib.as_array(skip, (m,))
        r = t.copy()
        rn = np.ctypeslib.as_array(rnorm, (2 * max(1, n_res),))
        done = []
        for j in range(n_res):
            if sk[j] and self.defect != "skipped root corrected":
                continue
            r[:, j] = t[:, j] + theta[j] * e[:, j] if self.defect == "theta sign" else t[:, j] - theta[j] * e[:, j]
            done.append(j)
        return r, rn, done

    def norms(self, ptr, n, m, rn, done):
        r = dev(ptr, n, m)                                         # (of what was stored)
        for j in done:
            rn[2 * j] = np.sqrt(float((D.ld(r[:, j]) ** 2).sum()) / ((n - 1) if self.defect == "rms over n - 1" else n))
            rn[2 * j + 1] = np.abs(r[:, j]).max()

    def dla_ritz_residual(self, h, n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, rnorm):
        yy = self.coeff(y, ldy, l, m)
        e, t = self.read(v, n, l) @ yy, self.read(av, n, l) @ yy
        res, rn, done = self.residual(n, m, e, t, eig, n_res, skip, rnorm)
        if evec:
            self.store(evec, n, m, e)
        self.store(r, n, m, res)
        if avy:
            self.store(avy, n, m, t)
        self.norms(r, n, m, rn, done)
        return 0

    def dla_ritz_residual_p(self, h, n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, rnorm, k2, c2, ldc2, p, ap):
        self.dla_ritz_residual(h, n, l, m, v, av, y, ldy, eig, n_res, skip, evec, r, avy, rnorm)
        if k2 > 0:
            cc = self.coeff(c2, ldc2, l, k2)
            self.store(p, n, k2, dev(v, n, l) @ cc)
            self.store(ap, n, k2, dev(av, n, l) @ cc)
        return 0

    def dla_ritz_residual2(self, h, n, l, m, v, av, y1, ldy1, y2, ldy2, eig, n_res, skip, e, r, tw, jk, rnorm):
        ee, t = self.read(v, n, l) @ self.coeff(y1, ldy1, l, m), self.read(av, n, l) @ self.coeff(y2, ldy2, l, m)
        res, rn, done = self.residual(n, m, ee, t, eig, n_res, skip, rnorm)
        self.store(e, n, m, ee)
        self.store(r, n, m, res)
        self.norms(r, n, m, rn, done)
        return 0


class HostCtx(capi.Context):
    """the wrappers of capi.Context on the emulation"""

    def __init__(self, defect=None):
        self.lib, self.h, self._keep = HostLib(defect), 1, []

    def trim(self):
        return 0

    def reset_stats(self):
        pass


# ------------------------------------------------------------------------------------------------------------------ teeth
N, L, K = 66, 13, 7                      # even n: a last row pair; pad = 3 / gpad = 5: a leading dimension to get wrong
ENTRIES = {
    "gemm": G.call("check_product", N, L, K, "gemm", pad=3), "update": G.call("check_product", N, L, K, "update", pad=3),
    "trmm": G.call("check_product", N, K, K, "trmm", pad=3), "alias": G.call("check_product", N, L, K, "gemm", alias=3, pad=3),
    "trmm_gram": G.call("check_fused", N, K, K, "trmm_gram", pad=3, gpad=5), "update_gram": G.call("check_fused", N, L, K, "update_gram", pad=3, gpad=5),
    "combo_gram": G.call("check_fused", N, L, K, "combo_gram", pad=3, gpad=5), "gram": G.call("check_gram", N, L, K, cpad=4),
    "gram_lower": G.call("check_gram", N, K, K, cpad=4, lower=True),
    "ritz": G.call("check_ritz", N, L, K), "ritz_no_evec": G.call("check_ritz", N, L, K, evec=False, avy=False, n_res=3),
    "ritz_p": G.call("check_ritz", N, L, K, k2=5), "ritz2": G.call("check_ritz2", N, L, K),
}
PURE_OUT = ["gemm", "ritz", "ritz_no_evec", "ritz_p", "ritz2"]                      # outputs prefilled with the sentinel
IN_PLACE = ["update", "trmm", "alias", "trmm_gram", "update_gram", "combo_gram"]
WRITERS = PURE_OUT + IN_PLACE
WITH_INPUT = ["gemm", "update", "update_gram", "combo_gram", "gram", "gram_lower", "ritz", "ritz_no_evec", "ritz_p", "ritz2"]
RITZ = ["ritz", "ritz_no_evec", "ritz_p", "ritz2"]
PREFILL, BOUND = "left at its prefill", r"x the bound"
SENTINEL = "a sentinel column next to the output block was overwritten|a guard column next to a block updated in place was overwritten"
# defect -> [(entries, message of the check that must catch it)]
DEFECTS = {
    "last row": [(PURE_OUT, PREFILL), (IN_PLACE, BOUND)],
    "last row pair": [(PURE_OUT, PREFILL), (IN_PLACE, BOUND)],
    "column": [(PURE_OUT, PREFILL), (IN_PLACE, BOUND)],
    "sentinel": [([e for e in WRITERS if e != "alias"], SENTINEL)],          # (behind an aliased Z lies another column of X)
    "input": [(WITH_INPUT, r"an input block \(or its guard columns\) was modified")],
    "nan leak": [(WRITERS, "non-finite output")],
    "ldc as l": [(WRITERS, "non-finite output"), (["gram", "gram_lower"], "padding rows under C were written|left at its prefill")],
    "upper of linv": [(["trmm"], r"trmm .*" + BOUND)],
    "skipped root corrected": [(RITZ, r" r: .*" + BOUND)],
    "theta sign": [(RITZ, r" r: .*" + BOUND)],
    "rms over n - 1": [(RITZ, "rms norm of root")],
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_exact_emulation_passes(entry):
    G.run(HostCtx(), ENTRIES[entry])


@pytest.mark.parametrize("defect,entry,message", [(d, e, msg) for d, rows in DEFECTS.items() for entries, msg in rows for e in entries])
def test_seeded_defect_is_caught_by_its_check(defect, entry, message):
    with pytest.raises(AssertionError) as err:
        G.run(HostCtx(defect), ENTRIES[entry])
    assert re.search(message, str(err.value), re.S), (defect, entry, str(err.value)[:300])


def test_nan_guard_is_one_fixed_quiet_nan():
    assert np.isnan(D.QNAN) and D.bits(np.array([D.QNAN]))[0] == D.QNAN_BITS and (int(D.QNAN_BITS) >> 51) & 1 == 1
    g = D.NanGuarded(HostCtx(), 5, 2, np.ones((5, 2)), offset=8)
    assert (g.ptr - 8 * 5) % 16 == 8 and np.all(D.bits(g.whole.download()[:, [0, 3]]) == D.QNAN_BITS)
    g.assert_unchanged()
    dev(g.ptr - 8, 1, 1)[0, 0] = np.array([D.QNAN_BITS ^ np.uint64(1)]).view(np.float64)[0]       # another NaN: equal as a float, not as bits
    with pytest.raises(AssertionError, match="was modified"):
        g.assert_unchanged()


# ------------------------------------------------------------------------------------------------------------------ headroom
def every_case():
    """the case lists of tests/test_dense_sweeps_gpu.py, by test (made when asked for: some come from the planner)"""
    lists = {}
    for n in (G.N_EVEN, G.N_ODD):
        for family in G.LADDER_FAMILIES:
            lists[f"ladder {n} {family}"] = lambda n=n, family=family: [c for c, _ in G.ladder_cases(n, family)]
    lists["tails"] = lambda: [c for n in G.TAIL_N for c in G.tail_cases(n)]
    lists["last"] = G.last_cases
    lists["alignment"] = lambda: [c for c, _ in G.alignment_cases()]
    for n, l, m in G.RITZ_NLM:
        for k2 in G.RITZ_K2:
            lists[f"ritz options {n} {l} {m} {k2}"] = lambda n=n, l=l, m=m, k2=k2: [(c, G.seed_of((n, l, m))) for pair in G.ritz_option_cases(n, l, m, k2) for c in pair]
    lists["ritz2 options"] = G.ritz2_cases
    lists["alias"] = lambda: G.alias_cases() + [G.call("check_product", n, l, k, "gemm") for n in (G.N_EVEN, G.N_ODD) for l, k in G.ALIAS_REFUSED]
    lists["leading dimensions"] = lambda: [c for pair in G.ld_cases() for c in pair]
    lists["second trip"] = lambda: [c for c, _, _ in G.second_trip_cases(256)]
    return lists


@pytest.mark.parametrize("which", sorted(every_case()))
def test_float64_products_stay_within_the_bounds(which):
    """the condition on the inputs: numpy's float64 results against the long-double reference, below 1.0 x the bound on every case"""
    ctx = HostCtx()
    for c in every_case()[which]():
        c, seed = c if isinstance(c[1], int) else (c, None)
        res = G.run(ctx, c, seed)
        ratio = res["ratio"] if isinstance(res, dict) else res[-1]
        assert ratio < 1.0, (c, ratio)
