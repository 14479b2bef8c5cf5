"""The dense panel and Ritz sweeps (gemm_kernel, ritz_kernel, ritz2_kernel and the Gram kernels behind dla_gram) against np.longdouble
references written straight from the definitions in include/diaglib_amd.h, with guards around everything that is read or written.

Conventions (those of tests/test_operators_gpu.py, whose Guarded, assert_within, SENT and LD are used here)
  * every OUTPUT block sits between two sentinel columns of 7.0 and is prefilled with 7.0: the sentinels must survive and every entry
    must have been written;
  * every INPUT block sits between two columns of one fixed quiet NaN (NanGuarded): it must come back bit-identical, and no output
    may be non-finite -- a neighbour that is read and multiplied by a zero coefficient shows as a NaN.  A block that is updated in
    place sits between NaN columns too: they guard what is read and what is written;
  * host coefficient blocks may carry padding rows (leading dimension > rows) filled with the same NaN; host results may carry padding
    rows filled with the sentinel, which must stay;
  * bounds are the project's own (tests/test_kernels_gpu.py): 64 eps |X||C| for a product, + 4 eps |U| for an update, the Gram bound
    of test_fused_sweeps_against_their_blas_pairs, b2 + |eig| b1 + 4 eps |r| for a residual, rtol 1e-13 for the rms norm against the
    downloaded r, equality for max |r|.

The checkers are plain functions of (ctx, rng, shape, options): tests/test_dense_sweeps_gpu.py calls them on the HIP context,
tests/test_dense_ref.py on a float64 numpy emulation of the C-ABI (no GPU), tools/fuzz_kernels.py on random shapes.  WORST keeps the
largest |got - ref| / bound seen per family."""
import collections

import numpy as np

from diaglib_amd import capi
from test_operators_gpu import LD, SENT, Guarded, assert_within

EPS = np.finfo(np.float64).eps
TINY = LD(1e-300)
QNAN_BITS = np.uint64(0x7FF8_0000_0000_0D1A)       # one quiet NaN with a payload of its own
QNAN = float(np.array([QNAN_BITS]).view(np.float64)[0])
WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(np.asfortranarray(a)), bits(np.asfortranarray(b)))


# ------------------------------------------------------------------------------------------------------------------ guards
class NanGuarded(Guarded):
    """[NaN | block | NaN] on the device: an input, or a block that is updated in place.  last = True leaves the trailing column
    out: the block is then the last columns of its allocation.  offset as in Guarded."""

    def __init__(self, ctx, n, m, fill, offset=0, last=False):
        Guarded.__init__(self, ctx, n, m - 1 if last else m, None, offset)          # (last: n x (m + 1) in all)
        self.m, self.last = m, last
        self.host[:, 0] = QNAN
        self.host[:, 1:m + 1] = fill
        if not last:
            self.host[:, -1] = QNAN
        self.whole.upload(self.host)

    def body(self):
        """the block (updated in place), after checking that the NaN columns kept their bits"""
        got = self.whole.download()
        edge = [0] if self.last else [0, -1]
        assert np.array_equal(bits(got[:, edge]), bits(self.host[:, edge])), "a guard column next to a block updated in place was overwritten"
        return got[:, 1:self.m + 1]

    def assert_unchanged(self, cols=None):
        """the whole panel bit for bit (cols: only these columns of the block, and the guards)"""
        got, want = self.whole.download(), self.host
        if cols is not None:
            keep = [0] + [1 + j for j in cols] + ([] if self.last else [self.m + 1])
            got, want = got[:, keep], want[:, keep]
        assert np.array_equal(bits(got), bits(want)), "an input block (or its guard columns) was modified"


def view(g, j=0, m=None):
    """columns j .. j + m - 1 of a guarded block as the panel the wrappers take"""
    m = g.m - j if m is None else m
    return capi.DevPanel(g.ctx, g.n, m, ptr=g.ptr + 8 * g.n * j, owner=False)


def padded(a, pad, fill=QNAN):
    """a host block with `pad` extra rows under it (leading dimension = rows + pad)"""
    out = np.full((a.shape[0] + pad, a.shape[1]), fill, order="F")
    out[:a.shape[0]] = a
    return out


def written(got, what):
    assert np.all(np.isfinite(got)), what + ": non-finite output"
    assert not np.any(got == SENT), what + ": an entry of the output block was left at its prefill"
    return got


def free(*blocks):
    for b in blocks:
        if b is not None:
            b.free()


# ------------------------------------------------------------------------------------------------------------------ references
def ld(a):
    return np.asarray(a, dtype=LD)


_PRODUCTS = collections.OrderedDict()


def ref_product(x, c):
    """X C and |X| |C| (read only: the last few are kept, the option crossings repeat their operands)"""
    x, c = np.ascontiguousarray(x), np.ascontiguousarray(c)
    key = (x.shape, c.shape, str(x.dtype), hash(x.tobytes()), hash(c.tobytes()))
    if key not in _PRODUCTS:
        res = ld(x) @ ld(c), np.abs(ld(x)) @ np.abs(ld(c))
        for a in res:
            a.setflags(write=False)
        _PRODUCTS[key] = res
        while len(_PRODUCTS) > 12:
            _PRODUCTS.popitem(last=False)
    return _PRODUCTS[key]


def ref_update(x, c, u):
    """U - X C and |X| |C|"""
    xc, mag = ref_product(x, c)
    return ld(u) - xc, mag


def ref_linvt(u, linv):
    """U Linv^T, reading only the lower triangle of Linv"""
    return ref_product(u, np.tril(linv).T)


def ref_combo(x, u, cp):
    """[X | U] C'"""
    return ref_product(np.hstack([x, u]), cp)


def ref_gram(x, u):
    """X^T U and |X|^T |U|"""
    xt, u = np.ascontiguousarray(ld(x).T), np.asfortranarray(ld(u))      # (both operands of the long-double products run along memory)
    return xt @ u, np.abs(xt) @ np.abs(u)


def ref_ritz(v, av, y, eig, n_res, skip):
    """V Y, AV Y and AV Y - theta o V Y on the open roots among the first n_res; the magnitudes |V||Y|, |AV||Y| and the open roots"""
    ev, m1 = ref_product(v, y)
    avy, m2 = ref_product(av, y)
    return (ev, avy) + ref_residual(ev, avy, eig, n_res, skip) + (m1, m2)


def ref_ritz2(v, av, y1, y2, eig, n_res, skip):
    """the two-coefficient form: e = V Y1, r = AV Y2 - theta o e"""
    e, m1 = ref_product(v, y1)
    t, m2 = ref_product(av, y2)
    return (e, t) + ref_residual(e, t, eig, n_res, skip) + (m1, m2)


def ref_residual(e, t, eig, n_res, skip):
    m = e.shape[1]
    open_ = np.array([j < n_res and not skip[j] for j in range(m)], dtype=bool)
    return t - np.where(open_, ld(eig), LD(0))[None, :] * e, open_


def ref_norms(r):
    """||r_i||_2 / sqrt(n) and max |r_i| of a float64 block"""
    return np.sqrt((ld(r) ** 2).sum(axis=0) / LD(r.shape[0])), np.abs(r).max(axis=0)


def product_bound(mag):
    return {"64 eps |X||C|": 64 * EPS * mag, "tiny": TINY}


def gram_bound_fused(want_u, ubound):
    """the Gram bound of test_fused_sweeps_against_their_blas_pairs: the dot products of the stored block, and what the stored block's
    own error moves them by"""
    a = np.abs(want_u)
    at = np.ascontiguousarray(a.T)                                  # (both operands of the long-double products run along memory)
    return {"64 eps |U|^T|U|": 64 * EPS * (at @ at.T), "2 |U|^T bound": 2 * (at @ np.asfortranarray(ubound)), "tiny": TINY}


def check_norms(rn, r_got, open_, n_res, what):
    rms, mx = ref_norms(r_got)
    for j in range(rn.shape[1]):
        if j < n_res and open_[j]:
            assert abs(LD(rn[0, j]) - rms[j]) <= LD(1e-13) * rms[j], f"{what}: rms norm of root {j}: {rn[0, j]!r} against {float(rms[j])!r} of the stored r"
            assert rn[1, j] == mx[j], f"{what}: max |r| of root {j}: {rn[1, j]!r} against {mx[j]!r} of the stored r"
        else:
            assert rn[0, j] == 0.0 and rn[1, j] == 0.0, f"{what}: the norms of root {j}, which is not open, were touched"


def skip_pattern(m, pattern):
    """ "none", "one", "all", or the flags themselves"""
    if not isinstance(pattern, str):
        return np.ascontiguousarray(pattern, dtype=np.int32)
    skip = np.zeros(m, np.int32)
    if pattern == "one":
        skip[1 % m] = 1
    elif pattern == "all":
        skip[:] = 1
    else:
        assert pattern == "none", pattern
    return skip


def sampled(n, sample):
    """the rows on which a long reference is formed: every 97th and the last 300 (the second trip of a sweep is in these)"""
    if not sample or n <= 600:
        return slice(None)
    return np.union1d(np.arange(0, n, 97), np.arange(n - 300, n))


# ------------------------------------------------------------------------------------------------------------------ checkers
def check_product(ctx, rng, n, l, k, mode, off=None, last=False, pad=0, alias=None, sample=False):
    """mode "gemm": Z = X C, "update": U -= X C, "trmm": U <- U Linv^T (l == k).  off: the one argument 8 bytes off ("x" / "z");
    last: X ends its allocation; pad: extra NaN rows under the coefficient block; alias = j (gemm): Z is columns j .. j+k-1 of X"""
    what = f"{mode} n={n} l={l} k={k} off={off} last={last} pad={pad} alias={alias}"
    rows = sampled(n, sample)
    x = np.asfortranarray(rng.standard_normal((n, l)))
    if mode == "trmm":
        assert l == k
        linv = np.tril(rng.standard_normal((k, k))) + 3 * np.eye(k)
        dirty = padded(linv + np.triu(rng.standard_normal((k, k)), 1), pad)          # the strict upper part must be ignored
        gu = NanGuarded(ctx, n, k, x, offset=8 if off else 0, last=last)
        ctx.trmm_linvt(view(gu), dirty)
        got = written(gu.body(), what)
        ref, mag = ref_linvt(x[rows], linv)
        ratio = note("trmm_linvt", assert_within(got[rows], ref, product_bound(mag), what))
        free(gu)
        return got, ratio
    c = np.asfortranarray(rng.standard_normal((l, k)))
    if alias is not None:
        assert mode == "gemm"
        gx = NanGuarded(ctx, n, l, x, offset=8 if off else 0, last=last)
        ctx.panel_gemm(view(gx), padded(c, pad), view(gx, alias, k))
        got = written(gx.body()[:, alias:alias + k], what)
        gx.assert_unchanged(cols=[j for j in range(l) if not alias <= j < alias + k])
        ref, mag = ref_product(x[rows], c)                                             # (of the ORIGINAL X)
        ratio = note("panel_gemm", assert_within(got[rows], ref, product_bound(mag), what))
        free(gx)
        return got, ratio
    gx = NanGuarded(ctx, n, l, x, offset=8 if off == "x" else 0, last=last)
    if mode == "gemm":
        gz = Guarded(ctx, n, k, offset=8 if off == "z" else 0)
        ctx.panel_gemm(view(gx), padded(c, pad), view(gz))
        got = gz.body()
        gx.assert_unchanged()
        written(got, what)
        ref, mag = ref_product(x[rows], c)
        ratio = note("panel_gemm", assert_within(got[rows], ref, product_bound(mag), what))
    else:
        assert mode == "update", mode
        u = np.asfortranarray(rng.standard_normal((n, k)))
        gz = NanGuarded(ctx, n, k, u, offset=8 if off == "z" else 0)
        ctx.panel_update(view(gx), padded(c, pad), view(gz))
        got = gz.body()
        gx.assert_unchanged()
        written(got, what)
        ref, mag = ref_update(x[rows], c, u[rows])
        ratio = note("panel_update", assert_within(got[rows], ref, dict(product_bound(mag), **{"4 eps |U|": 4 * EPS * np.abs(u[rows])}), what))
    free(gx, gz)
    return got, ratio


def check_fused(ctx, rng, n, l, k, which, off=None, last=False, pad=0, gpad=0):
    """which "trmm_gram": U <- U W (general W; l is ignored), "update_gram": U -= X C, "combo_gram": U <- [X | U] C' with U behind X
    in one panel; each with G = U^T U of the result.  gpad: extra sentinel rows under G"""
    what = f"{which} n={n} l={l} k={k} off={off} last={last} pad={pad} gpad={gpad}"
    g = np.full((k + gpad, k), SENT, order="F")
    u = np.asfortranarray(rng.standard_normal((n, k)))
    gx = None
    if which == "trmm_gram":
        w = rng.standard_normal((k, k)) + 2 * np.eye(k)
        gu = NanGuarded(ctx, n, k, u, offset=8 if off else 0, last=last)
        ctx.trmm_gram(view(gu), padded(w, pad), out=g)
        got = gu.body()
        ref, mag = ref_product(u, w)
        terms = product_bound(mag)
    elif which == "update_gram":
        x = np.asfortranarray(rng.standard_normal((n, l)))
        c = rng.standard_normal((l, k)) * 0.1
        gx = NanGuarded(ctx, n, l, x, offset=8 if off == "x" else 0, last=last)
        gu = NanGuarded(ctx, n, k, u, offset=8 if off == "z" else 0)
        ctx.update_gram(view(gx), padded(c, pad), view(gu), out=g)
        got = gu.body()
        gx.assert_unchanged()
        ref, mag = ref_update(x, c, u)
        terms = dict(product_bound(mag), **{"4 eps |U|": 4 * EPS * np.abs(u)})
    else:
        assert which == "combo_gram", which
        x = np.asfortranarray(rng.standard_normal((n, l)))
        cp = np.vstack([rng.standard_normal((l, k)) * 0.1, rng.standard_normal((k, k)) + 2 * np.eye(k)])
        gu = NanGuarded(ctx, n, l + k, np.hstack([x, u]), offset=8 if off else 0, last=last)
        ctx.combo_gram(view(gu, 0, l), padded(cp, pad), view(gu, l, k), out=g)
        got = gu.body()[:, l:]
        gu.assert_unchanged(cols=range(l))                                               # X untouched
        ref, mag = ref_combo(x, u, cp)
        terms = product_bound(mag)
    written(got, what)
    ratio = note(which, assert_within(got, ref, terms, what))
    assert np.all(g[k:] == SENT), what + ": the padding rows under G were written"
    gg = written(g[:k], what + " G")
    assert np.array_equal(gg, gg.T), what + ": G is not symmetric"
    gterms = gram_bound_fused(ref, sum(terms.values()))
    gref = np.ascontiguousarray(ref.T) @ np.asfortranarray(ref)
    gratio = note(which + " G", assert_within(gg, gref, gterms, what + " G"))
    free(gx, gu)
    return got, gg, max(ratio, gratio)


def check_gram(ctx, rng, n, l, k, off=None, last=False, cpad=0, lower=False):
    """dla_gram (lower: dla_gram_lower, k == l, the lower triangle is checked); cpad: extra sentinel rows under C"""
    what = f"gram n={n} l={l} k={k} off={off} cpad={cpad} lower={lower}"
    x, u = np.asfortranarray(rng.standard_normal((n, l))), np.asfortranarray(rng.standard_normal((n, k)))
    gx = NanGuarded(ctx, n, l, x, offset=8 if off == "x" else 0, last=last)
    gu = NanGuarded(ctx, n, k, u, offset=8 if off == "u" else 0)
    c = np.full((l + cpad, k), SENT, order="F")
    (ctx.gram_lower if lower else ctx.gram)(view(gx), view(gu), out=c)
    gx.assert_unchanged(); gu.assert_unchanged()
    assert np.all(c[l:] == SENT), what + ": the padding rows under C were written"
    got = written(c[:l], what)
    ref, mag = ref_gram(x, u)
    terms = {"64 eps |X|^T|U|": 64 * EPS * mag, "tiny": TINY}
    if lower:
        low = np.tril(np.ones((l, l), bool))
        ratio = assert_within(got[low], ref[low], {key: (v if np.ndim(v) == 0 else v[low]) for key, v in terms.items()}, what)
    else:
        ratio = assert_within(got, ref, terms, what)
    note("gram", ratio)
    free(gx, gu)
    return got, ratio


def check_ritz(ctx, rng, n, l, m, evec=True, avy=True, n_res=None, skip="one", k2=None, off=None, last=False, ypad=3, sample=False):
    """dla_ritz_residual (k2 = None) / dla_ritz_residual_p (k2 >= 0 extra products).  evec / avy = False: NULL; off: the one pointer
    8 bytes off ("v", "av", "evec", "r", "avy", "p", "ap"); ypad: NaN rows under Y (and C2).  Returns what was stored"""
    what = f"ritz n={n} l={l} m={m} evec={evec} avy={avy} n_res={n_res} skip={skip} k2={k2} off={off} last={last}"
    rows = sampled(n, sample)
    n_res = m if n_res is None else n_res
    v, av = np.asfortranarray(rng.standard_normal((n, l))), np.asfortranarray(rng.standard_normal((n, l)))
    y, eig = rng.standard_normal((l, m)), rng.standard_normal(m)
    c2 = rng.standard_normal((l, k2 or 0))
    sk = skip_pattern(m, skip)
    o8 = lambda name: 8 if off == name else 0  # noqa: E731
    gv, gav = NanGuarded(ctx, n, l, v, offset=o8("v"), last=last), NanGuarded(ctx, n, l, av, offset=o8("av"), last=last)
    ge = Guarded(ctx, n, m, offset=o8("evec")) if evec else None
    gr = Guarded(ctx, n, m, offset=o8("r"))
    ga = Guarded(ctx, n, m, offset=o8("avy")) if avy else None
    gp = gap = None
    if k2 is None:
        rn = ctx.ritz_residual(view(gv), view(gav), padded(y, ypad), eig, n_res, sk, view(ge) if evec else None, view(gr),
                               view(ga) if avy else None, m=m)
    else:
        gp, gap = Guarded(ctx, n, max(k2, 1), offset=o8("p")), Guarded(ctx, n, max(k2, 1), offset=o8("ap"))
        rn = ctx.ritz_residual_p(view(gv), view(gav), padded(y, ypad), eig, n_res, sk, view(ge) if evec else None, view(gr),
                                 view(ga) if avy else None, padded(c2, ypad) if k2 else c2, view(gp), view(gap), m=m)
    out = {"rn": rn, "r": gr.body(), "evec": ge.body() if evec else None, "avy": ga.body() if avy else None,
           "p": gp.body() if gp else None, "ap": gap.body() if gap else None}
    gv.assert_unchanged(); gav.assert_unchanged()
    ev_ref, avy_ref, r_ref, open_, m1, m2 = ref_ritz(v[rows], av[rows], y, eig, n_res, sk)
    b1, b2 = 64 * EPS * m1, 64 * EPS * m2
    ratio = 0.0
    if evec:
        ratio = max(ratio, note("ritz evec", assert_within(written(out["evec"], what + " evec")[rows], ev_ref, {"b1": b1, "tiny": TINY}, what + " evec")))
    if avy:
        ratio = max(ratio, note("ritz avy", assert_within(written(out["avy"], what + " avy")[rows], avy_ref, {"b2": b2, "tiny": TINY}, what + " avy")))
    terms = {"b2": b2, "|eig| b1": np.where(open_, np.abs(eig), 0.0)[None, :] * b1, "4 eps |r|": 4 * EPS * np.abs(r_ref), "tiny": TINY}
    ratio = max(ratio, note("ritz r", assert_within(written(out["r"], what + " r")[rows], r_ref, terms, what + " r")))
    check_norms(rn, out["r"], open_, n_res, what)
    if k2:
        pref, pm = ref_product(v[rows], c2)
        apref, apm = ref_product(av[rows], c2)
        ratio = max(ratio, note("ritz p", assert_within(written(out["p"], what + " p")[rows], pref, product_bound(pm), what + " p")))
        ratio = max(ratio, note("ritz p", assert_within(written(out["ap"], what + " ap")[rows], apref, product_bound(apm), what + " ap")))
    elif k2 == 0:
        assert np.all(out["p"] == SENT) and np.all(out["ap"] == SENT), what + ": k2 = 0 but the extra blocks were written"
    free(gv, gav, ge, gr, ga, gp, gap)
    out["ratio"] = ratio
    return out


def check_ritz2(ctx, rng, n, l, m, n_res=None, skip="one", off=None, last=False, ypad=3):
    """dla_ritz_residual2: e = V Y1, r = AV Y2 - theta o e and the norms of r; off: "v", "av", "e" or "r" """
    what = f"ritz2 n={n} l={l} m={m} n_res={n_res} skip={skip} off={off} last={last}"
    n_res = m if n_res is None else n_res
    v, av = np.asfortranarray(rng.standard_normal((n, l))), np.asfortranarray(rng.standard_normal((n, l)))
    y1, y2, eig = rng.standard_normal((l, m)), rng.standard_normal((l, m)), rng.standard_normal(m)
    sk = skip_pattern(m, skip)
    o8 = lambda name: 8 if off == name else 0  # noqa: E731
    gv, gav = NanGuarded(ctx, n, l, v, offset=o8("v"), last=last), NanGuarded(ctx, n, l, av, offset=o8("av"), last=last)
    ge, gr = Guarded(ctx, n, m, offset=o8("e")), Guarded(ctx, n, m, offset=o8("r"))
    rn = ctx.ritz_residual2(view(gv), view(gav), padded(y1, ypad), padded(y2, ypad + 1), eig, n_res, sk, view(ge), view(gr))
    out = {"rn": rn, "e": ge.body(), "r": gr.body()}
    gv.assert_unchanged(); gav.assert_unchanged()
    e_ref, _, r_ref, open_, m1, m2 = ref_ritz2(v, av, y1, y2, eig, n_res, sk)
    b1, b2 = 64 * EPS * m1, 64 * EPS * m2
    ratio = note("ritz2 e", assert_within(written(out["e"], what + " e"), e_ref, {"b1": b1, "tiny": TINY}, what + " e"))
    terms = {"b2": b2, "|eig| b1": np.where(open_, np.abs(eig), 0.0)[None, :] * b1, "4 eps |r|": 4 * EPS * np.abs(r_ref), "tiny": TINY}
    ratio = max(ratio, note("ritz2 r", assert_within(written(out["r"], what + " r"), r_ref, terms, what + " r")))
    check_norms(rn, out["r"], open_, n_res, what)
    free(gv, gav, ge, gr)
    out["ratio"] = ratio
    return out
