"""GPU: the dense panel and Ritz sweeps kernel by kernel -- gemm_kernel (dla_panel_gemm, dla_panel_update, dla_trmm_linvt and the fused
dla_trmm_gram, dla_update_gram, dla_combo_gram), ritz_kernel (dla_ritz_residual, dla_ritz_residual_p), ritz2_kernel
(dla_ritz_residual2) and dla_gram's alignment dispatch and leading dimensions -- through the guarded checkers of tests/dense_ref.py:
long-double references, sentinel columns around every output, NaN columns around every input.

  a. the gemm_kernel ladder (launch_gemm over GEMM_INSTANCES of hip_plans.h): every call a small request can reach without
     knobs is made once and must book the name(s) the CPU planner (tests/plans_driver.cpp) prints for the request line(s) of that shape;
     the names of the grid are all the planner gives on an exhaustive walk of the requests a dense entry can make (k <= 48)
  b. tails: n = 1 .. 257 around every wave-tile and block boundary, for every writer
  c. guards: in every call of this file; once per family the input panel also ENDS its allocation
  d. alignment: each pointer argument in turn is the only one 8 bytes off a 16-byte boundary on even n -- the VEC = 1 instance
  e. the Ritz options: evec_dev == NULL, avy_dev == NULL, n_res = 0 / 1 / m, no / one / all roots skipped, ldy > l
  f. dla_panel_gemm with Z a column block of X, at the documented edge and beyond it
  g. leading dimensions larger than the row count, for every host block
  h. the grid-stride second trip of gemm_kernel and ritz_kernel

The case lists are module-level data (tests/test_dense_ref.py runs the same lists on a float64 emulation: the inputs' own headroom).
Nothing here forces a failure path: the misaligned cases take a dispatch the engine already makes."""
import collections
import re
import zlib

import numpy as np
import pytest

import dense_ref as D
from diaglib_amd import capi
from test_plans import env_line, run_plans

pytestmark = pytest.mark.gpu
N_EVEN, N_ODD = 1000, 999
GEMM, RITZ, RITZ2, GRAM = r"gemm_kernel<", r"ritz_kernel<", r"ritz2_kernel<", r"(gram_lds_kernel|gram_kernel)<"


# ------------------------------------------------------------------------------------------------------------------ plumbing
def call(fn, *shape, **opts):
    """one checker call: (name of the checker in dense_ref, shape, options)"""
    return (fn, shape, tuple(sorted(opts.items())))


def seed_of(c, salt=0):
    return zlib.crc32(repr((c, salt)).encode())


def run(ctx, c, seed=None):
    fn, shape, opts = c
    return getattr(D, fn)(ctx, np.random.default_rng(seed_of(c) if seed is None else seed), *shape, **dict(opts))


def plans(lines, ncu=None):
    """(fields, name) of each request line under the default knobs"""
    return run_plans([env_line(ncu=ncu) if ncu else env_line()] + list(lines))[0]


def names_of(lines):
    return [name for _, name in plans(lines)]


def booked(ctx, family):
    """launches per booked kernel name of one family since the last reset_stats"""
    return {name: st["launches"] for name, st in ctx.kernel_stats().items() if st["launches"] > 0 and re.match(family, name)}


def run_booked(ctx, c, family, lines, seed=None):
    """run one call and hold the names it books against the planner's for `lines`"""
    ctx.reset_stats()
    res = run(ctx, c, seed)
    got, want = booked(ctx, family), dict(collections.Counter(names_of(lines)))
    assert got == want, (c, lines, got, want)
    return res, set(got)


def gemm_line(n, l, k, mode, fuse, vec2):
    return f"gemm {n} {l} {k} {mode} {fuse} 0 {vec2}"


# ------------------------------------------------------------------------------------------------------------------ a. the ladder
LADDER_K = [5, 13, 16, 17, 20, 21, 24, 25, 32, 33, 37, 40, 41, 48]      # kt = 1 .. 3, both quarter-tile counts in both positions
LADDER_L = [1, 3, 4, 13, 16, 17, 63, 111]                               # l4 <= 16 at kt = 1 travels in the kernel arguments
# l > the 64 KiB LDS chunk of kt tiles: mode 3 on the second chunk -- in the kernel arguments, packed, and with the quarter tiles of k = 20, 24, 36, 40
LADDER_CHUNKED = [(516, 13), (260, 29), (172, 45), (532, 13), (260, 20), (260, 24), (172, 36), (172, 40)]
LADDER_FAMILIES = ["gemm", "update", "trmm", "chunked", "combo_gram", "update_gram", "trmm_gram", "per_cu"]


def chunk_rows(k):
    """rows of C per LDS chunk (gemm_cols of hip_engine.hip: 64 KiB of 16-column tiles, a multiple of 4)"""
    return (65536 // (8 * 16 * ((k + 15) // 16))) // 4 * 4


def fused_rows(k):
    """the deepest contraction the one-sweep fused kernels take (update_gram_once, can_combo: C and three spare rows in 64 KiB)"""
    return 65536 // (8 * 16 * ((k + 15) // 16)) - 3


def per_cu_shapes(n, vec2):
    """the fused three-tile sweeps (k = 36, 40: one and two quarter tiles; k = 48: none) at the shallowest contraction whose LDS leaves
    two blocks per CU and at the shallowest whose LDS does not (row groups 1 and 2 on the 16-byte path), from the planner:
    [(entry, l, k)] -- l is X's width, the contraction of dla_combo_gram is l + k"""
    out = []
    for k in (36, 40, 48):
        for which, mode in (("update_gram", 1), ("combo_gram", 0)):
            depth = list(range(k + 1, fused_rows(k) + 1))
            res = plans([gemm_line(n, d, k, mode, 1, vec2) for d in depth])
            two = next(d for d, (f, _) in zip(depth, res) if f["per_cu"] >= 2)
            one = next(d for d, (f, _) in zip(depth, res) if f["per_cu"] < 2)
            if vec2:
                assert {f["rtp"] for (f, _), d in zip(res, depth) if d in (two, one)} == {1, 2}
            out += [(which, d - (k if mode == 0 else 0), k) for d in (two, one)]
    return out


def reachable_lines(n):
    """every request a dense entry can make of gemm_kernel without knobs, k <= 48: one chunk of a plain product (modes 0, 1, and 3 for
    a later chunk), the triangular update (mode 2, l = k) and the three fused sweeps within the depth they take"""
    v = 1 - n % 2
    lines = []
    for k in range(1, 49):
        for l in range(1, chunk_rows(k) + 1):
            lines += [gemm_line(n, l, k, mode, 0, v) for mode in (0, 1, 3)]
            if l <= fused_rows(k):
                lines += [gemm_line(n, l, k, 1, 1, v)] + ([gemm_line(n, l, k, 0, 1, v)] if l > k else [])
        lines += [gemm_line(n, k, k, 2, 0, v), gemm_line(n, k, k, 2, 1, v)]
    return lines


def ladder_cases(n, family):
    """[(call, planner lines)] of one family of the ladder"""
    v = 1 - n % 2
    if family in ("gemm", "update"):
        mode = 0 if family == "gemm" else 1
        return [(call("check_product", n, l, k, family), [gemm_line(n, l, k, mode, 0, v)]) for k in LADDER_K for l in LADDER_L]
    if family == "trmm":
        return [(call("check_product", n, k, k, "trmm"), [gemm_line(n, k, k, 2, 0, v)]) for k in LADDER_K]
    if family == "chunked":
        return [(call("check_product", n, l, k, "gemm"), [gemm_line(n, chunk_rows(k), k, 0, 0, v), gemm_line(n, l - chunk_rows(k), k, 3, 0, v)])
                for l, k in LADDER_CHUNKED]
    if family == "combo_gram":
        return [(call("check_fused", n, l, k, family), [gemm_line(n, l + k, k, 0, 1, v)]) for k in LADDER_K for l in LADDER_L]
    if family == "update_gram":
        return [(call("check_fused", n, l, k, family), [gemm_line(n, l, k, 1, 1, v)]) for k in LADDER_K for l in LADDER_L]
    if family == "trmm_gram":
        return [(call("check_fused", n, k, k, family), [gemm_line(n, k, k, 2, 1, v)]) for k in LADDER_K]
    assert family == "per_cu", family
    return [(call("check_fused", n, l, k, which), [gemm_line(n, l + (k if which == "combo_gram" else 0), k, 0 if which == "combo_gram" else 1, 1, v)])
            for which, l, k in per_cu_shapes(n, v)]


_seen = collections.defaultdict(set)


@pytest.mark.parametrize("family", LADDER_FAMILIES)
@pytest.mark.parametrize("n", [N_EVEN, N_ODD])
def test_gemm_ladder_books_the_planned_instance(ctx, n, family):
    """every (l, k) of the grid: the booked gemm_kernel instance(s) are the planner's, the numbers meet the long-double bounds"""
    cases = ladder_cases(n, family)
    want = names_of([ln for _, lines in cases for ln in lines])
    at = 0
    for c, lines in cases:
        ctx.reset_stats()
        run(ctx, c)
        got = booked(ctx, GEMM)
        assert got == dict(collections.Counter(want[at:at + len(lines)])), (c, lines, got, want[at:at + len(lines)])
        at += len(lines)
        _seen[n] |= set(got)
    print(n, family, sorted(set(want)))


@pytest.mark.parametrize("n", [N_EVEN, N_ODD])
def test_gemm_ladder_is_covered(ctx, n):
    """the instances seen by test_gemm_ladder_books_the_planned_instance are all the planner can name over the grid, and the grid's
    are all it can name for any request of a dense entry: no instance of launch_gemm that a request without knobs reaches
    is left out"""
    want = set()
    for family in LADDER_FAMILIES:
        cases = ladder_cases(n, family)
        names = iter(names_of([ln for _, lines in cases for ln in lines]))
        for c, lines in cases:
            mine = {next(names) for _ in lines}
            want |= mine
            if not mine <= _seen[n]:                  # (this test run on its own: one call per name not seen yet)
                _seen[n] |= run_booked(ctx, c, GEMM, lines)[1]
    print(n, len(want), "gemm_kernel instances:", sorted(_seen[n]))
    reachable = set(names_of(reachable_lines(n)))
    assert want == reachable, (sorted(reachable - want), sorted(want - reachable))
    assert _seen[n] == want, (sorted(want - _seen[n]), sorted(_seen[n] - want))
    vec = {re.match(r"gemm_kernel<\d, (\d),", name).group(1) for name in want}
    assert vec == ({"2"} if n % 2 == 0 else {"1"}), vec


# ------------------------------------------------------------------------------------------------------------------ b. tails
TAIL_N = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
TAIL_LK = [(13, 13), (26, 21), (63, 37), (5, 48)]


def tail_cases(n):
    out = []
    for l, k in TAIL_LK:
        out += [call("check_product", n, l, k, "gemm"), call("check_product", n, l, k, "update"), call("check_product", n, k, k, "trmm"),
                call("check_fused", n, k, k, "trmm_gram"), call("check_fused", n, l, k, "update_gram"), call("check_fused", n, l, k, "combo_gram"),
                call("check_ritz", n, l, k), call("check_ritz2", n, l, k)]
    return out


@pytest.mark.parametrize("n", TAIL_N)
def test_tails_of_every_writer(ctx, n):
    """fewer rows than one row pair, one wave tile (16 VEC RTP rows) and one block (four wave tiles), and every boundary's neighbours"""
    for c in tail_cases(n):
        run(ctx, c)


# ------------------------------------------------------------------------------------------------------------------ c. the panel ends its allocation
LAST_NLK = [(N_EVEN, 13, 17), (N_EVEN, 26, 33), (N_ODD, 63, 1)]         # l = 1, 2, 3 (mod 4), k = 1 (mod 16)


def last_cases():
    out = []
    for n, l, k in LAST_NLK:
        out += [call("check_product", n, l, k, "gemm", last=True), call("check_product", n, l, k, "update", last=True),
                call("check_product", n, k, k, "trmm", last=True), call("check_fused", n, k, k, "trmm_gram", last=True),
                call("check_fused", n, l, k, "update_gram", last=True), call("check_fused", n, l, k, "combo_gram", last=True),
                call("check_ritz", n, l, k, last=True), call("check_ritz", n, l, k, k2=5, last=True), call("check_ritz2", n, l, k, last=True),
                call("check_gram", n, l, k, last=True)]
    return out


def test_input_panel_is_the_last_columns_of_its_allocation(ctx):
    """nothing behind the last column is read (the l4 round-up of the column steps clamps to column l - 1), and the in-place entries
    change their own block only"""
    for c in last_cases():
        run(ctx, c)


# ------------------------------------------------------------------------------------------------------------------ d. alignment
AL_L, AL_K, AL_M, AL_K2 = 26, 21, 21, 5


def alignment_cases():
    """[(call, {family of names: (planner lines, VEC)})]: off = None is the aligned call (VEC = 2), every other one has exactly one
    pointer 8 bytes off.  A Ritz sweep with extra products that cannot take the 16-byte path goes through the plain Ritz sweep and two
    panel products: each of the three then goes by the pointers it touches itself"""
    n, l, k, m, k2 = N_EVEN, AL_L, AL_K, AL_M, AL_K2
    out = []
    for off in (None, "x", "z"):
        v = 0 if off else 1
        out += [(call("check_product", n, l, k, "gemm", off=off), {GEMM: ([gemm_line(n, l, k, 0, 0, v)], v)}),
                (call("check_product", n, l, k, "update", off=off), {GEMM: ([gemm_line(n, l, k, 1, 0, v)], v)}),
                (call("check_fused", n, l, k, "update_gram", off=off), {GEMM: ([gemm_line(n, l, k, 1, 1, v)], v)})]
    for off in (None, "x"):
        v = 0 if off else 1
        out += [(call("check_product", n, k, k, "trmm", off=off), {GEMM: ([gemm_line(n, k, k, 2, 0, v)], v)}),
                (call("check_fused", n, k, k, "trmm_gram", off=off), {GEMM: ([gemm_line(n, k, k, 2, 1, v)], v)}),
                (call("check_fused", n, l, k, "combo_gram", off=off), {GEMM: ([gemm_line(n, l + k, k, 0, 1, v)], v)})]
    for off in (None, "x", "u"):
        out.append((call("check_gram", n, l, 13, off=off), {GRAM: ([f"gram {n} {l} 13 0 {0 if off else 1} 0"], None)}))
    for off in (None, "v", "av", "evec", "r", "avy"):
        v = 0 if off else 1
        out.append((call("check_ritz", n, 64, m, off=off), {RITZ: ([f"ritz {n} 64 {m} 0 {v} 1"], v)}))
    for evec, avy in ((False, True), (True, False), (False, False)):               # NULL pointers count as aligned
        out.append((call("check_ritz", n, 64, m, evec=evec, avy=avy), {RITZ: ([f"ritz {n} 64 {m} 0 1 1"], 1)}))
    out.append((call("check_ritz", n, 64, m, k2=k2), {RITZ: ([f"ritz {n} 64 {m} {k2} 1 1"], 1), GEMM: ([], None)}))
    out.append((call("check_ritz", n, 64, m, k2=k2, evec=False, avy=False), {RITZ: ([f"ritz {n} 64 {m} {k2} 1 1"], 1), GEMM: ([], None)}))
    for off in ("v", "av", "evec", "r", "avy", "p", "ap"):
        vr, vp, vap = int(off in ("p", "ap")), int(off not in ("v", "p")), int(off not in ("av", "ap"))
        out.append((call("check_ritz", n, 64, m, k2=k2, off=off),
                    {RITZ: ([f"ritz {n} 64 {m} 0 {vr} 1"], vr), GEMM: ([gemm_line(n, 64, k2, 0, 0, vp), gemm_line(n, 64, k2, 0, 0, vap)], None)}))
    for off in (None, "v", "av", "e", "r"):
        v = 0 if off else 1
        out.append((call("check_ritz2", n, 64, m, off=off), {RITZ2: ([f"ritz2 {n} 64 {m} {v} 1"], v)}))
    return out


def test_one_pointer_off_alignment_takes_the_scalar_instance(ctx):
    """even n, one panel 8 bytes off a 16-byte boundary: the booked instance is the planner's for vec2 = 0 (VEC = 1; dla_gram: the
    kernel of aligned = 0), the results meet the same bounds; with every pointer aligned it is the VEC = 2 instance"""
    for c, families in alignment_cases():
        ctx.reset_stats()
        run(ctx, c)
        for family, (lines, vec2) in families.items():
            got, want = booked(ctx, family), dict(collections.Counter(names_of(lines)))
            assert got == want, (c, lines, got, want)
            for name in got:
                assert vec2 is None or re.match(r"\w+<\d, (\d)[,>]", name).group(1) == ("2" if vec2 else "1"), (c, name)
            print(c[0], c[1], dict(c[2]).get("off"), sorted(got))


# ------------------------------------------------------------------------------------------------------------------ e. the Ritz options
RITZ_NLM = [(N_EVEN, 64, 8), (N_ODD, 64, 21), (N_EVEN, 111, 37), (N_EVEN, 26, 48)]
RITZ_K2 = [None, 0, 5]                                                   # dla_ritz_residual, dla_ritz_residual_p without and with extra products


def ritz_option_cases(n, l, m, k2):
    """[(the call with evec, the same call with evec_dev == NULL)]"""
    return [(call("check_ritz", n, l, m, k2=k2, avy=avy, n_res=n_res, skip=skip), call("check_ritz", n, l, m, k2=k2, avy=avy, n_res=n_res, skip=skip, evec=False))
            for avy in (True, False) for n_res in (0, 1, m) for skip in ("none", "one", "all")]


@pytest.mark.parametrize("k2", RITZ_K2)
@pytest.mark.parametrize("n,l,m", RITZ_NLM)
def test_ritz_options(ctx, n, l, m, k2):
    """evec x avy x n_res x skip with ldy = l + 3 and NaN under Y; without evec the sweep stores the same bits and leaves the same norms"""
    seed = seed_of((n, l, m))
    for with_e, without_e in ritz_option_cases(n, l, m, k2):
        a, b = run(ctx, with_e, seed), run(ctx, without_e, seed)
        assert b["evec"] is None and a["evec"] is not None
        for key in ("r", "avy", "rn", "p", "ap"):
            assert (a[key] is None and b[key] is None) or D.same_bits(a[key], b[key]), (with_e, key)


RITZ2_M = [8, 21, 48, 52]                                                # m = 52: the three-sweep default through t_work / junk


def ritz2_cases():
    return [call("check_ritz2", n, 64, m, n_res=n_res, skip=skip) for n in (N_EVEN, N_ODD) for m in RITZ2_M
            for n_res, skip in ((m, "one"), (m - 2, "none"), (0, "none"), (m, "all"))]


def test_ritz2_options(ctx):
    for c in ritz2_cases():
        run(ctx, c)


# ------------------------------------------------------------------------------------------------------------------ f. aliasing
ALIAS_LK = [(512, 13), (256, 29), (168, 45), (64, 21)]                   # k <= 48 and 128 l ceil(k / 16) <= 65536, the first three at equality
ALIAS_REFUSED = [(516, 13), (260, 29)]


def alias_cases():
    return [call("check_product", n, l, k, "gemm", alias=j) for n in (N_EVEN, N_ODD) for l, k in ALIAS_LK for j in (0, l - k)]


def test_panel_gemm_into_a_column_block_of_x(ctx):
    """include/diaglib_amd.h: 'Z may be a column block of X itself when k <= 48 and 128*l*ceil(k/16) <= 65536' -- the result is that
    of the ORIGINAL X, the other columns keep their bits"""
    for c in alias_cases():
        run(ctx, c)


@pytest.mark.parametrize("l,k", ALIAS_REFUSED)
def test_panel_gemm_refuses_aliasing_beyond_one_lds_chunk(ctx, l, k):
    for n in (N_EVEN, N_ODD):
        rng = np.random.default_rng(seed_of((n, l, k)))
        x, c = rng.standard_normal((n, l)), rng.standard_normal((l, k))
        gx = D.NanGuarded(ctx, n, l, x)
        with pytest.raises(capi.DlaError, match="output aliases the input panel but the contraction needs several LDS chunks"):
            ctx.panel_gemm(D.view(gx), c, D.view(gx, l - k, k))
        gx.assert_unchanged()
        gx.free()
        run(ctx, call("check_product", n, l, k, "gemm"))                 # the same shape without aliasing


# ------------------------------------------------------------------------------------------------------------------ g. leading dimensions
LD_LK = [(13, 13), (63, 37)]                                             # l4 <= 16 at k <= 16: the in-argument path; the packed path


def ld_cases():
    """[(the minimal-ld call, the padded call)]: ldc = l + 3, ldw = k + 2, ldg = k + 5, dla_gram's ldc = l + 4"""
    out = []
    for n in (N_EVEN, N_ODD):
        for l, k in LD_LK:
            out += [(call("check_product", n, l, k, "gemm"), call("check_product", n, l, k, "gemm", pad=3)),
                    (call("check_product", n, l, k, "update"), call("check_product", n, l, k, "update", pad=3)),
                    (call("check_product", n, k, k, "trmm"), call("check_product", n, k, k, "trmm", pad=2)),
                    (call("check_fused", n, k, k, "trmm_gram"), call("check_fused", n, k, k, "trmm_gram", pad=2, gpad=5)),
                    (call("check_fused", n, l, k, "update_gram"), call("check_fused", n, l, k, "update_gram", pad=3, gpad=5)),
                    (call("check_fused", n, l, k, "combo_gram"), call("check_fused", n, l, k, "combo_gram", pad=3, gpad=5)),
                    (call("check_gram", n, l, k), call("check_gram", n, l, k, cpad=4)),
                    (call("check_gram", n, k, k, lower=True), call("check_gram", n, k, k, lower=True, cpad=4))]
    return out


def test_leading_dimensions_beyond_the_row_count(ctx):
    """NaN in the padding rows of the coefficient blocks, the sentinel in those of the results: nothing of the padding is read or
    written, and every stored bit is that of the minimal-ld call"""
    for tight, wide in ld_cases():
        seed = seed_of(tight)
        a, b = run(ctx, tight, seed), run(ctx, wide, seed)
        for p, q in zip(a[:-1], b[:-1]):
            assert D.same_bits(p, q), (wide,)


# ------------------------------------------------------------------------------------------------------------------ h. second trip
def second_trip_cases(ncu):
    """[(call, request line at the chosen n)]: the smallest even n whose row tiles exceed four times the blocks the launch is capped
    at on ncu compute units, for the narrowest shape of the plain one-tile product, the fused three-tile sweep and the Ritz sweep
    (whose grid takes two trips from five row tiles on -- the tails have those -- and is past its cap here as well)"""
    probes = [("gemm {n} 13 13 0 0 0 1", "check_product", (13, 13, "gemm"), {"sample": True}), ("gemm {n} 33 33 2 1 0 1", "check_fused", (33, 33, "trmm_gram"), {}),
              ("ritz {n} 13 13 0 1 1", "check_ritz", (13, 13), {"sample": True})]
    caps = plans([p[0].format(n=100_000_000) for p in probes], ncu)
    out = []
    for (line, fn, shape, opts), (f, _) in zip(probes, caps):
        rows = 32 * f.get("rtp", 1)                                      # rows per wave tile on the 16-byte path
        trips = 8 if fn == "check_ritz" else 4                           # (a Ritz grid is capped at one block per 8 row tiles)
        n = trips * f["blocks"] * rows + 2
        out.append((call(fn, n, *shape, **opts), line.format(n=n), rows))
    return out


@pytest.mark.parametrize("which", [0, 1, 2], ids=["gemm", "fused3", "ritz"])
def test_second_trip_of_the_grid_stride_loops(ctx, which):
    """tile += gridDim.x * 4 with the next tile's first column stage prefetched across the trip"""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    c, line, rows = second_trip_cases(ncu)[which]
    n = c[1][0]
    (f, name), = plans([line], ncu)
    assert n % 2 == 0 and -(-n // rows) > 4 * f["blocks"], (c, f)
    assert 8 * n * (c[1][1] + c[1][2] + 4) < 200e6
    try:
        ctx.reset_stats()
        run(ctx, c)
        assert ctx.kernel_stats().get(name, {}).get("launches", 0) > 0, (name, sorted(ctx.kernel_stats()))
        print(c, f["blocks"], name)
    finally:
        ctx.trim()


def test_worst_ratios():
    """the largest |got - ref| / bound per family over everything this file ran (DESIGN.md records them)"""
    for family, ratio in sorted(D.WORST.items()):
        print(f"worst ratio  {family:14s} {ratio:.4f}")
    assert all(r <= 1.0 for r in D.WORST.values())
