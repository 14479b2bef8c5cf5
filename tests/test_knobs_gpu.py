"""The engine's experiment knobs (DLA_OPT_TUNE0 + i, Knobs in hip_plans.h) still reach the decisions that the tests, bench.py and the
A/B tools take from them -- read off the kernels that ran (launch counts of ctx.kernel_stats()), not off the results, which the
suites of the kernels themselves check.

Shapes: the smallest that still take the 16-byte chain paths -- n = 4096 rows, a one-tile block of 13 columns behind 26 basis
columns, a two-tile block of 21 columns (16 + 5: two quarter instructions for the last tile) behind 42.

Every case runs in a context of its own: the library's context belongs to the calling thread, so a case is a short-lived thread
that destroys its context when it ends.  After each case every knob reads back 0.

One thing the launch counts cannot show: the engine books both instances of the reduction, gram_reduce_kernel<false> and <true>
(the one that carries a chain's tail), under the one name `gram_reduce_kernel`.  The host-driven-loop case therefore checks what
tells the two apart from outside: no k x k tail kernel of a chain ran, and the host waited for a small result more often than with
the chain (the chain reports once at its end; the host-driven loop reads every Gram matrix before it can decide the next sweep)."""
import re
import threading

import numpy as np
import pytest

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
TUNE0 = 100
N = 4096

# what bench.py sorts kernels by: the family prefix, `gemm_kernel<KT, VEC, 2,` for the triangular update, and the launches that move
# no panel bytes; here with every template argument, as rocprofv3 prints them and profiles/pmc_traffic.json keys them
BENCH_KEYS = [
    r"gram_lds_kernel<\d+, \d+, 1, (16|32), [01], [0-3], [01], [012]>",
    r"gram_kernel<\d+, \d+, [12], \d+, 0, -1>",
    r"gram_reduce_kernel",
    r"gemm_kernel<\d+, [12], [0-3], GemmArgs(Inl)?, (true|false), [01], [0-4], 9, [0-3], [12]>",
    r"ritz_kernel<\d+, [12], 3, [0-4], [0-3], (true|false), 0>",
    r"ritz_reduce_kernel",
    r"ortho_tail(16)?_kernel",
]


@pytest.fixture(scope="module")
def blocks():
    """an orthonormal basis of 42 columns and a random block of 21: computed once, read only"""
    rng = np.random.default_rng(20240611)
    x, _ = np.linalg.qr(rng.standard_normal((N, 42)))
    u = rng.standard_normal((N, 21))
    x.setflags(write=False); u.setflags(write=False)
    return x, u


def fresh_context(work):
    """work(ctx) with a context nobody has used, destroyed afterwards; every knob must read 0 once it has been put back"""
    out = {}

    def run():
        c = capi.Context()
        try:
            assert c.backend.startswith("hip:"), c.backend
            assert [c.get_option(TUNE0 + i) for i in range(8)] == [0] * 8
            out["value"] = work(c)
        except BaseException as e:      # (reported in the test's thread)
            out["error"] = e
        finally:
            for i in range(8):
                c.set_option(TUNE0 + i, 0)
            out["left"] = [c.get_option(TUNE0 + i) for i in range(8)]
            c.destroy()

    t = threading.Thread(target=run)
    t.start(); t.join()
    if "error" in out:
        raise out["error"]
    assert out["left"] == [0] * 8
    return out["value"]


def set_knob(c, knob, value):
    c.set_option(TUNE0 + knob, value)
    assert c.get_option(TUNE0 + knob) == value


def launched(c):
    return {name: st["launches"] for name, st in c.kernel_stats().items() if st["launches"] > 0}


def first_chain(c, blocks, m, k):
    """the first ortho_vs_x of a solve: the k-column block that follows m basis columns in one panel"""
    x, u = blocks
    p = c.panel(np.asfortranarray(np.hstack([x[:, :m], u[:, :k]])))
    c.reset_stats()
    c._chk(c.lib.dla_begin_solve(c.h))
    c.ortho_vs_x(p.col(0, m), p.col(m, k))
    return launched(c), c.stats()["host_syncs"]


def args_of(name):
    return name[name.index("<") + 1:-1].split(", ")


def measuring_projection_sweeps(names):
    return [nm for nm in names if nm.startswith("gram_lds_kernel<") and args_of(nm)[7] == "2"]


def test_option_numbers_round_trip():
    def work(c):
        values = [4, 3, 1, 2, -1, 3, 17, 23]
        for i, v in enumerate(values):
            set_knob(c, i, v)
        assert [c.get_option(TUNE0 + i) for i in range(8)] == values      # (no knob disturbs another)
    fresh_context(work)


@pytest.mark.parametrize("knob6,expect", [(13, True), (12, False)])
def test_schedule_knobs_of_the_first_chain(blocks, knob6, expect):
    """6 = 13: the three-pass schedule from the first chain of a solve -- its projections are measuring sweeps (gram_lds_kernel<..., 2>);
    6 = 12: the five-sweep schedule, which has none"""
    def work(c):
        set_knob(c, 6, knob6)
        return first_chain(c, blocks, 26, 13)[0]
    names = fresh_context(work)
    assert any(nm.startswith("ortho_tail16_kernel") for nm in names), names          # a chain of the one-tile schedule ran
    assert bool(measuring_projection_sweeps(names)) == expect, names


def test_host_loop_knob_runs_no_chain(blocks):
    """6 = 3: the host-driven loop -- no k x k tail kernel, and no reduction that carries one (see the module's docstring)"""
    def work(knob6):
        def w(c):
            set_knob(c, 6, knob6)
            return first_chain(c, blocks, 26, 13)
        return w
    chain_names, chain_waits = fresh_context(work(0))
    host_names, host_waits = fresh_context(work(3))
    assert any(nm.startswith("ortho_tail") for nm in chain_names), chain_names
    assert not any(nm.startswith("ortho_tail") for nm in host_names), host_names
    assert host_names.get("gram_reduce_kernel", 0) > 0, host_names
    print("host waits: chain", chain_waits, "host-driven loop", host_waits)
    assert host_waits > chain_waits, (host_waits, chain_waits)


@pytest.mark.parametrize("knob7", [1, 0])
def test_quarter_tile_knob(blocks, knob7):
    """7 = 1: every two-tile kernel of the 21-column block is booked with quarter-tile argument 0; 7 = 0: with 2 (21 = 16 + 5 columns)"""
    x, u = blocks

    def work(c):
        set_knob(c, 7, knob7)
        chain = first_chain(c, blocks, 42, 21)[0]
        c.reset_stats()
        px, pu = c.panel(np.asfortranarray(x)), c.panel(np.asfortranarray(u))
        c.gram(px, pu)                                                    # gram_lds_kernel, two U tiles
        c.panel_gemm(px, np.asfortranarray(x.T @ u), c.panel(N, 21))      # plain gemm_kernel, mode 0
        c.update_gram(px, np.asfortranarray(x.T @ u), pu)                 # fused gemm_kernel
        return chain, launched(c)
    chain, direct = fresh_context(work)
    qt = {"gemm_kernel": [], "gram_lds_kernel": []}
    for names in (chain, direct):
        for nm in names:
            a = args_of(nm) if "<" in nm else []
            if nm.startswith("gemm_kernel<") and a[0] == "2":
                qt["gemm_kernel"].append(int(a[8]))
            if nm.startswith("gram_lds_kernel<") and a[1] == "2":
                qt["gram_lds_kernel"].append(int(a[5]))
    print(knob7, sorted(chain), sorted(direct))
    assert qt["gemm_kernel"] and qt["gram_lds_kernel"], (chain, direct)
    if knob7 == 1:
        assert set(qt["gemm_kernel"]) == {0} and set(qt["gram_lds_kernel"]) == {0}, (chain, direct)
        assert "gemm_kernel<2, 2, 0, GemmArgs, false, 1, 2, 9, 0, 2>" in direct, direct
    else:
        # (not every two-tile kernel has the variant -- the plain two-tile update measured slower with it -- but each family has)
        assert 2 in qt["gemm_kernel"] and 2 in qt["gram_lds_kernel"], (chain, direct)
        assert "gemm_kernel<2, 2, 0, GemmArgs, false, 1, 2, 9, 2, 2>" in direct, direct


def test_gemm_depth_knob_is_booked_as_launched(blocks):
    """2 = 1: the plain two-tile product runs the instance without a column-step pipeline and without quarter tiles -- and the
    statistics say so (pipeline depth 0 in the name, as rocprofv3 prints the launched kernel)"""
    x, u = blocks

    def work(c):
        set_knob(c, 2, 1)
        c.reset_stats()
        c.panel_gemm(c.panel(np.asfortranarray(x)), np.asfortranarray(x.T @ u), c.panel(N, 21))
        return launched(c)
    names = fresh_context(work)
    assert names == {"gemm_kernel<2, 2, 0, GemmArgs, false, 1, 0, 9, 0, 2>": 1}, names


def test_default_names_are_the_benchmarks_keys(blocks):
    """every knob 0: what the statistics book are the names bench.py and profiles/pmc_traffic.json key on"""
    x, u = blocks

    def work(c):
        names = dict(first_chain(c, blocks, 26, 13)[0])
        names.update(first_chain(c, blocks, 42, 21)[0])
        c.reset_stats()
        v, av = c.panel(np.asfortranarray(x[:, :26])), c.panel(np.asfortranarray(x[:, 16:42]))
        y = np.asfortranarray(np.eye(26)[:, :13])
        c.ritz_residual(v, av, y, np.arange(13.0), 13, np.zeros(13, np.int32), c.panel(N, 13), c.panel(N, 13))
        pu = c.panel(np.asfortranarray(u[:, :13]))
        c.trmm_linvt(pu, np.asfortranarray(np.tril(np.ones((13, 13))) + np.eye(13)))
        c.panel_gemm(v, np.asfortranarray(np.ones((26, 13))), c.panel(N, 13))
        names.update(launched(c))
        return names
    names = fresh_context(work)
    print(sorted(names))
    for nm in names:
        assert any(re.fullmatch(pat, nm) for pat in BENCH_KEYS), nm
    assert "ritz_kernel<1, 2, 3, 0, 0, false, 0>" in names, names                    # the benchmark's dominant kernel
    assert any(re.match(r"gemm_kernel<\d+, \d+, 2,", nm) for nm in names), names      # bench.py's pattern for the triangular update
    assert any(nm.startswith("gram") for nm in names) and any(nm.startswith("ritz") for nm in names)


FAMILIES = r"(gram_lds_kernel|gram_kernel|gemm_kernel|ritz_kernel|ritz2_kernel)<"


def test_solver_names_are_the_planners_names(blocks):
    """every knob 0.  The statistics carry names and no shapes, so names are tied to shapes in two steps.

    1. One Davidson and one LOBPCG solve (8 roots, n_max = 13): every name of the Gram, product, Ritz and tail families that they book
       is one of bench.py's keys (the two-coefficient Ritz sweep, which bench.py does not key, by its own pattern), and every Gram,
       product and Ritz sweep carries a name the CPU planners (tests/plans_driver.cpp) print at n = 4096 for a shape such a solve can
       issue -- blocks shrink as roots converge, so every basis width up to 20 blocks counts.  This step alone would pass
       a wrong argument that spells another name of the family.
    2. The sweeps those solves are made of, called one at a time at known shapes in the same context, with the statistics reset
       before each: the names booked must EQUAL what the driver prints for the request line of exactly that (n, l, k, ...) -- mode,
       fuse, packed_on_device, same and lower as the call site passes them.  For the chain, whose sweeps depend on the schedule that
       is taken, the names must lie within the driver's for that chain's m and k, and its measuring sweep and fused projection must
       be among them."""
    from test_plans import env_line, run_plans
    n_targ, n_max, max_dav = 8, 13, 20
    x, u = blocks
    wide = np.asfortranarray(np.hstack([x, x, x])[:, :117])
    ones = lambda l, k: np.asfortranarray(np.ones((l, k)))
    tri = np.asfortranarray(np.triu(np.ones((13, 13))) + np.eye(13))

    def ritz(c, l, m):
        v, av = c.panel(np.asfortranarray(wide[:, :l])), c.panel(np.asfortranarray(wide[:, 3:l + 3]))
        c.ritz_residual(v, av, np.asfortranarray(np.eye(l)[:, :m]), np.arange(float(m)), m, np.zeros(m, np.int32), c.panel(N, m), c.panel(N, m))

    def combo(c):
        p = c.panel(np.asfortranarray(np.hstack([x[:, :26], u[:, :13]])))
        c.combo_gram(p.col(0, 26), np.asfortranarray(np.eye(39)[:, 26:]), p.col(26, 13))

    def same13(c):
        p = c.panel(np.asfortranarray(u[:, :13]))
        c.gram(p, p)

    # (request line of the plans driver, the call of exactly that shape)
    known = [
        (f"gram {N} 13 13 1 1 0", same13),
        (f"gram {N} 26 13 0 1 0", lambda c: c.gram(c.panel(np.asfortranarray(x[:, :26])), c.panel(np.asfortranarray(u[:, :13])))),
        (f"gram {N} 117 13 0 1 0", lambda c: c.gram(c.panel(wide), c.panel(np.asfortranarray(u[:, :13])))),
        (f"gram {N} 42 21 0 1 0", lambda c: c.gram(c.panel(np.asfortranarray(x)), c.panel(np.asfortranarray(u)))),
        (f"gram {N} 4 13 0 1 0", lambda c: c.gram(c.panel(np.asfortranarray(x[:, :4])), c.panel(np.asfortranarray(u[:, :13])))),
        (f"gram {N} 39 39 0 1 1", lambda c: c.gram_lower(c.panel(np.asfortranarray(x[:, :39])), c.panel(np.asfortranarray(wide[:, 50:89])))),
        (f"gemm {N} 13 13 0 0 0 1", lambda c: c.panel_gemm(c.panel(np.asfortranarray(x[:, :13])), ones(13, 13), c.panel(N, 13))),
        (f"gemm {N} 26 13 0 0 0 1", lambda c: c.panel_gemm(c.panel(np.asfortranarray(x[:, :26])), ones(26, 13), c.panel(N, 13))),
        (f"gemm {N} 42 21 0 0 0 1", lambda c: c.panel_gemm(c.panel(np.asfortranarray(x)), ones(42, 21), c.panel(N, 21))),
        (f"gemm {N} 42 21 1 1 0 1", lambda c: c.update_gram(c.panel(np.asfortranarray(x)), np.asfortranarray(x.T @ u), c.panel(np.asfortranarray(u)))),
        (f"gemm {N} 39 13 0 1 0 1", combo),
        (f"gemm {N} 13 13 2 0 0 1", lambda c: c.trmm_linvt(c.panel(np.asfortranarray(u[:, :13])), np.asfortranarray(tri.T))),
        (f"gemm {N} 13 13 2 1 0 1", lambda c: c.trmm_gram(c.panel(np.asfortranarray(u[:, :13])), tri)),
        (f"ritz {N} 26 8 0 1 1", lambda c: ritz(c, 26, 8)),
        (f"ritz {N} 104 13 0 1 1", lambda c: ritz(c, 104, 13)),
        (f"ritz {N} 42 21 0 1 1", lambda c: ritz(c, 42, 21)),
    ]

    def swept(names):
        return sorted(nm for nm in names if re.match(FAMILIES, nm))

    def work(c):
        c.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
        c.synth_setup(N, 0, N)
        mv, pc = capi.fn_address("dla_synth_matvec"), capi.fn_address("dla_synth_precnd")
        guess = np.zeros((N, n_max), order="F")
        guess[np.arange(n_max), np.arange(n_max)] = 1.0
        c.reset_stats()
        c.davidson_driver(N, n_targ, n_max, 100, 1e-9, max_dav, 0.0, mv, pc, c.panel(guess))      # (whether they converge is the solver suites' matter)
        c.lobpcg_driver(N, n_targ, n_max, 60, 1e-9, 0.0, mv, pc, c.panel(guess))
        solves = launched(c)
        one_by_one = []
        for _, call in known:
            c.reset_stats()
            call(c)
            one_by_one.append(swept(launched(c)))
        return solves, one_by_one, swept(first_chain(c, blocks, 26, 13)[0])
    names, one_by_one, chain = fresh_context(work)
    print(sorted(names))
    # ---- 1. the solves
    keys = BENCH_KEYS + [r"ritz2_kernel<[123], [12]>"]
    for nm in names:            # (a solve also books the operator's and the element-wise kernels, which belong to no family)
        if re.match(r"(gram|gemm|ritz|ortho)", nm):
            assert any(re.fullmatch(pat, nm) for pat in keys), nm
    basis = range(0, max_dav * n_max + 1)
    lines = [env_line()]              # (no name depends on the CU count: it only sets block counts)
    lines += [f"gram {N} {l} {k} {same} 1 {low}" for l in basis[1:] for k in range(1, 49) for same in (0, 1) for low in (0, 1) if l == k or not (same or low)]
    lines += [f"gram {N} {l} {l} {same} 1 {low}" for l in basis[49:] for same in (0, 1) for low in (0, 1)]
    lines += [f"wp {N} {m} {k} {pr}" for m in basis for k in range(1, n_max + 1) for pr in (0, 1) if m or not pr]
    lines += [f"gemm {N} {l} {k} {mode} {fuse} {pk} 1" for l in basis[1:] for k in range(1, 49) for mode in range(4) for fuse in (0, 1) for pk in (0, 1)
              if not (fuse and mode == 3)]
    lines += [f"ritz {N} {l} {m} {k2} 1 1" for l in basis[1:] for m in range(1, n_max + 1) for k2 in range(0, 2 * n_max + 1)]
    lines += [f"ritz2 {N} {l} {m} 1 1" for l in basis[1:] for m in range(1, n_max + 1)]
    table = {name for _, name in run_plans(lines)[0]}
    ran = swept(names)
    assert any(nm.startswith("gram") for nm in ran) and any(nm.startswith("gemm") for nm in ran) and any(nm.startswith("ritz") for nm in ran)
    assert not [nm for nm in ran if nm not in table], [nm for nm in ran if nm not in table]
    # ---- 2. one sweep at a time, one to one
    expect = [name for _, name in run_plans([env_line()] + [req for req, _ in known])[0]]
    for (req, _), want, got in zip(known, expect, one_by_one):
        print(req, "->", want, got)
        assert got == [want], (req, want, got)
    m, k = 26, 13
    lines = [env_line(), f"wp {N} {m} {k} 0", f"gemm {N} {m + k} {k} 0 1 1 1", f"wp {N} {m} {k} 1"]
    lines += [f"gemm {N} {l} {k} {mode} {fuse} 1 1" for l in (k, m + k) for mode in (0, 2) for fuse in (0, 1)]
    of_chain = [name for _, name in run_plans(lines)[0]]
    print("chain", chain)
    assert set(chain) <= set(of_chain) and of_chain[0] in chain and of_chain[1] in chain, (chain, of_chain)
