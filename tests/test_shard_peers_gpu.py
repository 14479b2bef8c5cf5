"""GPU: one rank of a row-sharded run in one process, the test as its peers (tests/shard_peers.py: the scripted reduction hook, the
players of every exchange, the long-double references and the case lists).  Every path of the HIP engine that exists only for
nranks > 1 and travels through the hook transport is held to a reference of its own:

  a. the sharded ELLPACK product on integer data, bit-equal: halo_pack_kernel, ell_spmm_halo_kernel<4 | 8 | 16 | 32 | 0>, GatherHalo::at
     and the column chunks of spmm_matvec_sharded (42 + 6 columns; one column per exchange with the pack's second grid-stride trip);
     every slot this rank must not read arrives as NaN, every slot it must not write has to leave as +0.0
  b. the same on random data, (w + 2) eps |A||x|
  c. the refusals of spmm_setup_csr_sharded and dla_set_shard, status and full text, and an exact product after each
  d. peers_even: an even shard with an odd peer takes the VEC = 1 instances of ritz_kernel, the Gram kernels, gemm_kernel and
     synth_precnd_kernel -- the entries whose schedule reads Engine::even_rows / peers_even -- and with even peers what the CPU
     planner (tests/plans_driver.cpp) prints for the request
  e. the slot layout of ritz_reduce_kernel, [ncol sums | nranks x ncol maxima], before and after the one sum; dla_nrm2's one double
  f. the sample operators, synth_lrprec_kernel and synth_precnd_kernel<1 | 2> at row0 > 0; m = 65 refused
  g. the worst error-to-bound ratio per family

tests/test_shard_peers.py runs the same case lists on the host-memory engine.  Nothing here waits on a peer: every refusal is a
status return, every exchange is played synchronously by the test."""
import collections

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref as D
import shard_peers as S
from diaglib_amd import capi
from test_dense_sweeps_gpu import GEMM, GRAM, RITZ, booked, gemm_line, names_of
from test_operators_gpu import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(ctx):
    """device callbacks; whatever a case leaves in the operator slot is replaced by a plain operator (the session context must never
    keep a sharded one), and nothing is booked from here on"""
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    yield ctx
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 0)
    ctx.spmm_setup(sp.identity(4, format="csr"))
    ctx.reset_stats()


def ids(cases):
    return [c["name"] for c in cases]


# ------------------------------------------------------------------------------------------------------------------ a, b. the product
@pytest.mark.parametrize("case", S.PRODUCT_CASES, ids=ids(S.PRODUCT_CASES))
def test_sharded_product_is_exact_on_integer_data(dev, case):
    S.check_product(dev, case, True)


@pytest.mark.parametrize("case", S.PRODUCT_CASES, ids=ids(S.PRODUCT_CASES))
def test_sharded_product_on_random_data(dev, case):
    S.check_product(dev, case, False)


def test_the_case_list_reaches_every_width_bucket_and_both_chunk_regimes():
    """what the list is meant to contain, read off the list: the widths of the five instances of ell_spmm_halo_kernel, halo = 1 and
    halo = n_local, one row, the chunked exchange and the one-column regime"""
    widths = {c["w"] for c in S.PRODUCT_CASES}
    assert {3, 7, 13, 25, 33, 41} <= widths
    assert any(c["halo"] == 1 for c in S.PRODUCT_CASES) and any(c["halo"] == c["shards"][c["rank"]] for c in S.PRODUCT_CASES)
    assert any(c["shards"][c["rank"]] == 1 for c in S.PRODUCT_CASES)
    assert {tuple(c["hip_chunks"]) for c in S.PRODUCT_CASES if c["hip_chunks"] is not None} == {(42, 6), (1, 1), ()}
    assert {c["m"] for c in S.PRODUCT_CASES} >= {1, 13, 48}
    assert {len(c["shards"]) for c in S.PRODUCT_CASES} == {2, 3, 8}


# ------------------------------------------------------------------------------------------------------------------ c. refusals
@pytest.mark.parametrize("case", S.REFUSALS, ids=ids(S.REFUSALS))
def test_refused_setups_say_why_and_leave_the_context_usable(dev, case):
    S.check_refusal(dev, case)


# ------------------------------------------------------------------------------------------------------------------ d. peers_even
N_EVEN, L, M = 1000, 24, 13


def _three_calls(ctx, lay):
    """one dla_ritz_residual, one dla_gram, one dla_panel_gemm and one dla_synth_precnd on an even shard; the names they book"""
    rng = np.random.default_rng(7)
    ctx.reset_stats()
    ritz_case = dict(two=False, n=lay.n, m=M, n_res=M, skip="one", nranks=lay.nranks, rank=lay.rank)
    # (check_ritz lays its own peers out: the same heights by construction)
    assert S.peer_shards(lay.n, lay.nranks, lay.rank) == lay.shards
    S.check_ritz(ctx, ritz_case)
    with S.Peers(ctx, lay.nranks, lay.rank) as peers:
        peers.announce(lay)
        peers.expect(S.small_sum(np.zeros((L, M))))                 # (the peers' rows are zero: the Gram matrix is this rank's)
        D.check_gram(ctx, rng, lay.n, L, M)
        D.check_product(ctx, rng, lay.n, L, M, "gemm")
        x = np.asfortranarray(rng.standard_normal((lay.n, M)))
        ctx.synth_setup(lay.n_global, lay.r0, lay.n)
        gx, gp = D.NanGuarded(ctx, lay.n, M, x), Guarded(ctx, lay.n, M)
        S.call_precnd(ctx, "dla_synth_precnd", lay.n, M, 0.37, gx.ptr, gp.ptr)
        D.written(gp.body(), "synth_precnd")
        D.free(gx, gp)
        peers.check()
    return {fam: booked(ctx, fam) for fam in (RITZ, GRAM, GEMM, r"synth_precnd_kernel<")}


def _planned(n, vec2, nslots):
    return {RITZ: names_of([f"ritz {n} {L} {M} 0 {vec2} {nslots}"]), GRAM: names_of([f"gram {n} {L} {M} 0 {vec2} 0"]),
            GEMM: names_of([gemm_line(n, L, M, 0, 0, vec2)]), r"synth_precnd_kernel<": [f"synth_precnd_kernel<{2 if vec2 else 1}>"]}


@pytest.mark.parametrize("peer,vec2", [(107, 0), (106, 1)], ids=["odd peer", "even peers"])
def test_an_even_shard_takes_the_schedule_every_rank_takes(dev, monkeypatch, peer, vec2):
    """peers_even governs the sweeps of dla_ritz_residual (ritz_plan), dla_gram (gram_plan), dla_panel_gemm (launch_gemm) and
    dla_synth_precnd: 1000 aligned rows beside a peer of 107 rows book the VEC = 1 instances, beside 106 rows the instances the planner
    gives for the 16-byte request.  The results go through the checkers of tests/dense_ref.py either way."""
    monkeypatch.setattr(S, "peer_shards", lambda n, nranks, rank: [n, peer])
    lay = S.Layout([N_EVEN, peer], 0)
    got = _three_calls(dev, lay)
    want = _planned(N_EVEN, vec2, 2)
    for fam, names in want.items():
        assert got[fam] == dict(collections.Counter(names)), (fam, got[fam], names)
    other = _planned(N_EVEN, 1 - vec2, 2)
    assert all(set(want[fam]).isdisjoint(other[fam]) for fam in want), "the two schedules must differ in every family for this to be a test"


# ------------------------------------------------------------------------------------------------------------------ e. Ritz slots
RITZ_GROUPS = sorted({(c["two"], c["n"]) for c in S.RITZ_CASES})


@pytest.mark.parametrize("two,n", RITZ_GROUPS, ids=[f"{'ritz2' if t else 'ritz'}-n{n}" for t, n in RITZ_GROUPS])
def test_ritz_slots_before_and_after_the_one_sum(dev, two, n):
    cases = [c for c in S.RITZ_CASES if (c["two"], c["n"]) == (two, n)]
    assert {c["m"] for c in cases} == set(S.RITZ_M) and len(cases) == 24
    for c in cases:
        S.check_ritz(dev, c)


def test_ritz_reduction_is_one_exchange_of_whole_tiles(dev):
    """the layout itself: 13 columns as rank 1 of 3 are one sum of 16 + 3 x 16 doubles"""
    c = next(c for c in S.RITZ_CASES if c["m"] == 13 and c["n_res"] == 13 and (c["nranks"], c["rank"]) == (3, 1))
    lay = S.Layout(S.peer_shards(c["n"], 3, 1), 1)
    (count, op, _), = [e for e in S.ritz_exchanges(dev, lay, 13, 13, np.zeros(13), [np.zeros(13)] * 3)]
    assert (count, op) == (64, S.SUM)
    S.check_ritz(dev, c)


@pytest.mark.parametrize("case", S.NRM2_CASES, ids=[f"n{c['n']}-m{c['m']}" for c in S.NRM2_CASES])
def test_nrm2_is_one_double(dev, case):
    S.check_nrm2(dev, case)


# ------------------------------------------------------------------------------------------------------------------ f. sample operators
@pytest.mark.parametrize("case", S.SYNTH_CASES, ids=[f"n{c['n']}" for c in S.SYNTH_CASES])
def test_sample_products_on_a_shard(dev, oracle, case):
    S.check_synth_products(dev, oracle, case)


@pytest.mark.parametrize("case", S.SYNTH_CASES, ids=[f"n{c['n']}" for c in S.SYNTH_CASES])
def test_sample_lrprec_on_a_shard(dev, oracle, case):
    S.check_synth_lrprec(dev, oracle, case)


@pytest.mark.parametrize("case", S.SYNTH_CASES, ids=[f"n{c['n']}" for c in S.SYNTH_CASES])
def test_sample_precnd_on_a_shard(dev, oracle, case):
    S.check_synth_precnd(dev, oracle, case)


def test_sample_products_refuse_65_columns(dev):
    """m = 65: a status with its text, before any exchange"""
    lay = S.Layout((300, 256, 200), 1)
    dev.synth_setup(lay.n_global, lay.r0, lay.n)
    x, y = dev.panel(lay.n, 65).zero(), dev.panel(lay.n, 65)
    with S.Peers(dev, lay.nranks, lay.rank) as peers:
        for name, who in [("dla_synth_matvec", "synth_matvec"), ("dla_synth_apbmul", "dla_synth_apbmul"), ("dla_synth_metric", "dla_synth_metric")]:
            with pytest.raises(capi.DlaError) as e:
                S.call_matvec(dev, name, lay.n, 65, x.ptr, y.ptr)
            assert str(e.value) == f"status 3: {who} failed: synth operator: m > 64"
        peers.check()
    x.free(); y.free()


@pytest.mark.parametrize("which", ["x", "px", "neither"])
def test_sample_precnd_off_a_16_byte_boundary_books_the_one_row_instance(dev, oracle, which):
    """even n, even peers: the panel 8 bytes off a 16-byte boundary takes synth_precnd_kernel<1>, the aligned call <2>; 4 ulp either way"""
    lay = S.Layout((300, 1000, 200), 1)
    _, diag_g, _, _ = S.synth_global(oracle, lay.n_global)
    dev.synth_setup(lay.n_global, lay.r0, lay.n)
    x = np.asfortranarray(S.rng_of("off", which).standard_normal((lay.n, 7)))
    gx, gp = Guarded(dev, lay.n, 7, x, offset=8 if which == "x" else 0), Guarded(dev, lay.n, 7, offset=8 if which == "px" else 0)
    with S.Peers(dev, lay.nranks, lay.rank) as peers:
        peers.announce(lay)
        dev.reset_stats()
        S.call_precnd(dev, "dla_synth_precnd", lay.n, 7, 0.37, gx.ptr, gp.ptr)
        peers.check()
    assert S.booked_precnd(dev) == {f"synth_precnd_kernel<{2 if which == 'neither' else 1}>": 1}
    got = D.written(gp.body(), "synth_precnd " + which)
    ref = D.ld(x) / (D.ld(diag_g[lay.rows()]) + S.LD(0.37))[:, None]
    assert S.note("sample precnd on a shard (ulp / 4)", float(S.ulps(got, ref).max()) / 4) <= 1
    D.free(gx, gp)


# ------------------------------------------------------------------------------------------------------------------ g. worst ratios
def test_worst_ratios():
    """the worst |got - ref| / bound of every family this file ran (printed with -s; profiles/shard_peers.txt keeps a run)"""
    assert S.WORST, "no family was run before this test"
    for family, ratio in sorted(S.WORST.items()):
        print(f"{family:45s} {ratio:.4f}")
    assert all(r <= 1.0 for r in S.WORST.values()), S.WORST
