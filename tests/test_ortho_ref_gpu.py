"""GPU: the orthogonalisation on the standard inner product -- dla_ortho_cd and dla_ortho_vs_x -- against the long-double reference of
tests/ortho_ref.py, with bounds that follow each case's conditioning (the cancellation a of the projection and of the factorisation,
its column-equilibrated form a_eq, the norm pi of the projector; see that module).  The CPU test tests/test_ortho_ref.py shows on the
same cases that the double-precision oracle meets a quarter of every bound, and that the blocks meant to need level shifts do.

What runs here and nowhere else at kernel level:
  * ortho_tail16, the matrix-core k x k step (blocked 4-row LDL^T, rank-4 updates, masked rows): every 4-row block boundary and the
    partly masked last block (k = 1, 2, 3, 4, 8, 12, 13, 15), the full tile k = 16; the one-wave LDS-loop step at its tile edges
    (17, 31 / 32 / 33, 47 / 48); the hand-over to the host-driven loop at 49;
  * the level-shift ladder in both steps and on the sweep-per-update route (odd n), on blocks whose double-precision Gram matrix
    provably has no Cholesky factorisation (graded to condition 1e10, rank deficient);
  * both sides of every edge of chain_choice (hip_plans.h), see ortho_ref.EDGE_CASES;
  * every case twice in a row (the default or a neighbour's plan, then its own history), under the schedules of tune knob 6 (0 the
    shipped choice, 12 five-sweep, 13 three-pass from the first chain on, 3 the host-driven loop) and with X and U in separate panels;
  * guard columns around [X | U].

$DIAGLIB_ORTHO_REF_RECORD names a file the worst ratios error / bound of every case are appended to (profiles/ortho_ref.txt)."""
import os
import types

import numpy as np
import pytest

import ortho_ref as R

pytestmark = pytest.mark.gpu
RECORD = os.environ.get("DIAGLIB_ORTHO_REF_RECORD")
GUARD = 1e30
HOST_LOOP = 3
CHAIN_ROUTES = (("chain", 0), ("chain", 12), ("chain", 13))
ROUTES = CHAIN_ROUTES + (("chain", HOST_LOOP), ("separate", 0))           # m > 0
ROUTES_ALONE = (("alone", 0), ("alone", HOST_LOOP))                       # m = 0: ortho_cd


def _run(ctx, c, route, knob):
    """one call under tune knob 6 = knob; the host waits are those of the call itself"""
    ctx.set_option(R.TUNE6, knob)
    ok = True
    if c.m == 0:
        px, pu = None, ctx.panel(c.u)
    elif route == "separate":
        px, pu = ctx.panel(c.x), ctx.panel(c.u)
    else:
        big = ctx.panel(np.asfortranarray(np.hstack([c.x, c.u])))
        px, pu = big.col(0, c.m), big.col(c.m, c.k)
    s0 = ctx.stats()["host_syncs"]
    if c.m == 0:
        ok = ctx.ortho_cd(pu)[1]
    else:
        ctx.ortho_vs_x(px, pu)
    syncs = ctx.stats()["host_syncs"] - s0
    return types.SimpleNamespace(q=pu.download(), x_after=px.download() if px is not None else None, syncs=syncs, ok=ok)


@pytest.mark.parametrize("key", R.ALL_CASES, ids=R.ident)
def test_every_route_twice_against_the_long_double_reference(ctx, key):
    """every route passes the checker on both runs and the routes agree with each other within the bound on |Q - Q_ref|.  Second run
    of a plain random block behind an X: the chain costs one host wait; the host-driven loop (knob 3, separate panels) costs more; k = 49 is the
    host-driven loop under every knob.  After a rank-deficient block (invariants only) the well-conditioned block of the same shape
    passes on the same route: status word, phase and re-arm state are clean after a chain that shifted."""
    c = R.case(*key)
    twin = None if c.unique else R.case(*R.well_conditioned_twin(key))
    rows, second = [], {}
    try:
        for route, knob in (ROUTES if c.m else ROUTES_ALONE):
            for attempt in (1, 2):
                r = _run(ctx, c, route, knob)
                what = f"{c.name} {route} knob6={knob} run {attempt} (host waits {r.syncs})"
                assert r.ok, what + ": ortho_cd reports failure"
                rows.append(("device " + what, R.check(r.q, c, r.x_after, what=what)))
            second[(route, knob)] = r
            if twin is not None:
                t = _run(ctx, twin, route, knob)
                what = f"{twin.name} {route} knob6={knob} after {c.kind} (host waits {t.syncs})"
                assert t.ok, what
                rows.append(("device " + what, R.check(t.q, twin, t.x_after, what=what)))
    finally:
        ctx.set_option(R.TUNE6, 0)
    R.record(RECORD, rows)
    routes = list(second)
    if c.unique:
        for other in routes[1:]:
            assert np.abs(second[other].q - second[routes[0]].q).max() <= R.q_bound(c.ref()), (c.name, other)
    host = second[routes[0][0], HOST_LOOP].syncs
    chains = [second[r].syncs for r in (CHAIN_ROUTES if c.m else ROUTES_ALONE[:1])]
    if c.k > 48:
        assert all(s == host for s in chains), (c.name, chains, host)         # chain_choice declines: the host loop's count
    else:
        assert all(s <= 3 for s in chains), (c.name, chains)                  # a few waits when the expected schedule does not hold
        if c.kind == "random" and c.m:
            assert all(s == 1 for s in chains), (c.name, chains)              # one wait once the chain has its own history
        if c.m:                                                               # (a block alone may take the host loop one wait as well)
            assert host > max(chains), (c.name, chains, host)
            assert second["separate", 0].syncs > max(chains), (c.name, chains, second["separate", 0].syncs)
        else:
            assert host >= max(chains), (c.name, chains, host)


@pytest.mark.parametrize("key", R.GUARD_CASES, ids=R.ident)
def test_nothing_is_written_outside_the_block(ctx, key):
    """the panel is [1e30 | X | U | 1e30], X at column 1 (odd n: 8-byte aligned only): both guard columns and X are bit-identical after the
    call, twice in a row, and the results pass"""
    c = R.case(*key)
    wall = np.full((c.n, 1), GUARD)
    rows = []
    for attempt in (1, 2):
        big = ctx.panel(np.asfortranarray(np.hstack([wall, c.x, c.u, wall])))
        ctx.ortho_vs_x(big.col(1, c.m), big.col(1 + c.m, c.k))
        got = big.download()
        what = f"{c.name} between guard columns run {attempt}"
        assert np.array_equal(got[:, :1], wall) and np.array_equal(got[:, -1:], wall), what + ": a guard column was modified"
        rows.append(("device " + what, R.check(got[:, 1 + c.m:-1], c, got[:, 1:1 + c.m], what=what)))
    R.record(RECORD, rows)
