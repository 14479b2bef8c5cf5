"""GPU: whole Davidson solves with the next block formed inside the Ritz sweep (dla_ritz_expand in davidson_core), in three settings:
the product (fused sweeps on), knob 0 = 16 (off: the sweep, the preconditioner and the chain's own first sweep as before) and knob 0 = 17
(the driver bets on one lock more than its rule says, so that bets are lost and fused sweeps discarded).

The small golden configurations of tests/test_golden_gpu.py -- the reference's dense test matrix a(i,j) = 1 / (i + j), a(i,i) = i + 1,
the fixtures' guesses and parameters -- run here on the library's own dense operator and its diagonal preconditioner with device
callbacks (the fused sweep takes no caller-supplied preconditioner): eigenvalues within that file's tolerance of the fixtures,
iteration counts as the fixtures', the counters say which path ran, and a repeated solve is bit-identical in every setting.  One
solve each on a stored sparse and a stored dense operator compares fused on against off."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from diaglib_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = {"fused": 0, "off": 16, "forced miss": 17}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_fixtures.npz"), allow_pickle=False)


def _guess(kind, n, m, seed):
    if kind == "unit":
        g = np.zeros((n, m), order="F"); g[np.arange(m), np.arange(m)] = 1.0
        return g
    return np.asfortranarray(np.random.default_rng(seed).random((n, m)) - 0.5)


def _reference_matrix(n):
    idx = np.arange(1, n + 1.0)
    a = 1.0 / (idx[:, None] + idx[None, :])
    np.fill_diagonal(a, idx + 1.0)
    return np.asfortranarray(a)


def _solve(ctx, knob, n, t, m, max_iter, tol, max_dav, shift, guess, matvec, precnd):
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    ctx.set_option(100, knob)
    run0, dropped0 = ctx.ritz_expand_counts()
    ev = ctx.panel(guess)
    eig, _, ok, info = ctx.davidson_driver(n, t, m, max_iter, tol, max_dav, shift, capi.fn_address(matvec), capi.fn_address(precnd), ev)
    vec = ev.download()
    run1, dropped1 = ctx.ritz_expand_counts()
    return eig, vec, ok, info, run1 - run0, dropped1 - dropped0


@pytest.mark.parametrize("name", ["dav_n2000_unit", "dav_n2000_rand", "dav_n600_rand_dav10"])
def test_golden_configurations_in_three_settings(ctx, gold, name):
    spec = next(s for s in json.loads(str(gold["driver_specs"])) if s["name"] == name)
    n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
    g = _guess(spec["guess"], n, m, spec["seed"])
    ctx.dense_setup(_reference_matrix(n))
    it_ref = int(gold[name + "_tr_iters"])
    seen = {}
    for setting, knob in SETTINGS.items():
        args = (ctx, knob, n, t, m, spec["max_iter"], spec["tol"], spec["max_dav"], spec["shift"], g, "dla_dense_matvec", "dla_dense_precnd")
        eig, vec, ok, info, ran, dropped = _solve(*args)
        print(f"{name} [{setting}]: iters {info['iters']} (fixture {it_ref}), restarts {info['restarts']}, fused sweeps {ran}, discarded {dropped}, "
              f"max rel eig error {np.abs(eig[:t] / gold[name + '_eig'][:t] - 1).max():.2e}")
        assert ok and bool(gold[name + "_ok"])
        assert np.allclose(eig[:t], gold[name + "_eig"][:t], rtol=1e-10, atol=0)
        assert info["iters"] == it_ref, (setting, info, it_ref)
        if setting == "fused":
            assert ran > 0 and dropped < ran
        elif setting == "off":
            assert ran == 0 and dropped == 0
        else:
            assert dropped > 0
        eig2, vec2, ok2, info2, ran2, dropped2 = _solve(*args)
        assert ok2 and info2 == info and (ran2, dropped2) == (ran, dropped)
        assert np.array_equal(eig, eig2) and np.array_equal(vec, vec2), f"{name} [{setting}]: a repeated solve differs"
        seen[setting] = (eig, vec)
    # the fused sweep stores the residuals and the block of the plain path and leaves its measuring sweep's partials, all bit for bit:
    # only the norms are summed in another order, which no lock of these solves depends on
    same = {s: bool(np.array_equal(seen[s][0], seen["off"][0]) and np.array_equal(seen[s][1], seen["off"][1])) for s in seen}
    print(f"{name}: bit-identical to the plain path: {same}")
    assert all(same.values())


def _compare_on_off(ctx, n, t, m, guess, matvec, precnd):
    out = {}
    for setting in ("fused", "off"):
        eig, _, ok, info, ran, dropped = _solve(ctx, SETTINGS[setting], n, t, m, 100, 1e-9, 10, 0.0, guess, matvec, precnd)
        print(f"{matvec} [{setting}]: iters {info['iters']}, fused sweeps {ran}, discarded {dropped}, eig {eig[:t]}")
        assert ok
        out[setting] = (eig[:t], ran)
    assert out["fused"][1] > 0 and out["off"][1] == 0
    assert np.allclose(out["fused"][0], out["off"][0], rtol=1e-11, atol=0)


def test_stored_sparse_operator_fused_against_off(ctx):
    n, t, m = 2000, 4, 8
    rng = np.random.default_rng(11)
    off = rng.uniform(-0.3, 0.3, n - 1)
    far = rng.uniform(-0.1, 0.1, n - 7)
    a = sp.diags([np.arange(1.0, n + 1.0), off, off, far, far], [0, 1, -1, 7, -7]).tocsr()
    ctx.spmm_setup(a)
    _compare_on_off(ctx, n, t, m, _guess("unit", n, m, 0), "dla_spmm_matvec", "dla_spmm_precnd")


def test_stored_dense_operator_fused_against_off(ctx):
    n, t, m = 512, 4, 8
    rng = np.random.default_rng(12)
    b = rng.uniform(-0.2, 0.2, (n, n))
    a = (b + b.T) / 2
    np.fill_diagonal(a, np.arange(1.0, n + 1.0))
    ctx.dense_setup(np.asfortranarray(a))
    _compare_on_off(ctx, n, t, m, _guess("unit", n, m, 0), "dla_dense_matvec", "dla_dense_precnd")
