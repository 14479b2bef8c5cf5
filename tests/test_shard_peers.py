"""CPU: the case lists of tests/test_shard_peers_gpu.py on the host-memory engine (tests/hostsim.py), whose plain loops are the correct
implementation that has to stay within every bound -- this validates the harness of tests/shard_peers.py, its players and its bounds
without a GPU.  A case the host engine cannot meet has a wrong bound or a wrong player.

Left to the GPU file, because only the HIP engine has them: the column chunks of the sharded product, booked kernel names, the refusal
of m = 65, the peers_even instances, and synth_lrprec (the host engine has no such entry: here the 4-ulp bound is held against a float64
numpy evaluation of the kernel's own expression instead).  The run is one child process: the library a process has loaded cannot be
exchanged, and the other CPU tests of this process load the product's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shard_peers as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"product exact": len(S.PRODUCT_CASES), "product random": len(S.PRODUCT_CASES), "refusals": len(S.REFUSALS), "ritz": len(S.RITZ_CASES),
          "nrm2": len(S.NRM2_CASES), "sample products": len(S.SYNTH_CASES), "sample precnd": len(S.SYNTH_CASES),
          "sample lrprec (float64 emulation)": len(S.SYNTH_CASES)}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    out = tmp_path_factory.mktemp("shard_peers") / "report.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shard_peers.py"), str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.load(open(out))


def test_every_family_has_its_cases():
    assert set(COUNTS) == set(S.FAMILIES) and all(COUNTS.values())
    assert len(S.RITZ_CASES) == 2 * 3 * 4 * 6 and {(c["nranks"], c["rank"]) for c in S.RITZ_CASES} == set(S.POSITIONS)
    assert {len(S.synth_layout(c).shards) for c in S.SYNTH_CASES} == {2, 3, 8} and all(S.synth_layout(c).r0 > 0 for c in S.SYNTH_CASES)


@pytest.mark.parametrize("family", list(COUNTS))
def test_host_engine_meets_every_shared_case(report, family):
    """every case of the family ran, every exact case was bit-equal, every peers.check() was clean"""
    assert report[family]["failure"] is None, report[family]["failure"]
    assert report[family]["cases"] == COUNTS[family]


def test_worst_ratios(report):
    assert report["worst"], report
    for family, ratio in sorted(report["worst"].items()):
        print(f"{family:45s} {ratio:.4f}")
    assert all(r <= 1.0 for r in report["worst"].values()), report["worst"]


# ------------------------------------------------------------------------------------------------------------------ the harness itself
class FakeCtx:
    """what Peers needs of a context: the hook door.  reduce() is an engine's collective"""
    backend = "hostsim:fake"

    def __init__(self):
        self.fn, self.shard = None, None

    def set_allreduce_hook(self, fn, nranks, rank):
        self.fn = fn

    def set_shard(self, n_global, row0):
        self.shard = (n_global, row0)

    def reduce(self, values, op):
        buf = np.array(values, dtype=np.float64)
        self.fn(buf, op)
        return buf


def test_hook_plays_the_expected_exchanges_in_order():
    ctx = FakeCtx()
    with S.Peers(ctx, 2, 0) as peers:
        peers.expect(S.small_sum(np.array([[1.0, 3.0], [2.0, 4.0]])), S.nrm2_exchange(5.0))
        assert np.array_equal(ctx.reduce([10, 20, 30, 40], S.SUM), [11, 22, 33, 44])            # (column-major 2 x 2)
        assert np.array_equal(ctx.reduce([1.5], S.SUM), [6.5])
        peers.check()
        assert [(c, o) for c, o, _, _ in peers.calls] == [(4, S.SUM), (1, S.SUM)]
        assert np.array_equal(peers.calls[0][2], [10, 20, 30, 40]) and np.array_equal(peers.calls[0][3], [11, 22, 33, 44])
    assert ctx.fn is None and ctx.shard == (-1, 0)


@pytest.mark.parametrize("what", ["unexpected", "count", "op", "missing", "player raises"])
def test_hook_never_raises_and_check_reports(what):
    """nothing may leave a ctypes callback: a mismatch leaves the buffer as it came and is reported by check(), with the call list"""
    ctx = FakeCtx()

    def bad(buf):
        buf[0] = 99.0
        raise ValueError("boom")

    with S.Peers(ctx, 2, 1) as peers:
        if what == "count":
            peers.expect(S.small_sum(np.ones(3)))
        elif what == "op":
            peers.expect((2, S.MAX, lambda buf: None))
        elif what == "missing":
            peers.expect(S.small_sum(np.ones(2)), S.nrm2_exchange(1.0))
        elif what == "player raises":
            peers.expect((2, S.SUM, bad))
        got = ctx.reduce([1.0, 2.0], S.SUM)
        if what != "missing":
            assert np.array_equal(got, [1.0, 2.0])
        with pytest.raises(AssertionError, match="the calls of this rank"):
            peers.check()
        peers.check()                                                                     # (reported once)


def test_players_follow_the_layouts_of_the_comments():
    lay = S.Layout((5, 4, 6), 1)
    assert (lay.row0, lay.n_global, lay.n, lay.r0) == ([0, 5, 9], 15, 4, 5)
    # agreement: [row0 | tag | n_global] per rank, the peers copy this rank's tag
    count, op, play = S.agreement(lay)
    buf = np.zeros(9); buf[1], buf[4], buf[7] = 5, 4e15 + 3, 15
    play(buf)
    assert (count, op) == (9, S.SUM) and np.array_equal(buf, [0, 5, 9, 4e15 + 3, 4e15 + 3, 4e15 + 3, 15, 15, 15])
    # set-up: [need, bad] under max, then [row0, n] per rank
    (c1, o1, p1), (c2, o2, p2) = S.setup_exchanges(lay, peer_need=3)
    buf = np.array([2.0, 0.0]); p1(buf)
    assert (c1, o1, c2, o2) == (2, S.MAX, 6, S.SUM) and np.array_equal(buf, [3, 0])
    buf = np.zeros(6); buf[2:4] = 5, 4; p2(buf)
    assert np.array_equal(buf, [0, 5, 5, 4, 9, 6])
    # halo: buf[((r 2 + side) m + c) halo + h]; near sides from x, everything else this rank must not read is NaN
    xg = np.arange(30.0).reshape(2, 15).T.copy(order="F")
    count, op, play = S.halo_exchange(lay, 2, xg)
    buf = np.zeros(count); play(buf)
    b = buf.reshape(3, 2, 2, 2)
    assert count == 3 * 2 * 2 * 2 and np.all(b[1] == 0)
    assert np.array_equal(b[0, 1], [[3, 4], [18, 19]]) and np.array_equal(b[2, 0], [[9, 10], [24, 25]])
    assert np.all(np.isnan(b[0, 0])) and np.all(np.isnan(b[2, 1]))
    # Ritz on the host engine: sums, then maxima under max
    (c1, o1, p1), (c2, o2, p2) = S.ritz_exchanges(FakeCtx(), lay, 3, 2, np.array([1.0, 2.0]), [np.array([9.0, 0.5])] * 3)
    buf = np.array([1.0, 1.0]); p2(buf)
    assert (c1, o1, c2, o2) == (2, S.SUM, 2, S.MAX) and np.array_equal(buf, [9.0, 1.0])


def test_references_on_a_small_band():
    lay = S.Layout((4, 3), 1)
    a = S.banded(lay, np.random.default_rng(0), 1)
    assert a.shape == (7, 7) and (a != a.T).nnz == 0 and S.shard_need(a[lay.rows()], lay.r0, lay.n) == 1
    x = np.arange(1.0, 15.0).reshape(7, 2)
    y, mag = S.ref_banded(a[lay.rows()], x)
    assert np.array_equal(y.astype(float), (a @ x)[4:]) and np.array_equal(mag.astype(float), (abs(a) @ abs(x))[4:])
    blocks = S.banded(S.Layout((4, 3), 0), np.random.default_rng(0), 2, blocks=True)
    assert blocks[:4, 4:].nnz == 0 and blocks[4:, :4].nnz == 0
