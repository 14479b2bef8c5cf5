"""The sample sparse operator on ROW SHARDS (dla_spmm_setup_csr_sharded, SURVEY 8f row 4 + 8e): every rank holds its rows of a
banded symmetric matrix with global column indices; the halo rows of x travel through the same all-reduce transport as the
small products (every rank fills its own slots of a zeroed buffer, the sum gathers).

CPU leg: the host-memory engine over gloo (2 and 3 ranks, banded and ragged).  GPU legs: two ranks sharing one GPU over the
reduction hook and over the peer-to-peer mailboxes, three ranks (a middle rank with both halos) over the hook.  Checked: the product against scipy on every shard, a Davidson solve on the sharded operator against
the single-rank solve and against a dense eigensolver, and that a matrix with a long-range coupling is refused on every rank."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, json
os.environ.setdefault("OMP_NUM_THREADS", "2")
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import scipy.sparse as sp
from diaglib_amd import capi
spec = json.loads({spec!r})
if spec["backend"] == "hostsim":
    import hostsim
    capi.load(hostsim.build())
import torch, torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
from bench import shard_rows
n, t, m, hb = spec["n"], spec["n_targ"], spec["n_max"], spec["half_band"]
row0, n_loc = shard_rows(n, world, rank)
ctx = capi.Context()
assert ctx.backend.startswith("hostsim" if spec["backend"] == "hostsim" else "hip:")
def hook(buf, op):
    tt = torch.from_numpy(buf)
    dist.all_reduce(tt, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
if world > 1 and spec["transport"] == "p2p":
    mine = ctx.p2p_export(world)
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    ctx.p2p_attach(world, rank, everyone)
elif world > 1:
    ctx.set_allreduce_hook(hook, world, rank)
if world > 1:
    ctx.set_shard(n, row0)
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
# a banded symmetric matrix: diag 2 + i / 50, off-diagonals 0.3 / d * cos(i + d), d = 1 .. half_band  (+ one far coupling on request)
i = np.arange(n, dtype=np.float64)
diags, offs = [2.0 + i / 50.0], [0]
for d in range(1, hb + 1):
    v = 0.3 / d * np.cos(i[:n - d] + d)
    if spec.get("ragged"):                  # the reach varies with the row: (r, r + d) is present iff d <= 1 + (r mod half_band), mirrored
        v = np.where(d <= 1 + (np.arange(n - d) % hb), v, 0.0)
    diags += [v, v]; offs += [d, -d]
if spec.get("reach"):                       # one more pair of diagonals far out: the halo has to be that wide
    d = spec["reach"]; v = 0.01 * np.cos(i[:n - d]); diags += [v, v]; offs += [d, -d]
a = sp.diags(diags, offs, shape=(n, n), format="lil")
if spec.get("far"):
    a[0, n - 1] = 0.1; a[n - 1, 0] = 0.1
a = a.tocsr()
a.eliminate_zeros()                         # (ragged: the rows really are of different lengths)
status = "ok"
try:
    ctx.spmm_setup_sharded(a[row0:row0 + n_loc], row0, n)
except Exception as e:
    status = "refused: " + str(e)
res = dict(status=status, row0=row0)
if status == "ok":
    x = np.asfortranarray(np.random.default_rng(3).standard_normal((n, m)))
    px = ctx.panel(np.asfortranarray(x[row0:row0 + n_loc])); pax = ctx.panel(n_loc, m); ppx = ctx.panel(n_loc, m)
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address("dla_spmm_matvec"), n_loc, m, px.ptr, pax.ptr))
    ctx._chk(ctx.lib.dla_call_precnd(ctx.h, capi.fn_address("dla_spmm_precnd"), n_loc, m, -1.25, px.ptr, ppx.ptr))
    ref = (a @ x)[row0:row0 + n_loc]
    den = a.diagonal()[row0:row0 + n_loc, None] - 1.25
    res["matvec_err"] = float(np.abs(pax.download() - ref).max() / np.abs(ref).max())
    xl = x[row0:row0 + n_loc]
    res["precnd_err"] = float(np.abs(ppx.download() - np.where(np.abs(den) > 1e-5, xl / den, xl)).max())
    res["ell_w"] = int(np.diff(a[row0:row0 + n_loc].indptr).max())
    g = np.zeros((n_loc, m), order="F")
    for j in range(m):
        if row0 <= j < row0 + n_loc: g[j - row0, j] = 1.0
    ev = ctx.panel(g)
    mv, pc = capi.fn_address("dla_spmm_matvec"), capi.fn_address("dla_spmm_precnd")
    eig, _, ok, info = ctx.davidson_driver(n_loc, t, m, 300, spec["tol"], 20, 0.0, mv, pc, ev)
    res.update(ok=bool(ok), iters=int(info["iters"]), allreduces=int(ctx.stats()["allreduces"]))
    np.savez(os.path.join({out!r}, f"rank{{rank}}.npz"), eig=eig, vec=ev.download())
json.dump(res, open(os.path.join({out!r}, f"rank{{rank}}.json"), "w"))
dist.barrier()
if world > 1 and spec["transport"] == "p2p":
    ctx.comm_finalize()
dist.destroy_process_group()
"""


def _run_world(tmp_path, spec, world):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, spec=json.dumps(spec), out=str(tmp_path)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    res = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(world)]
    npz = [np.load(tmp_path / f"rank{r}.npz") if os.path.exists(tmp_path / f"rank{r}.npz") else None for r in range(world)]
    return res, npz


def _dense_lowest(spec):
    n, hb = spec["n"], spec["half_band"]
    i = np.arange(n, dtype=np.float64)
    a = np.diag(2.0 + i / 50.0)
    for d in range(1, hb + 1):
        v = 0.3 / d * np.cos(i[:n - d] + d)
        if spec.get("ragged"):
            v = np.where(d <= 1 + (np.arange(n - d) % hb), v, 0.0)
        a += np.diag(v, d) + np.diag(v, -d)
    return np.linalg.eigvalsh(a)[:spec["n_targ"]]


def _check(tmp_path, spec, world):
    d1 = tmp_path / "w1"; d1.mkdir()
    dn = tmp_path / "wn"; dn.mkdir()
    (one,), (v1,) = _run_world(d1, spec, 1)
    many, vn = _run_world(dn, spec, world)
    t = spec["n_targ"]
    for r in [one] + many:
        assert r["status"] == "ok", r
        assert r["matvec_err"] < 1e-14 and r["precnd_err"] < 1e-13, r
        assert r["ok"]
    assert one["allreduces"] == 0 and all(r["allreduces"] > 0 for r in many)
    assert len({r["iters"] for r in many}) == 1                              # identical decisions on every rank
    assert all(np.array_equal(vn[0]["eig"], v["eig"]) for v in vn)
    assert abs(many[0]["iters"] - one["iters"]) <= max(1, one["iters"] // 10)
    assert np.allclose(vn[0]["eig"][:t], v1["eig"][:t], rtol=1e-10, atol=0)
    if spec["n"] <= 4000:
        assert np.allclose(v1["eig"][:t], _dense_lowest(spec), rtol=1e-8, atol=0)
    stitched = np.vstack([v["vec"] for v in vn])
    sgn = np.sign((stitched * v1["vec"]).sum(0))
    assert np.abs(stitched * sgn - v1["vec"])[:, :t].max() < 1e-6
    return many


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_banded_operator_gloo(tmp_path, world):
    """host-memory engine, reduction hook over gloo: 2 and 3 ranks (a middle rank has two neighbours)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostsim
    hostsim.build()
    spec = dict(backend="hostsim", transport="hook", n=3000, n_targ=4, n_max=8, half_band=6, tol=1e-9)
    _check(tmp_path, spec, world)


def test_sharded_ragged_operator_three_ranks_gloo(tmp_path):
    """host-memory engine, 3 ranks: a symmetric pattern whose reach depends on the row, so the ranks need halos of different widths
    (the agreed halo is the widest) and the rows are of different lengths"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostsim
    hostsim.build()
    spec = dict(backend="hostsim", transport="hook", n=3000, n_targ=4, n_max=8, half_band=6, tol=1e-9, ragged=True)
    _check(tmp_path, spec, 3)


def test_sharded_operator_refuses_long_range_couplings_on_every_rank(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hostsim
    hostsim.build()
    spec = dict(backend="hostsim", transport="hook", n=20000, n_targ=4, n_max=8, half_band=2, tol=1e-9, far=True)
    res, _ = _run_world(tmp_path, spec, 2)
    assert all(r["status"].startswith("refused") for r in res), res


@pytest.mark.gpu
@pytest.mark.parametrize("transport", ["hook", "p2p"])
def test_sharded_banded_operator_two_ranks_on_one_gpu(tmp_path, transport):
    spec = dict(backend="hip", transport=transport, n=200_000, n_targ=6, n_max=10, half_band=6, tol=1e-9)
    _check(tmp_path, spec, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("half_band,ragged,ell_w", [(1, False, 3), (3, False, 7), (12, False, 25), (12, True, 20)])
def test_sharded_banded_operator_three_ranks_on_one_gpu(tmp_path, half_band, ragged, ell_w):
    """Three ranks share one GPU over the reduction hook: the middle rank reads a `prev` AND a `next` halo.  w = 3, 7, 25 are the
    halo kernel's width buckets 4, 8, 32 (the two-rank legs above run w = 13: bucket 16); `ragged` gives rows of 2 .. 20 entries
    and ranks that need halos of 8, 8 and 10 rows."""
    spec = dict(backend="hip", transport="hook", n=30_000, n_targ=4, n_max=8, half_band=half_band, tol=1e-9, ragged=ragged)
    many = _check(tmp_path, spec, 3)
    assert max(r["ell_w"] for r in many) == ell_w, many


@pytest.mark.gpu
def test_sharded_operator_wide_block_exchanges_in_column_chunks(tmp_path):
    """halo 40 rows x 2 ranks x 2 sides: a 13-column block needs 2080 doubles per exchange, a 120-row halo with 37 columns does
    not fit one mailbox slot (16384) -- the product goes through in column chunks"""
    spec = dict(backend="hip", transport="p2p", n=100_000, n_targ=8, n_max=37, half_band=120, tol=1e-9)
    _check(tmp_path, spec, 2)


@pytest.mark.gpu
def test_sharded_operator_refuses_a_halo_beyond_a_mailbox_slot_on_every_rank(tmp_path):
    """Round-4 advisor: three ranks on the peer-to-peer mailboxes and a 3000-row halo need 3 x 2 x 3000 = 18000 doubles per column,
    more than a slot (16384): every rank refuses the layout at setup (nothing is left waiting in an exchange)."""
    spec = dict(backend="hip", transport="p2p", n=30_000, n_targ=2, n_max=4, half_band=2, reach=3000, tol=1e-6)
    res, _ = _run_world(tmp_path, spec, 3)
    assert all(r["status"].startswith("refused") and "mailbox slot" in r["status"] for r in res), res
