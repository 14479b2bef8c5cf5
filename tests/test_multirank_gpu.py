"""GPU: the row-sharded path of the HIP engine on real hardware with TWO ranks sharing one GPU.
RCCL refuses two ranks on one device, so the small cross-rank sums travel either
  * through the dla_set_allreduce_hook door over gloo ("hook": host round trip per reduction, host-driven ortho loops), or
  * through the one-shot peer-to-peer all-reduce over hipIpc mailboxes ("p2p", SURVEY 8f row 2: device-to-device, fixed
    summation order, part of the device-driven orthogonalisation chains -- the transport meant for the 8-GPU runs).
Every reduction point of the engine (Gram / fused Gram / Ritz norms / nrm2 / the operator's r x m product), the shard
offsets of the generator and of the built-in operator, and the replicated small-matrix logic are the same code that runs
under RCCL (whose transport is exercised by tests/test_solver_gpu.py::test_rccl_communicator_single_rank)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, json
os.environ.setdefault("OMP_NUM_THREADS", "2")
sys.path.insert(0, {root!r})
import numpy as np
from diaglib_amd import capi
import torch, torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
from bench import shard_rows
spec = json.loads({spec!r})
n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
row0, n_loc = shard_rows(n, world, rank)
ctx = capi.Context()
assert ctx.backend.startswith("hip:")
def hook(buf, op):
    tt = torch.from_numpy(buf)
    dist.all_reduce(tt, op=dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX)
if world > 1 and spec.get("transport", "hook") == "p2p":
    mine = ctx.p2p_export(world)
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    ctx.p2p_attach(world, rank, everyone)
    ctx.set_shard(n, row0)
elif world > 1 and spec.get("transport") == "rccl":
    uid = [ctx.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(uid, src=0)
    ctx.comm_init(world, rank, uid[0])
    ctx.set_shard(n, row0)
elif world > 1:
    ctx.set_allreduce_hook(hook, world, rank)
    ctx.set_shard(n, row0)
ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
ctx.synth_setup(n, row0, n_loc)
g = np.zeros((n_loc, m), order="F")
if spec["guess"] == "unit":
    for j in range(m):
        if row0 <= j < row0 + n_loc: g[j - row0, j] = 1.0
ev = ctx.panel(g)
mv, pc = capi.fn_address("dla_synth_matvec"), capi.fn_address("dla_synth_precnd")
extra = dict()
if spec["solver"] == "ortho_then_reduce":
    # ortho_vs_x of a shape this context has not seen (its launch paths are walked without launching, then the chain runs) and,
    # with no other reduction in between, the norm and the Gram matrix of the block it left
    mm, kk = spec["m"], spec["k"]
    rs = np.random.default_rng(7)
    xu = np.hstack([np.linalg.qr(rs.standard_normal((n, mm)))[0], rs.standard_normal((n, kk))])
    big = ctx.panel(np.asfortranarray(xu[row0:row0 + n_loc]))
    pu = big.col(mm, kk)
    ctx.ortho_vs_x(big.col(0, mm), pu)
    extra = dict(nrm2=ctx.nrm2(pu), gram=ctx.gram(pu, pu))
    eig, ok, info = np.zeros(m), True, dict(iters=0, matvec_cols=0)
elif spec["solver"] == "check_guess":
    # zero guess -> library-generated random block (global row indices) + sharded ortho_cd
    ctx.check_guess(ev)
    eig, ok, info = np.zeros(m), True, dict(iters=0, matvec_cols=0)
elif spec["solver"] == "davidson":
    eig, _, ok, info = ctx.davidson_driver(n_loc, t, m, 200, spec["tol"], 20, 0.0, mv, pc, ev)
elif spec["solver"] == "gen_david":
    eig, _, ok, info = ctx.gen_david_driver(n_loc, t, m, 200, spec["tol"], 20, 0.0, mv, pc, capi.fn_address("dla_synth_metric"), ev)
elif spec["solver"] == "gen_lobpcg":
    eig, _, ok, info = ctx.lobpcg_driver(n_loc, t, m, 200, spec["tol"], 0.0, mv, pc, ev, bvec=capi.fn_address("dla_synth_metric"))
else:
    eig, _, ok, info = ctx.lobpcg_driver(n_loc, t, m, 200, spec["tol"], 0.0, mv, pc, ev)
st = ctx.stats()
np.savez(os.path.join({out!r}, f"rank{{rank}}.npz"), eig=eig, ok=ok, iters=info["iters"], cols=info["matvec_cols"],
         row0=row0, vec=ev.download(), allreduces=st["allreduces"], host_syncs=st["host_syncs"], **extra)
dist.barrier()
if world > 1 and spec.get("transport", "hook") in ("p2p", "rccl"):
    ctx.comm_finalize()
dist.destroy_process_group()
"""


def _run_world(tmp_path, spec, world, one_gpu_each=False):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, spec=json.dumps(spec), out=str(tmp_path)))
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LOCAL_RANK=str(r) if one_gpu_each else "0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=900) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    return [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]


def oracle_run(oracle, spec):
    """The same problem through the oracle (the C restatement of the reference's drivers, pinned to the reference by
    tests/test_oracle.py) on ONE rank, with the oracle's own restatement of the built-in operators: what every multi-rank result is
    measured against -- SURVEY 8(e): eigenvalues to 1e-11 relative against the 1-rank reference result, iteration counts reported.
    Returns (eigenvalues, eigenvectors, ok, iterations)."""
    n, t, m = spec["n"], spec["n_targ"], spec["n_max"]
    oracle.synth_setup(n, 0, n)
    g = np.zeros((n, m), order="F")
    g[np.arange(m), np.arange(m)] = 1.0
    mv, pc, bv = oracle.fn("orc_synth_matvec"), oracle.fn("orc_synth_precnd"), oracle.fn("orc_synth_metric")
    s = spec["solver"]
    if s == "davidson":
        e, v, ok, tr = oracle.davidson(n, t, m, 200, spec["tol"], 20, 0.0, mv, pc, g)
    elif s == "gen_david":
        e, v, ok, tr = oracle.gen_davidson(n, t, m, 200, spec["tol"], 20, 0.0, mv, pc, bv, g)
    elif s == "gen_lobpcg":
        e, v, ok, tr = oracle.lobpcg_gen(n, t, m, 200, spec["tol"], 0.0, mv, pc, bv, g)
    else:
        e, v, ok, tr = oracle.lobpcg(n, t, m, 200, spec["tol"], 0.0, mv, pc, g)
    return e, v, ok, tr.iters


def assert_parity_with_oracle(oracle, spec, ranks, iters_slack=None):
    """ranks: the per-rank results of a multi-rank run.  Eigenvalues rtol 1e-11 against the oracle's, iteration count within the
    margin the single-rank GPU path is held to against the oracle (the counts on this operator depend on last-bit
    differences of the Gram sums; +-20 %, at least one), eigenvectors up to sign."""
    t = spec["n_targ"]
    eo, vo, oko, ito = oracle_run(oracle, spec)
    assert oko
    assert np.allclose(ranks[0]["eig"][:t], eo[:t], rtol=1e-11, atol=0), (ranks[0]["eig"][:t], eo[:t])
    slack = iters_slack if iters_slack is not None else max(1, ito // 5)
    assert abs(int(ranks[0]["iters"]) - ito) <= slack, (int(ranks[0]["iters"]), ito)
    v = np.vstack([r["vec"] for r in ranks])
    sgn = np.sign((vo * v).sum(0))
    assert np.abs(v * sgn - vo)[:, :t].max() < 1e-6
    return ito


@pytest.mark.parametrize("transport", ["hook", "p2p"])
@pytest.mark.parametrize("solver,guess", [("davidson", "unit"), ("lobpcg", "unit"), ("check_guess", "zero"),
                                          ("gen_david", "unit"), ("gen_lobpcg", "unit")])
def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path, oracle, solver, guess, transport):
    spec = dict(n=200_000, n_targ=8, n_max=13, tol=1e-10, solver=solver, guess=guess, transport=transport)
    d1 = tmp_path / "w1"; d1.mkdir()
    d2 = tmp_path / "w2"; d2.mkdir()
    one = _run_world(d1, spec, 1)[0]
    two = _run_world(d2, spec, 2)
    t = spec["n_targ"]
    if solver == "check_guess":
        v2 = np.vstack([two[0]["vec"], two[1]["vec"]]); v1 = one["vec"]
        assert np.abs(v2 - v1).max() < 1e-12                         # same random stream, same orthonormalisation
        assert np.abs(v2.T @ v2 - np.eye(v2.shape[1])).max() < 1e-13
        assert int(two[0]["allreduces"]) > 0
        # ... and against the oracle's check_guess on the zero guess: the documented generator + ortho_cd (reference :3749-3757)
        assert np.abs(v2 - oracle.check_guess(np.zeros((spec["n"], spec["n_max"]), order="F"))).max() < 1e-12
        return
    assert bool(one["ok"]) and all(bool(r["ok"]) for r in two)
    assert int(two[0]["iters"]) == int(two[1]["iters"]) and int(two[0]["cols"]) == int(two[1]["cols"])
    assert np.array_equal(two[0]["eig"], two[1]["eig"])            # identical decisions on both ranks
    assert int(two[0]["allreduces"]) > 0 and int(one["allreduces"]) == 0
    if transport == "p2p":
        # device-to-device reductions keep the orthogonalisation chains on the device: about as many host waits as one rank
        assert int(two[0]["host_syncs"]) <= int(one["host_syncs"]) + 8, (int(two[0]["host_syncs"]), int(one["host_syncs"]))
    assert np.allclose(two[0]["eig"][:t], one["eig"][:t], rtol=1e-11, atol=0)
    assert abs(int(two[0]["iters"]) - int(one["iters"])) <= max(1, int(one["iters"]) // 5)
    v2 = np.vstack([two[0]["vec"], two[1]["vec"]])
    assert int(two[1]["row0"]) == two[0]["vec"].shape[0]
    v1 = one["vec"]
    sgn = np.sign((v1 * v2).sum(0))
    assert np.abs(v2 * sgn - v1)[:, :t].max() < 1e-6
    if not solver.startswith("gen_"):          # (with a metric the vectors are B-orthonormal)
        assert np.abs(v2[:, :t].T @ v2[:, :t] - np.eye(t)).max() < 1e-12
    assert_parity_with_oracle(oracle, spec, two)   # ... and the 2-rank result against the oracle, not only against this engine


@pytest.mark.parametrize("solver", ["davidson", "lobpcg"])
def test_two_ranks_wide_blocks_peer_to_peer(tmp_path, oracle, solver):
    """Blocks of 21 columns (two column tiles: the LDS-loop k x k step, the one-sweep X^T U + U^T U and the storing sweep OP_XW)
    with the cross-rank sum inside the reduction kernels: two ranks on one GPU over the peer-to-peer mailboxes against one rank."""
    spec = dict(n=120_000, n_targ=16, n_max=21, tol=1e-10, solver=solver, guess="unit", transport="p2p")
    d1 = tmp_path / "w1"; d1.mkdir()
    d2 = tmp_path / "w2"; d2.mkdir()
    one = _run_world(d1, spec, 1)[0]
    two = _run_world(d2, spec, 2)
    t = spec["n_targ"]
    assert bool(one["ok"]) and all(bool(r["ok"]) for r in two)
    assert int(two[0]["iters"]) == int(two[1]["iters"]) and np.array_equal(two[0]["eig"], two[1]["eig"])
    assert np.allclose(two[0]["eig"][:t], one["eig"][:t], rtol=1e-11, atol=0)
    assert abs(int(two[0]["iters"]) - int(one["iters"])) <= max(1, int(one["iters"]) // 5)
    assert int(two[0]["host_syncs"]) <= int(one["host_syncs"]) + 10, (int(two[0]["host_syncs"]), int(one["host_syncs"]))
    v2 = np.vstack([two[0]["vec"], two[1]["vec"]]); v1 = one["vec"]
    sgn = np.sign((v1 * v2).sum(0))
    assert np.abs(v2 * sgn - v1)[:, :t].max() < 1e-6
    assert np.abs(v2[:, :t].T @ v2[:, :t] - np.eye(t)).max() < 1e-12
    assert_parity_with_oracle(oracle, spec, two)


def test_reductions_right_behind_a_first_chain_peer_to_peer(tmp_path):
    """The first ortho_vs_x of an (m, k) shape walks its launch paths without launching and then runs the chain, whose reductions
    carry the cross-rank sum inside the reduction kernel.  Neither may leave anything behind for the next reduction: the norm
    (its own kernels, then the exchange as a launch) and the Gram matrix of the block must still be summed over both ranks.
    A sum that was skipped gives each rank its own half: different bits, norm^2 and diagonal far from k and 1.
    Tolerances: the orthonormality bound of tests/test_ortho_chain_gpu.py, 50 eps per entry of U^T U - I; norm^2 is the sum of
    the k diagonal entries, hence k times that."""
    eps = np.finfo(np.float64).eps
    k = 8
    spec = dict(n=2048, n_targ=1, n_max=1, m=16, k=k, solver="ortho_then_reduce", guess="zero", transport="p2p")
    two = _run_world(tmp_path, spec, 2)
    assert np.array_equal(two[0]["nrm2"], two[1]["nrm2"])          # the exchange has a fixed summation order
    assert np.array_equal(two[0]["gram"], two[1]["gram"])
    assert abs(float(two[0]["nrm2"]) ** 2 - k) < k * 50 * eps, float(two[0]["nrm2"]) ** 2 - k
    assert np.abs(two[0]["gram"] - np.eye(k)).max() < 50 * eps, np.abs(two[0]["gram"] - np.eye(k)).max()
    assert int(two[0]["allreduces"]) == int(two[1]["allreduces"]) > 0


@pytest.mark.parametrize("world,solver", [(3, "davidson"), (4, "lobpcg"), (4, "gen_david")])
def test_odd_row_count_on_three_and_four_ranks(tmp_path, oracle, world, solver):
    """An odd n leaves ONE rank with an odd shard: that rank cannot use the 16-byte sweeps, and before r04 it also chose another
    orthogonalisation schedule than its peers -- the exchanges no longer paired up (three ranks waited for a peer, the fourth
    factorised garbage; found by tools/fuzz_multirank.py).  The ranks now agree on the schedule when the shards are announced
    (dla_set_shard): every rank takes the same sweeps, identical bits, the single-rank result."""
    spec = dict(n=95_775, n_targ=4, n_max=9, tol=1e-9, solver=solver, guess="unit", transport="p2p")
    d1 = tmp_path / "w1"; d1.mkdir()
    dn = tmp_path / "wn"; dn.mkdir()
    one = _run_world(d1, spec, 1)[0]
    many = _run_world(dn, spec, world)
    t = spec["n_targ"]
    assert bool(one["ok"]) and all(bool(r["ok"]) for r in many)
    assert all(np.array_equal(many[0]["eig"], r["eig"]) and int(r["iters"]) == int(many[0]["iters"]) for r in many)
    assert np.allclose(many[0]["eig"][:t], one["eig"][:t], rtol=1e-11, atol=0)
    assert abs(int(many[0]["iters"]) - int(one["iters"])) <= max(1, int(one["iters"]) // 5)
    v = np.vstack([r["vec"] for r in many]); v1 = one["vec"]
    assert v.shape == v1.shape and many[-1]["vec"].shape[0] % 2 == 1          # (the last shard is the odd one)
    sgn = np.sign((v1 * v).sum(0))
    assert np.abs(v * sgn - v1)[:, :t].max() < 1e-6
    assert_parity_with_oracle(oracle, spec, many)


def test_linear_response_drivers_on_row_shards():
    """caslr_eff_driver / caslr_driver on 2, 3 (odd n) and 4 ranks sharing the GPU, peer-to-peer mailboxes, built-in LR operators:
    identical bits on every rank, the single-rank eigenvalues and iteration count (tools/multirank_lr_probe.py)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "multirank_lr_probe.py")], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0 and "linear-response drivers on row shards: ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])


def test_empty_shard_is_refused_on_every_rank(tmp_path):
    """300 rows over four ranks in 64-row multiples leave the last rank without rows: every rank learns the layout when the
    shards are announced and refuses it at once (before r04 the empty rank failed in its first launch and the others waited
    for the peer-to-peer timeout)."""
    import socket
    spec = dict(n=300, n_targ=2, n_max=4, tol=1e-8, solver="davidson", guess="unit", transport="p2p")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, spec=json.dumps(spec), out=str(tmp_path)))
    procs = []
    for r in range(4):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="4", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode != 0 and "a rank holds no rows" in e, e[-1500:]


def test_two_gpus_rccl_equal_one_rank(tmp_path):
    """the RCCL data path with more than one rank -- one rank per GPU, ncclAllReduce on the engines' streams,
    device-driven chains with the collective between reduction and tail.  Needs two visible GPUs (skipped on the
    one-GPU boxes this suite normally runs on)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    spec = dict(n=400_000, n_targ=8, n_max=13, tol=1e-10, solver="davidson", guess="unit", transport="rccl")
    d1 = tmp_path / "w1"; d1.mkdir()
    d2 = tmp_path / "w2"; d2.mkdir()
    one = _run_world(d1, spec, 1)[0]
    two = _run_world(d2, spec, 2, one_gpu_each=True)
    t = spec["n_targ"]
    assert bool(one["ok"]) and all(bool(r["ok"]) for r in two)
    assert np.array_equal(two[0]["eig"], two[1]["eig"])
    assert np.allclose(two[0]["eig"][:t], one["eig"][:t], rtol=1e-11, atol=0)
    assert int(two[0]["iters"]) == int(two[1]["iters"])
    assert abs(int(two[0]["iters"]) - int(one["iters"])) <= max(1, int(one["iters"]) // 5)


TIMEOUT_WORKER = r"""
import os, sys, time
sys.path.insert(0, {root!r})
import numpy as np
from diaglib_amd import capi
import torch.distributed as dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
ctx = capi.Context()
mine = ctx.p2p_export(world)
everyone = [None] * world
dist.all_gather_object(everyone, mine)
ctx.p2p_attach(world, rank, everyone)
ctx.set_option(capi.OPT_P2P_TIMEOUT_MS, 400)
probe = ctx.panel(np.full((64, 2), float(rank + 1), order="F"))
got = ctx.gram(probe, probe)                      # one good exchange first
assert abs(got[0, 0] - 64.0 * sum((r + 1) ** 2 for r in range(world))) < 1e-9
dist.barrier()
if rank == {late}:
    time.sleep(2.0)                               # this rank withholds its contribution beyond the limit
t0 = time.time()
code = 0
try:
    ctx.gram(probe, probe)
except capi.DlaError as e:
    code = 3 if "status 7" in str(e) and "p2p" in str(e) else 4      # DLA_ERR_COMM
    print("FAILED", round(time.time() - t0, 2), str(e)[:120], flush=True)
    try:
        ctx.gram(probe, probe)                    # the transport stays down
        code = 5
    except capi.DlaError:
        pass
sys.exit(code)
"""


def test_p2p_rank_that_withholds_its_contribution_fails_every_rank(tmp_path):
    """ADVICE r02 / VERDICT r02 6(c): one rank arrives 2 s late at an exchange whose limit is 0.4 s (DLA_OPT_P2P_TIMEOUT_MS).
    The early rank gives up and marks the exchange as failed in every mailbox; the late rank -- which would find flag and data
    in place and succeed alone -- fails the SAME exchange.  Both return DLA_ERR_COMM within seconds, the transport stays down,
    every process exits non-zero on its own (fresh child processes)."""
    import time
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(TIMEOUT_WORKER.format(root=ROOT, late=1))
    procs = []
    t0 = time.time()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0",
                   DIAGLIB_AMD_SHARE_DEVICES="1")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=120) for p in procs]
    for r, (p, (o, e)) in enumerate(zip(procs, outs)):
        assert p.returncode == 3, (r, p.returncode, o[-500:], e[-1500:])
        assert "FAILED" in o
        took = float(o.split("FAILED")[1].split()[0])
        assert took < 5.0, (r, took)
