"""CPU: dense_t_plan (diaglib_amd/csrc/hip_plans.h), the split of the rows of y = A^T x over workgroups (include/diaglib_amd.h,
dla_dense_matvec_t).  tests/dense_t_plan_driver.cpp is a stand-alone program, compiled with g++, no ROCm include and
-fsanitize=address,undefined; expected values are the rule the planner's comment states, transcribed below."""
import os
import subprocess

import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "dense_t_plan_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "dense_t_plan_driver")
NS = [1, 15, 16, 17, 63, 64, 65, 130, 257, 1024, 2048, 8192, 32768, 100003]
MS = [1, 8, 13, 16, 17, 37, 48]
NCUS = [1, 64, 256, 304]
# DENSE_T_WAVE_BLOCKS, DENSE_T_MIN_CHUNK_TILES, DENSE_WS_SHARE of hip_plans.h (the driver prints them: held against these below)
CONSTANTS = dict(wave_blocks=4, min_chunk_tiles=4, ws_share=8)


def run_plans(requests):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([EXE], input="".join("%d %d %d\n" % r for r in requests), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    out = []
    for ln in p.stdout.splitlines():
        fields, _, name = ln.partition(" | ")
        out.append(({k: int(v) for k, v in (kv.split("=") for kv in fields.split())}, name))
    assert len(out) == len(requests)
    return out


def rule(ncu, n, m, wave_blocks=CONSTANTS["wave_blocks"], min_chunk_tiles=CONSTANTS["min_chunk_tiles"], ws_share=CONSTANTS["ws_share"]):
    """the planner's comment, transcribed: (row_chunks, chunk_tiles, strips, what bounded the split)"""
    n_pad = (n + 15) // 16 * 16
    row_tiles = n_pad // 16
    strips = -(-(n_pad // 16) // wave_blocks)
    bounds = {"simds": -(-4 * ncu // strips), "traffic": n // (2 * ws_share * m), "length": row_tiles // min_chunk_tiles}
    chunks = max(1, min(bounds.values()))
    chunk_tiles = -(-row_tiles // chunks)
    return -(-row_tiles // chunk_tiles), chunk_tiles, strips, bounds


@pytest.fixture(scope="module")
def plans():
    req = [(c, n, m) for c in NCUS for n in NS for m in MS]
    return dict(zip(req, run_plans(req)))


def test_plan_follows_the_stated_rule_and_covers_every_row_once(plans):
    for (ncu, n, m), (p, name) in plans.items():
        assert {k: p[k] for k in CONSTANTS} == CONSTANTS
        chunks, chunk_tiles, strips, _ = rule(ncu, n, m)
        assert p["n_pad"] == (n + 15) // 16 * 16 and p["row_tiles"] == p["col_blocks"] == p["n_pad"] // 16
        assert (p["row_chunks"], p["chunk_tiles"], p["strips"]) == (chunks, chunk_tiles, strips), (ncu, n, m, p)
        # chunk c covers the row tiles [c chunk_tiles, min(row_tiles, (c + 1) chunk_tiles)): disjoint, none empty, all tiles
        covered = []
        for c in range(p["row_chunks"]):
            lo, hi = c * p["chunk_tiles"], min(p["row_tiles"], (c + 1) * p["chunk_tiles"])
            assert lo < hi
            covered += range(lo, hi)
        assert covered == list(range(p["row_tiles"]))
        # ... and the strips cover every block of 16 output indices
        assert (p["strips"] - 1) * p["wave_blocks"] < p["col_blocks"] <= p["strips"] * p["wave_blocks"]
        assert p["acc_groups"] == -(-m // 16) and name == "dense_t_mfma_kernel<%d>" % p["acc_groups"]
        assert p["ws_doubles"] == (p["row_chunks"] * m * n if p["row_chunks"] > 1 else 0)


def test_plan_splits_where_the_rule_says_and_not_where_it_says_not(plans):
    split = {k: p["row_chunks"] for k, (p, _) in plans.items()}
    # few strips, many rows, a narrow block: the rows are split ...
    assert split[(256, 1024, 1)] == 16 and split[(256, 1024, 8)] == 8        # bounded by the chunk length, by the workspace traffic
    assert split[(256, 8192, 8)] == 8                                         # bounded by the SIMDs to fill: 1024 / 128 strips
    # ... a wide block would move more partial sums than 1 / 8 of the matrix: not split
    assert split[(256, 1024, 48)] == 1 and split[(256, 1024, 37)] == 1
    # a matrix of a few tiles has no chunk of 4 tiles to give away
    assert all(split[(256, n, m)] == 1 for n in (1, 15, 16, 17, 63) for m in MS)
    # enough strips for every SIMD: not split
    assert split[(64, 32768, 8)] == 1 and split[(1, 1024, 1)] == 1
    # the bound in force is the smallest of the three
    for (ncu, n, m), (p, _) in plans.items():
        _, _, _, bounds = rule(ncu, n, m, p["wave_blocks"], p["min_chunk_tiles"], p["ws_share"])
        if p["row_chunks"] > 1:
            assert p["row_chunks"] <= min(bounds.values())
            assert 2 * p["row_chunks"] * n * m * 8 * p["ws_share"] <= 8 * n * n      # the partial sums' traffic against the matrix
            assert p["chunk_tiles"] >= p["min_chunk_tiles"]


def test_plan_is_a_pure_function(plans):
    req = list(plans)[::7]
    assert run_plans(req) == [plans[r] for r in req]
    assert run_plans(list(reversed(req))) == [plans[r] for r in reversed(req)]
