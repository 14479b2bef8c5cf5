"""CPU: the stored layout of the dense operator and the plan of its product (dense_pack, dense_index, dense_plan in
diaglib_amd/csrc/hip_plans.h; the contract: include/diaglib_amd.h, dla_dense_setup).

tests/dense_layout_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_sell_layout.py builds its driver): it packs a matrix with the product's own code and multiplies by walking the stored
array the way the kernels do -- tile order, chunk order, combine order.  Matrices and blocks hold small integers (entries in
[-8, 8]), for which every order of summation is exact: the product must equal NumPy's bit for bit.  The plan is held against a
transcription of the planner's rule."""
import os
import subprocess

import numpy as np
import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "dense_layout_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "dense_layout_driver")
TILE, GROUP, WAVE_TILES, MAX_COLS, MIN_CHUNK_GROUPS, WS_SHARE = 16, 8, 4, 48, 8, 8
SIZES = [1, 15, 16, 17, 63, 65, 130, 1000]
WIDTHS = [1, 8, 16, 17, 48, 49]


def planner_rule(ncu, n, m):
    """dense_plan, transcribed from its comment: (k_chunks, chunk_groups, groups, row_groups, what bounded the split)"""
    n_pad = -(-n // TILE) * TILE
    groups, row_groups = n_pad // GROUP, -(-(n_pad // TILE) // WAVE_TILES)
    bounds = {"want": -(-4 * ncu // row_groups), "traffic": n // (2 * WS_SHARE * m), "length": groups // MIN_CHUNK_GROUPS}
    chunks = max(1, min(bounds.values()))
    chunk_groups = -(-groups // chunks)
    return -(-groups // chunk_groups), chunk_groups, groups, row_groups, bounds


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("dense")

    def run(a, lda, x, ncu):
        n, m = x.shape
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        held = np.full((lda, n), 77.0, order="F")       # (rows n .. lda - 1 of the caller's array must never be read into the copy)
        held[:n, :] = a
        with open(fin, "wb") as f:
            np.array([n, lda, m, ncu], np.int64).tofile(f)
            held.T.tofile(f)
            np.asfortranarray(x, np.float64).T.tofile(f)
        p = subprocess.run([EXE, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        raw = open(fout, "rb").read()
        at = 0

        def take(dtype, count):
            nonlocal at
            v = np.frombuffer(raw, dtype, count, at)
            at += v.nbytes
            return v
        out = dict(zip(("n_pad", "row_tile", "bad_pad", "bad_value", "bad_roundtrip", "passes"), (int(v) for v in take(np.int64, 6))))
        names = ("m", "acc_groups", "k_chunks", "chunk_groups", "groups", "row_groups", "ws_doubles")
        out["plans"] = [dict(zip(names, (int(v) for v in take(np.int64, 7)))) for _ in range(out["passes"])]
        out["y"] = take(np.float64, n * m).reshape(m, n).T
        out["diag"] = take(np.float64, n)
        out["writes"] = take(np.int32, n * m)
        out["ws_writes_bad"] = int(take(np.int64, 1)[0])
        assert at == len(raw)
        return out
    return run


@pytest.mark.parametrize("n", SIZES)
def test_the_stored_layout_multiplies_exactly_and_the_plan_follows_its_rule(driver, n):
    rng = np.random.default_rng(1000 + n)
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)        # not symmetric: row i of the result is row i of a
    for lda in (n, n + 3):
        for m in WIDTHS:
            x = rng.integers(-8, 9, (n, m)).astype(np.float64)
            for ncu in ((256, 8) if m in (1, 48) else (256,)):
                out = driver(a, lda, x, ncu)
                tag = f"n={n} lda={lda} m={m} ncu={ncu}"
                # ---- the copy: every element where the index map says, padding +0.0, nothing of rows n .. lda - 1
                assert out["n_pad"] == -(-n // TILE) * TILE and out["row_tile"] == TILE * WAVE_TILES, tag
                assert (out["bad_pad"], out["bad_value"], out["bad_roundtrip"]) == (0, 0, 0), tag
                assert np.array_equal(out["diag"], np.diag(a)), tag
                # ---- the product, bit for bit, every element stored once, every workspace element written once
                assert np.array_equal(out["y"], a @ x), tag
                assert np.all(out["writes"] == 1) and out["ws_writes_bad"] == 0, tag
                # ---- the plan of every pass
                widths = [min(MAX_COLS, m - c0) for c0 in range(0, m, MAX_COLS)]
                assert [p["m"] for p in out["plans"]] == widths, tag
                for p in out["plans"]:
                    k_chunks, chunk_groups, groups, row_groups, bounds = planner_rule(ncu, n, p["m"])
                    assert (p["k_chunks"], p["chunk_groups"], p["groups"], p["row_groups"]) == (k_chunks, chunk_groups, groups, row_groups), (tag, p)
                    assert p["acc_groups"] == -(-p["m"] // 16), (tag, p)
                    # the chunks [8 c chunk_groups, min(n_pad, 8 (c + 1) chunk_groups)) cover [0, n_pad) once: ascending starts,
                    # none empty, the last one ends at n_pad; boundaries are multiples of 4
                    starts = [GROUP * c * p["chunk_groups"] for c in range(p["k_chunks"])]
                    ends = [min(out["n_pad"], s + GROUP * p["chunk_groups"]) for s in starts]
                    assert starts[0] == 0 and ends[-1] == out["n_pad"] and starts[1:] == ends[:-1], (tag, p)
                    assert all(s < e and s % 4 == 0 and e % 4 == 0 for s, e in zip(starts, ends)), (tag, p)
                    assert p["ws_doubles"] == (p["k_chunks"] * p["m"] * n if p["k_chunks"] > 1 else 0), (tag, p)
                    # one chunk wherever a bound of the rule says so; a split keeps the workspace traffic within its share
                    if min(bounds.values()) <= 1:
                        assert p["k_chunks"] == 1, (tag, p, bounds)
                    if p["k_chunks"] > 1:
                        assert 2 * p["k_chunks"] * n * p["m"] * 8 * WS_SHARE <= 8 * n * n, (tag, p)
                        assert p["chunk_groups"] >= MIN_CHUNK_GROUPS, (tag, p)


def test_the_planner_splits_where_the_rule_allows_it():
    """the shapes above must not all be one-chunk cases: n = 1000 splits for a narrow block and does not for a wide one"""
    assert planner_rule(256, 1000, 1)[0] > 1 and planner_rule(256, 1000, 8)[0] > 1
    assert planner_rule(256, 1000, 48)[0] == 1 and planner_rule(256, 65, 1)[0] == 1
    assert planner_rule(256, 32768, 37)[0] > 1 and planner_rule(256, 2000, 48)[0] > 1 and planner_rule(256, 65536, 8)[0] == 1
