"""CPU: the triangular copy of a symmetric dense operator and the plan of its product (dense_sym_index, dense_sym_pack,
dense_sym_plan in diaglib_amd/csrc/hip_plans.h; the contract: include/diaglib_amd.h, dla_dense_setup_sym).

tests/dense_sym_layout_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_dense_operator_layout.py builds its driver): it packs one triangle of a matrix with the product's own code and multiplies
by walking the stored array the way the kernels do -- panel, chunk, wavefront order, combine order -- through the workspace at the
offsets the plan states.  Matrices and blocks hold small integers (entries in [-8, 8]), for which every order of summation is
exact: the product must equal NumPy's bit for bit.  The caller's unreferenced strict triangle and the rows n .. lda - 1 hold NaN:
neither the copy nor the product may hold one.  The plan is held against a transcription of the planner's rule."""
import os
import subprocess

import numpy as np
import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "dense_sym_layout_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "dense_sym_layout_driver")
TILE, PANEL_TILES, MAX_COLS, WS_SHARE, ITEMS_PER_CU = 16, 16, 48, 8, 4
SIZES = [1, 15, 16, 17, 63, 65, 130, 255, 257, 513, 1000]
WIDTHS = [1, 8, 16, 17, 48, 49]


def chunks_before(panel, cp):
    """the chunks of the panels below `panel`: panel P has P // cp + 1"""
    return sum(q // cp + 1 for q in range(panel))


def first_panel(nt, b):
    """the first panel with a tile below column block b (it and every later panel hold a transposed partial for b)"""
    return next((p for p in range(-(-nt // PANEL_TILES)) if min(PANEL_TILES * p + PANEL_TILES - 1, nt - 1) > b), -(-nt // PANEL_TILES))


def planner_rule(ncu, n, m):
    """dense_sym_plan, transcribed from its comment"""
    n_pad = -(-n // TILE) * TILE
    nt = n_pad // TILE
    panels = -(-nt // PANEL_TILES)
    last = panels - 1
    rows_last = n - 256 * last
    stored = 128 * nt * (nt + 1)

    def forward(cp):
        return m * (256 * chunks_before(last, cp) + (last // cp + 1) * rows_last)
    enough = [cp for cp in range(1, panels + 1) if chunks_before(panels, cp) >= ITEMS_PER_CU * ncu]
    cp = max(enough) if enough else 1
    while cp < panels and 16 * forward(cp) * WS_SHARE > 8 * stored:
        cp += 1
    t_blocks = sum(min(PANEL_TILES * p + PANEL_TILES - 1, nt - 1) for p in range(panels))
    out = {"m": m, "acc_groups": -(-m // 16), "panels": panels, "chunk_panels": cp, "chunk_blocks": PANEL_TILES * cp, "max_chunks": last // cp + 1,
           "items": chunks_before(panels, cp),
           "max_partials": max(b // PANEL_TILES // cp + 1 + panels - first_panel(nt, b) for b in range(nt)),
           "t_base": forward(cp) if nt > 1 else 0, "ws_doubles": forward(cp) + 16 * m * t_blocks if nt > 1 else 0}
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("dense_sym")

    def run(a, lda, x, ncu, uplo):
        n, m = x.shape
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        held = np.full((lda, n), np.nan, order="F")      # rows n .. lda - 1 and the other strict triangle must never be read
        held[:n, :] = np.tril(a) if uplo == "L" else np.triu(a)
        other = np.triu_indices(n, 1) if uplo == "L" else np.tril_indices(n, -1)
        held[:n, :][other] = np.nan
        with open(fin, "wb") as f:
            np.array([n, lda, m, ncu, ord(uplo)], np.int64).tofile(f)
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
        out = dict(zip(("n_pad", "stored", "bad_pad", "bad_value", "bad_roundtrip", "bad_index", "nan_stored", "passes"), (int(v) for v in take(np.int64, 8))))
        names = ("m", "acc_groups", "panels", "chunk_panels", "chunk_blocks", "max_chunks", "items", "max_partials", "t_base", "ws_doubles",
                 "items_walked", "partials_walked", "ws_bad")
        out["plans"] = [dict(zip(names, (int(v) for v in take(np.int64, len(names))))) for _ in range(out["passes"])]
        out["y"] = take(np.float64, n * m).reshape(m, n).T
        out["diag"] = take(np.float64, n)
        out["writes"] = take(np.int32, n * m)
        assert at == len(raw)
        return out
    return run


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("n", SIZES)
def test_the_triangular_copy_multiplies_exactly_and_the_plan_follows_its_rule(driver, n, uplo):
    rng = np.random.default_rng(1500 + n)
    a = rng.integers(-8, 9, (n, n)).astype(np.float64)
    a = np.tril(a) + np.tril(a, -1).T                          # symmetric, entries in [-8, 8]
    lda = n + 3 if uplo == "L" else n
    for m in WIDTHS:
        x = rng.integers(-8, 9, (n, m)).astype(np.float64)
        for ncu in ((1, 8, 256) if m in (1, 48) else (256,) if n < 500 else (8,)):
            out = driver(a, lda, x, ncu, uplo)
            tag = f"n={n} uplo={uplo} lda={lda} m={m} ncu={ncu}"
            nt = -(-n // TILE)
            # ---- the index and the copy: a bijection with its inverse; the referenced values, padding +0.0, no NaN
            assert out["n_pad"] == nt * TILE and out["stored"] == 128 * nt * (nt + 1) == out["n_pad"] ** 2 // 2 + 8 * out["n_pad"], tag
            assert (out["bad_index"], out["bad_roundtrip"], out["bad_pad"], out["bad_value"], out["nan_stored"]) == (0, 0, 0, 0, 0), (tag, out)
            assert np.array_equal(out["diag"], np.diag(a)), tag
            # ---- the product, bit for bit, every element stored once, every workspace element written once
            assert not np.isnan(out["y"]).any(), tag
            assert np.array_equal(out["y"], a @ x), tag
            assert np.all(out["writes"] == 1), tag
            # ---- the plan of every pass: the rule, and what the walk did
            widths = [min(MAX_COLS, m - c0) for c0 in range(0, m, MAX_COLS)]
            assert [p["m"] for p in out["plans"]] == widths, tag
            for p in out["plans"]:
                want = planner_rule(ncu, n, p["m"])
                assert {k: p[k] for k in want} == want, (tag, p, want)
                assert p["ws_bad"] == 0 and p["items_walked"] == p["items"] and p["partials_walked"] == p["max_partials"], (tag, p)


@pytest.mark.parametrize("ncu", [1, 8, 256])
def test_the_plan_equals_its_rule_at_sizes_the_walk_does_not_reach(driver, tmp_path, ncu):
    """the driver's plan-only mode (lda = 0): dense_sym_plan against the transcription at the sizes of the benchmark and beyond"""
    names = ("m", "acc_groups", "panels", "chunk_panels", "chunk_blocks", "max_chunks", "items", "max_partials", "t_base", "ws_doubles")
    for n, m in ((2048, 8), (2048, 37), (8192, 8), (8192, 13), (8192, 37), (32768, 8), (32768, 48), (65536, 13)):
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        np.array([n, 0, m, ncu, ord("L")], np.int64).tofile(fin)
        p = subprocess.run([EXE, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        got = dict(zip(names, (int(v) for v in np.fromfile(fout, np.int64))))
        assert got == planner_rule(ncu, n, m), (n, m, ncu)


def test_the_planner_splits_where_the_rule_allows_it():
    """the shapes must not all be one-chunk cases"""
    assert planner_rule(8, 1000, 1)["max_chunks"] > 1 and planner_rule(8, 513, 8)["max_chunks"] > 1
    assert planner_rule(1, 1000, 1)["max_chunks"] == 1 and planner_rule(2, 1000, 1)["max_chunks"] == 4 and planner_rule(2, 1000, 48)["max_chunks"] == 1 and planner_rule(256, 255, 8)["items"] == 1
    assert planner_rule(256, 8192, 8)["chunk_panels"] == 1 and planner_rule(256, 32768, 8)["items"] >= 1024
    assert planner_rule(64, 8192, 8)["chunk_panels"] == 2 and planner_rule(64, 8192, 8)["items"] >= 256
