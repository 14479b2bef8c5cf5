"""CPU: dla::sell_build as its two halves (diaglib_amd/csrc/dla_internal.h) and the launch shapes of the set-up from device arrays
(dla_plans::spmm_setup_plan, diaglib_amd/csrc/hip_plans.h).

dla::sell_layout computes from the row pointers alone what the set-up from device arrays needs on the host; dla::sell_fill scatters
host entries; dla::sell_build is one after the other.  tests/sell_layout_split_driver.cpp (g++, no ROCm include, tests/_build/,
$DIAGLIB_HOSTSIM_SANITIZE honoured as in tests/test_sell_layout.py) builds a matrix both ways with the product's own code and
prints, field by field of dla::SellLayout, whether the two agree (doubles by their bits).  sell_layout cannot read a column or a
value: its signature has no parameter for them, and what it leaves of the entry arrays is empty."""
import os
import subprocess

import numpy as np
import pytest

import hostsim
from spmm_cases import LONG_ROW, SLICE, csr_from_lengths, skewed_csr

SRC = os.path.join(hostsim.ROOT, "tests", "sell_layout_split_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "sell_layout_split_driver")
SIZES = [1, 63, 64, 65, 4096, 4097, 9000]
LONG_SEG = 4096                      # dla_internal.h: SELL_LONG_SEG
FIELDS = ["n", "slices", "nnz", "stored", "long_entries", "slice_ptr", "perm", "col", "val", "diag", "long_row", "long_ptr", "long_col", "long_val",
          "long_segments", "multi_segments", "seg_ptr", "seg_row", "seg_part", "multi_row", "part_ptr"]


def special_lengths(rng, n):
    """a few entries per row, then -- on distinct rows, as far as n allows -- tail rows of 8193, 4097 and 4096 entries (three, two and
    one segment), rows of LONG_ROW + 1 and LONG_ROW entries (the first tail row and the last slice row) and empty rows"""
    lens = rng.integers(0, 6, n).astype(np.int64)
    special = [2 * LONG_SEG + 1, 0, LONG_ROW + 1, LONG_ROW, LONG_SEG + 1, LONG_SEG, 0, 0]
    rows = rng.choice(n, min(n, len(special)), replace=False)
    for r, w in zip(rows, special):
        lens[r] = w
    return lens


@pytest.fixture(scope="module")
def exe():
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    return EXE


def run_layout(exe, work, n, indptr, indices, data):
    fin = str(work / "in.bin")
    with open(fin, "wb") as f:
        np.array([n, len(indices)], np.int64).tofile(f)
        np.ascontiguousarray(indptr, np.int64).tofile(f)
        np.ascontiguousarray(indices, np.int32).tofile(f)
        np.ascontiguousarray(data, np.float64).tofile(f)
    p = subprocess.run([exe, "layout", fin], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return {k: int(v) for k, v in (ln.split("=") for ln in p.stdout.split())}


@pytest.mark.parametrize("kind", ["skewed", "special"])
@pytest.mark.parametrize("n", SIZES)
def test_layout_then_fill_is_build(exe, tmp_path, n, kind):
    rng = np.random.default_rng(1000 + n)
    if kind == "skewed":
        indptr, indices, data = skewed_csr(rng, n)
    else:
        lens = special_lengths(rng, n)
        indptr, indices, data = csr_from_lengths(rng, n, lens)
        if n >= 8:
            assert {0, LONG_ROW, LONG_ROW + 1, LONG_SEG, LONG_SEG + 1, 2 * LONG_SEG + 1} <= set(int(v) for v in lens)
    out = run_layout(exe, tmp_path, n, indptr, indices, data)
    assert [f for f in FIELDS if out[f] != 1] == []
    assert out["layout_only_empty"] == 1, "sell_layout left entries behind: it has none to read"
    lens = np.diff(indptr)
    tail = lens[lens > LONG_ROW]
    assert out["count_slices"] == -(-n // SLICE) and out["count_long_rows"] == len(tail)
    segs = -(-tail // LONG_SEG)
    assert out["count_long_segments"] == int(segs.sum()) and out["count_multi_segments"] == int(segs[segs > 1].sum())
    if kind == "special" and n >= 8:
        assert out["count_multi_segments"] == 3 + 2              # the rows of 8193 and 4097 entries


def test_launch_shapes_of_the_device_setup(exe):
    """blocks >= 1 wherever something is launched, also at n = 1; never above 8 blocks per CU; nothing for a format's absent part"""
    cases = []
    for ncu in (1, 8, 256):
        for n in SIZES + [2 * 10 ** 6, 2 ** 31 - 1]:
            for nnz in (1, n, 38 * 10 ** 6, 2 ** 40):
                for slices, segs in ((0, 0), (-(-n // SLICE), 0), (-(-n // SLICE), 1), (-(-n // SLICE), 3), (-(-n // SLICE), 10 ** 6)):
                    cases.append((ncu, n, nnz, slices, segs))
    p = subprocess.run([exe, "plan"], input="".join("%d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == len(cases)
    for (ncu, n, nnz, slices, segs), ln in zip(cases, lines):
        got = {k: int(v) for k, v in (t.split("=") for t in ln.split())}
        cap = got["cap"]
        assert cap == 8 * ncu
        assert got["entry_blocks"] == max(1, min(cap, -(-nnz // 256))), (ncu, n, nnz, ln)
        assert got["row_blocks"] == max(1, min(cap, -(-n // 256))), (ncu, n, ln)
        assert got["slice_blocks"] == (max(1, min(cap, -(-slices // 4))) if slices else 0), (ncu, slices, ln)
        assert got["seg_blocks"] == (max(1, min(cap, -(-segs // 4))) if segs else 0), (ncu, segs, ln)
        for k in ("entry_blocks", "row_blocks", "slice_blocks", "seg_blocks"):
            assert 0 <= got[k] <= cap
        assert got["entry_blocks"] >= 1 and got["row_blocks"] >= 1
