"""CPU: the segments of the sliced format's CSR tail (dla::sell_build, diaglib_amd/csrc/dla_internal.h) and the plan of their
launches (dla_plans::long_rows_plan, diaglib_amd/csrc/hip_plans.h).

tests/long_segments_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_sell_layout.py does): it builds the layout with the product's own code, multiplies the tail rows by walking the
segment table the way csr_long_segments_kernel and long_rows_combine_kernel do, and writes the tables.  Here they are held to
what include/diaglib_amd.h promises: every tail entry in exactly one segment, segments in row order and contiguous, all but a
row's last of exactly SEG entries, a dense and disjoint workspace, one writer per element."""
import os
import subprocess

import numpy as np
import pytest

import hostsim
from spmm_cases import LONG_ROW, csr_from_lengths, skewed_csr
from test_operators_gpu import EPS, LD, assert_within, csr_product_reference

SRC = os.path.join(hostsim.ROOT, "tests", "long_segments_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "long_segments_driver")
PLANS = [(ncu, m) for ncu in (1, 256) for m in (1, 4, 5, 13, 37)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    work = tmp_path_factory.mktemp("segments")

    def run(n, indptr, indices, data, x):
        m = x.shape[1]
        fin, fout = str(work / "in.bin"), str(work / "out.bin")
        with open(fin, "wb") as f:
            np.array([n, m, len(indices), len(PLANS)], np.int64).tofile(f)
            np.ascontiguousarray(indptr, np.int64).tofile(f)
            np.ascontiguousarray(indices, np.int32).tofile(f)
            np.ascontiguousarray(data, np.float64).tofile(f)
            np.asfortranarray(x, np.float64).T.tofile(f)
            np.array(PLANS, np.int64).tofile(f)
        p = subprocess.run([EXE, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        raw = open(fout, "rb").read()
        at = 0

        def take(dtype, count):
            nonlocal at
            a = np.frombuffer(raw, dtype, count, at)
            at += a.nbytes
            return a
        names = ("n", "m", "SEG", "LONG_ROW", "long_rows", "long_entries", "long_segments", "multi_segments", "multi_rows")
        out = dict(zip(names, (int(v) for v in take(np.int64, 9))))
        assert (out["n"], out["m"]) == (n, m)
        out["long_row"], out["long_ptr"] = take(np.int32, out["long_rows"]), take(np.int64, out["long_rows"] + 1)
        out["seg_ptr"], out["seg_row"], out["seg_part"] = (take(np.int64, out["long_segments"] + 1), take(np.int32, out["long_segments"]),
                                                           take(np.int32, out["long_segments"]))
        out["multi_row"], out["part_ptr"] = take(np.int32, out["multi_rows"]), take(np.int32, out["multi_rows"] + 1)
        out["ax"] = take(np.float64, n * m).reshape(m, n).T
        out["ax_writes"], out["part_writes"] = take(np.int32, n), take(np.int32, out["multi_segments"])
        out["plans"] = take(np.int64, 4 * len(PLANS)).reshape(len(PLANS), 4)
        assert at == len(raw)
        return out
    return run


@pytest.fixture(scope="module")
def seg(driver):
    """SEG as the product was compiled (tuning it must not break this file)"""
    p = subprocess.run([EXE, "constants"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    s, long_row = (int(v) for v in p.stdout.split())
    assert long_row == LONG_ROW
    assert s > 0 and s % 64 == 0, "a segment is a positive multiple of the wavefront width"
    return s


def check_segments(out, n, indptr, indices, data, x, seg):
    lens = np.diff(indptr)
    m = x.shape[1]
    assert (out["SEG"], out["LONG_ROW"]) == (seg, LONG_ROW)
    is_long = lens > LONG_ROW
    # ---- the tail itself, as tests/test_sell_layout.py holds it
    assert np.array_equal(out["long_row"], np.flatnonzero(is_long))
    tail_len = lens[out["long_row"]]
    assert np.array_equal(np.diff(out["long_ptr"]), tail_len) and out["long_entries"] == int(tail_len.sum())
    # ---- counts
    per_row = -(-tail_len // seg)
    assert out["long_segments"] == int(per_row.sum())
    assert out["multi_rows"] == int((per_row > 1).sum()) and out["multi_segments"] == int(per_row[per_row > 1].sum())
    # ---- every tail entry in exactly one segment: the segments tile [0, long_entries) without gap or overlap, in row order
    sp, sr = out["seg_ptr"], out["seg_row"]
    assert sp[0] == 0 and sp[-1] == out["long_entries"]
    assert np.all(np.diff(sp) >= 1) and np.all(np.diff(sp) <= seg)
    assert np.array_equal(sr, np.repeat(np.arange(out["long_rows"]), per_row)), "segments are not in row order"
    first = (np.cumsum(per_row) - per_row).astype(np.int64)                           # first segment of every tail row
    assert np.array_equal(sp[first], out["long_ptr"][:-1]), "a row's first segment does not start at the row"
    assert np.array_equal(sp[first + per_row], out["long_ptr"][1:]), "a row's last segment does not end with the row"
    s_in_row = np.arange(out["long_segments"]) - first[sr]
    assert np.array_equal(sp[:-1], out["long_ptr"][sr] + s_in_row * seg), "segment s of a row does not start at p0 + s SEG"
    last = s_in_row == per_row[sr] - 1
    assert np.all(np.diff(sp)[~last] == seg), "a segment that is not its row's last must have SEG entries"
    assert np.array_equal(np.diff(sp)[last], tail_len - (per_row - 1) * seg)
    # ---- the workspace: dense, disjoint, in row and segment order; single segments own no slot
    multi = per_row[sr] > 1
    assert np.all(out["seg_part"][~multi] == -1)
    assert np.array_equal(out["seg_part"][multi], np.arange(out["multi_segments"])), "the slots of the workspace are not dense and disjoint"
    assert np.array_equal(out["multi_row"], out["long_row"][per_row > 1])
    assert out["part_ptr"][0] == 0 and np.array_equal(np.diff(out["part_ptr"]), per_row[per_row > 1])
    if out["multi_rows"]:
        assert np.array_equal(out["seg_part"][multi][s_in_row[multi] == 0], out["part_ptr"][:-1])
    # ---- one writer per element, and the walk gives the product of the triplets on the tail rows
    assert np.array_equal(out["ax_writes"], is_long.astype(np.int32)), "every tail row is stored exactly once, no other row is touched"
    assert np.array_equal(out["part_writes"], np.ones(out["multi_segments"], np.int32))
    assert np.all(out["ax"][~is_long] == 7.0)
    if is_long.any():
        ref, mag = csr_product_reference(indptr, indices, data, x)
        assert_within(out["ax"][is_long], ref[is_long], {"(len + 2) eps |A||x|": (lens[is_long, None] + 2) * EPS * mag[is_long], "tiny": LD(1e-300)},
                      f"segment walk n={n}")
    # ---- the plan
    for (ncu, mp), (seg_blocks, combine_blocks, part_doubles, named) in zip(PLANS, out["plans"]):
        assert named == 1
        assert 1 <= seg_blocks <= max(1, min(8 * ncu, -(-out["long_segments"] // 4)))
        assert part_doubles == out["multi_segments"] * mp
        if out["multi_segments"] == 0:
            assert combine_blocks == 0, "nothing to combine: no launch"
        else:
            assert 1 <= combine_blocks <= max(1, min(8 * ncu, -(-out["multi_rows"] * mp // 256)))
    return m


@pytest.mark.parametrize("n", [257, 4097, 20000])
def test_segments_of_skewed_matrices(driver, seg, n):
    rng = np.random.default_rng(300 + n)
    indptr, indices, data = skewed_csr(rng, n)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = driver(n, indptr, indices, data, x)
    check_segments(out, n, indptr, indices, data, x, seg)
    assert out["long_rows"] >= 1
    if n > seg:
        assert out["multi_segments"] >= 2            # the dense row


def test_no_tail_row(driver, seg):
    n = 500
    rng = np.random.default_rng(1)
    lens = rng.integers(0, LONG_ROW + 1, n)
    lens[3] = LONG_ROW
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    x = np.asfortranarray(rng.standard_normal((n, 1)))
    out = driver(n, indptr, indices, data, x)
    check_segments(out, n, indptr, indices, data, x, seg)
    assert out["long_rows"] == out["long_segments"] == out["multi_segments"] == 0
    assert np.all(out["plans"][:, 1] == 0) and np.all(out["plans"][:, 0] == 1) and np.all(out["plans"][:, 2] == 0)


def test_only_tail_rows(driver, seg):
    n = 300
    rng = np.random.default_rng(2)
    indptr, indices, data = csr_from_lengths(rng, n, rng.integers(LONG_ROW + 1, n + 1, n))
    x = np.asfortranarray(rng.standard_normal((n, 3)))
    out = driver(n, indptr, indices, data, x)
    check_segments(out, n, indptr, indices, data, x, seg)
    assert out["long_rows"] == n


def edge_lengths(seg):
    return [LONG_ROW + 1, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 63, 3 * seg + 1]


def test_rows_on_the_edges_of_a_segment(driver, seg):
    """rows of LONG_ROW + 1, SEG - 1, SEG, SEG + 1, 2 SEG, 2 SEG + 63, 3 SEG + 1 and n entries on distinct rows among short ones"""
    n = 3 * seg + 70
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 6, n)
    special = edge_lengths(seg) + [n]
    rows = rng.choice(n, len(special), replace=False)
    lens[rows] = special
    indptr, indices, data = csr_from_lengths(rng, n, lens)
    x = np.asfortranarray(rng.standard_normal((n, 2)))
    out = driver(n, indptr, indices, data, x)
    check_segments(out, n, indptr, indices, data, x, seg)
    want = {r: -(-w // seg) for r, w in zip(rows.tolist(), special) if w > LONG_ROW}
    got = {int(out["long_row"][r]): int(c) for r, c in zip(*np.unique(out["seg_row"], return_counts=True))}
    assert got == want
    assert out["long_segments"] == sum(want.values()) and out["multi_segments"] == sum(v for v in want.values() if v > 1)
    assert out["multi_rows"] >= 4                    # SEG + 1, 2 SEG, 2 SEG + 63, 3 SEG + 1 and the dense row
