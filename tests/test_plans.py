"""CPU: what the HIP engine decides before it launches (diaglib_amd/csrc/hip_plans.h) -- tile shapes, passes, blocks, LDS bytes,
quarter tiles, pipeline depth, the booked kernel names and the schedule of an orthogonalisation chain.

tests/plans_driver.cpp is compiled with g++ and no ROCm include (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured, as
tests/test_sell_layout.py does); it reads shape lines and prints plan fields and names from the product's own planners.  Expected
values come from outside the planners: the committed rocprofv3 record of the benchmark, the literal names tests/test_knobs_gpu.py
asserts, the rules the planners' comments state, and the kernels' instance lists.  Those lists live in hip_plans.h (GRAM_TILES,
gram_direct_instance, GRAM_LOW_TILES, GRAM_LDS_FORMS, WP_TILES, GEMM_INSTANCES, RITZ_INSTANCES, RITZ2_INSTANCES), where the planners
and the dispatch ladders of hip_engine.hip both read them; they are transcribed below as literal sets (the gemm_kernel set as its rules),
and test_transcribed_instance_lists_are_the_engines holds each transcription against what the driver prints from the header."""
import csv
import itertools
import os
import re
import subprocess

import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "plans_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "plans_driver")
RECORD = os.path.join(hostsim.ROOT, "profiles", "r06", "kernel_stats_bench_steps5.csv")
KIB = 1024
NCU, LDS = 256, 160 * KIB
N_BENCH, N_MAX, ROOTS = 2_000_000, 13, 8


def run_plans(lines):
    """the driver's answer to each request line: (fields, name) per line, and the OP_* numbers it prints last"""
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    out = p.stdout.splitlines()
    ops = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in out[-1].split()[1:]}
    silent = sum(1 for ln in lines if ln.split()[0] in ("env", "policy"))
    assert len(out) - 1 == len(lines) - silent, (len(out), len(lines))
    res = []
    for ln in out[:-1]:
        fields, _, name = ln.partition(" | ")
        d = {}
        for kv in fields.split():
            key, val = kv.split("=")
            d[key] = val if key in ("take", "ops") or ";" in val else int(val)
        if "ops" in d:
            d["ops"] = [int(v) for v in d["ops"].split(",")] if d["ops"] else []
        res.append((d, name))
    return res, ops


def env_line(ncu=NCU, lds=LDS, **knob):
    t = [0] * 8
    for key, v in knob.items():
        t[int(key[1:])] = v
    return "env %d %d %s" % (ncu, lds, " ".join(str(v) for v in t))


def recorded_names():
    names = {}
    with open(RECORD) as f:
        for row in csv.DictReader(f):
            nm = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
            names[nm.split("(")[0]] = int(row["Calls"])
    return names


# ---------------------------------------------------------------- a. names against the record
def test_names_of_the_benchmark_shapes_are_the_recorded_kernels():
    """a Davidson solve of the benchmark: 13-column blocks behind 0, 13, ... basis columns (one-tile chains: the pending-factor sweeps,
    the plain projections, the fused triangular update), the operator's 4-column W^T x, the Ritz sweep of 8 roots.

    The reach is the record's: its 5 steps converge with 8 blocks in the basis (its widest pass holds 7 tiles), so the basis widths
    stop at 104 columns and not at max_dav blocks.  And in it the chain's fused sweeps carry every product of the solve -- it lists
    one gemm_kernel instance, the fused triangular update -- so the plain products (modes 0 / 1) have no recorded name to be held
    against here; test_names_the_knob_tests_assert and the GPU test of tests/test_knobs_gpu.py hold them against literal names and
    against the kernels that run."""
    rec = recorded_names()
    basis = [N_MAX * j for j in range(1, 9)]
    lines = [env_line(), f"gram {N_BENCH} {N_MAX} {N_MAX} 1 1 0", f"gram {N_BENCH} 4 {N_MAX} 0 1 0", f"wp {N_BENCH} 0 {N_MAX} 0",
             f"gemm {N_BENCH} {N_MAX} {N_MAX} 2 1 1 1"]
    for m in basis:
        lines += [f"gram {N_BENCH} {m} {N_MAX} 0 1 0", f"wp {N_BENCH} {m} {N_MAX} 0", f"wp {N_BENCH} {m} {N_MAX} 1",
                  f"ritz {N_BENCH} {m + N_MAX} {ROOTS} 0 1 1"]
    res, _ = run_plans(lines)
    produced = {name for _, name in res}
    missing = sorted(nm for nm in produced if nm not in rec)
    assert not missing, missing
    top = ["ritz_kernel<1, 2, 3, 0, 0, false, 0>", "gram_lds_kernel<5, 1, 1, 16, 0, 0, 0, 1>", "gemm_kernel<1, 2, 2, GemmArgs, true, 0, 0, 9, 0, 2>",
           "gram_kernel<1, 1, 2, 4, 0, -1>"]
    for nm in top:
        assert nm in rec and nm in produced, nm
    # every Gram, product and Ritz sweep of the record is one the planners name for these shapes (the reductions have no plan)
    swept = {nm for nm in rec if re.match(r"(gram_lds_kernel|gram_kernel|gemm_kernel|ritz_kernel)<", nm)}
    assert swept <= produced, sorted(swept - produced)


def test_names_the_knob_tests_assert():
    """tests/test_knobs_gpu.py: the plain two-tile product of 21 columns at n = 4096 with knob 2 = 1, and with knob 7 = 1 / 0"""
    req = "gemm 4096 42 21 0 0 0 1"
    res, _ = run_plans([env_line(t2=1), req, env_line(t7=1), req, env_line(), req])
    assert [name for _, name in res] == ["gemm_kernel<2, 2, 0, GemmArgs, false, 1, 0, 9, 0, 2>", "gemm_kernel<2, 2, 0, GemmArgs, false, 1, 2, 9, 0, 2>",
                                         "gemm_kernel<2, 2, 0, GemmArgs, false, 1, 2, 9, 2, 2>"]


# ---------------------------------------------------------------- b. invariants the kernels impose
# the (TLW, KT) pairs gram_dev_once can launch (GRAM_TILES)
GL = {(t, 1) for t in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)} | {(t, 2) for t in range(1, 9)} | {(t, 3) for t in range(1, 8)} | {(t, 4) for t in (1, 2, 3)}


def direct_load_instance(t, k):
    """the widths launch_gram has a gram_kernel instance for"""
    return not (t in (5, 7, 10) or (t == 12 and k > 1) or (t == 3 and 2 <= k <= 3) or (t >= 5 and k == 3) or (t >= 7 and k == 2))


# the (TLW, KT, R) triples gram_wp_once can launch (WP_TILES)
GWP = {(t, 1, 32) for t in (1, 2)} | {(t, 1, 16) for t in (3, 4, 5, 6, 7, 8, 10, 12)} | {(t, 2, 16) for t in range(1, 9)} | {(t, 3, 16) for t in range(1, 6)}


def gemm_kernel_instance(kt, vec, mode, inl, fuse, pipe, qt, rtp):
    """the gemm_kernel instances launch_gemm can launch (GEMM_INSTANCES), rule by rule"""
    if fuse and mode == 3:
        return False                                  # the fused form: modes 0 .. 2
    if inl and kt != 1:
        return False                                  # coefficients in the kernel arguments: one tile
    if qt and not (vec == 2 and kt >= 2):
        return False                                  # quarter tiles: the 16-byte path, two and three tiles
    if qt and not fuse and mode == 1 and kt == 2:
        return False                                  # ... which the plain two-tile update never takes
    if rtp == 1 and not (fuse and kt == 3 and vec == 2):
        return False                                  # one row group: the fused three-tile sweep on the 16-byte path
    own = {1: 0, 2: 2, 3: 3 if fuse else 2}[kt]       # the kernel's own depth
    return pipe == own or (pipe in (0, 4) and not fuse and vec == 2 and kt >= 2 and mode in (0, 1) and not qt)


# (kt, vec, mode, inl, fuse, pipe, qt, rtp) of gemm_kernel<kt, vec, mode, GemmArgsInl / GemmArgs, fuse, mode != 2, pipe, 9, qt, rtp>
GEMM = {r for r in itertools.product((1, 2, 3), (1, 2), (0, 1, 2, 3), (0, 1), (0, 1), (0, 2, 3, 4), (0, 1, 2), (1, 2)) if gemm_kernel_instance(*r)}


def listed_instances():
    """what the driver prints of hip_plans.h: each list as a list of integer tuples, in the header's order"""
    res, _ = run_plans(["instances"])
    return {key: [tuple(int(v) for v in row.split(",")) for row in val.split(";") if row] for key, val in res[0][0].items()}


def test_transcribed_instance_lists_are_the_engines():
    inst = listed_instances()
    for rows in inst.values():
        assert len(set(rows)) == len(rows), rows                     # no row twice: a ladder launches the first hit
    assert set(inst["gram_tiles"]) == GL and len(inst["gram_tiles"]) == 28
    assert set(inst["gram_direct"]) == {(t, k) for t in range(1, 13) for k in range(1, 5) if direct_load_instance(t, k)}
    assert inst["gram_low_tiles"] == [(4,), (5,), (6,), (7,)]
    assert set(inst["wp_tiles"]) == GWP and len(inst["wp_tiles"]) == 23
    # ritz_kernel<kt, vec, 3, pipe, qt, xp>: (kt, vec, pipe, qt, xp), the kernel's own pipeline depth 0 / 2 / 3 / 3 / 3 by kt
    own = {1: 0, 2: 2, 3: 3, 4: 3, 5: 3}
    ritz = {(kt, 2, own[kt], 0, 1) for kt in range(1, 6)} | {(kt, 2, own[kt], qt, 1) for kt in (2, 3) for qt in (1, 2)}
    ritz |= {(kt, 2, pipe, 0, 0) for kt in (2, 3) for pipe in (0, 4)} | {(kt, 2, own[kt], qt, 0) for kt in (2, 3) for qt in (1, 2)}
    ritz |= {(kt, vec, own[kt], 0, 0) for kt in (1, 2, 3) for vec in (1, 2)}
    assert set(inst["ritz_instances"]) == ritz and len(inst["ritz_instances"]) == 23
    # ritz2_kernel<kt, vec>
    assert set(inst["ritz2_instances"]) == {(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)} and len(inst["ritz2_instances"]) == 6
    # gram_lds_kernel<tlw, kt, 1, R, self, qt> of a listed pass: (self, qt)
    assert set(inst["gram_lds_forms"]) == {(s, q) for s in (0, 1) for q in (0, 1, 2)} and len(inst["gram_lds_forms"]) == 6
    assert set(inst["gemm"]) == GEMM and len(inst["gemm"]) == 99
    assert sum(1 for r in GEMM if r[4]) == 45 and sum(1 for r in GEMM if r[3]) == 14              # fused; coefficients in the arguments


@pytest.mark.parametrize("lds_limit", [64 * KIB, 160 * KIB])
def test_gram_plans_fit_the_kernels(lds_limit):
    cases = [(l, k, same, al, low) for l in range(1, 209) for k in range(1, 65) for same in (0, 1) for al in (0, 1) for low in (0, 1)]
    res, _ = run_plans([env_line(lds=lds_limit)] + [f"gram {N_BENCH} {l} {k} {s} {a} {w}" for l, k, s, a, w in cases])
    for (l, k, same, al, low), (p, name) in zip(cases, res):
        what = (l, k, same, al, low, p, name)
        tx, tu = -(-l // 16), -(-k // 16)
        if p["low_single"]:
            assert p["tlw"] == p["kt"] and 4 <= p["tlw"] <= 7 and p["passes"] == 1 and p["tlw"] >= tx and p["lds"] and p["rows"] == 16, what
        else:
            assert (p["tlw"], p["kt"]) in GL, what
            assert p["passes"] % p["px"] == 0 and (p["passes"] // p["px"]) * p["kt"] >= tu, what
        assert p["px"] * p["tlw"] >= tx, what
        if p["lds"]:
            assert p["kt"] <= 3 or p["low_single"], what
        else:
            assert direct_load_instance(p["tlw"], p["kt"]), what
        assert p["lds_bytes"] <= lds_limit, what
        assert p["rows"] in (16, 32) and (p["rows"] == 16 or p["can32"]), what
        if p["self"]:
            assert same and l == k and p["passes"] == 1 and p["lower"], what
        assert p["qt"] in (0, 1, 2), what
        if p["qt"]:
            assert 1 <= k % 16 <= 8 and p["kt"] in (2, 3) and p["vec2"] and p["lds"] and p["qt"] == -(-(k % 16) // 4), what
        assert 1 <= p["blocks_per_pass"] <= 2 * NCU, what
        assert p["vec2"] == al, what


def per_cu_steps(lds):
    return 1 if lds > 80 * KIB else 2 if lds > 40 * KIB else 4


@pytest.mark.parametrize("knob", [0, 1, 4, "no_quarter_tiles", "fused3_two_row_groups"])
def test_gemm_plans_fit_the_kernels(knob):
    """knob 2 at 0 / 1 / 4 (Knobs::gemm_pipe_depth), and knob 7 at 1 (no_quarter_tiles) and 5 (fused3_two_row_groups)"""
    tune = {"no_quarter_tiles": {"t7": 1}, "fused3_two_row_groups": {"t7": 5}}.get(knob, {"t2": knob})
    depth = {1: 0, 4: 4}.get(knob)                                       # the depth knob 2 asks for, if any
    cases = [(l, k, mode, fuse, packed, v) for l in (1, 4, 13, 16, 17, 42, 63, 104, 208, 320, 512) for k in range(1, 49) for mode in range(4)
             for fuse in (0, 1) for packed in (0, 1) for v in (0, 1) if not (fuse and mode == 3)]
    rows = listed_instances()["gemm"]
    res, _ = run_plans([env_line(**tune)] + [f"gemm {N_BENCH} {l} {k} {m} {f} {pk} {v}" for l, k, m, f, pk, v in cases])
    for (l, k, mode, fuse, packed, v), (p, name) in zip(cases, res):
        what = (l, k, mode, fuse, packed, v, p, name)
        kt = -(-k // 16)
        assert p["kt"] == kt and p["l4"] == -(-l // 4) * 4 and p["l4"] >= l, what
        assert p["per_cu"] == per_cu_steps(p["lds"]), what
        one_group = bool(fuse and kt == 3 and v and p["per_cu"] >= 2 and knob != "fused3_two_row_groups")
        assert (p["rtp"] == 1) == one_group and p["rtp"] in (1, 2), what
        own = 3 if (fuse and kt >= 3) else 2 if kt >= 2 else 0           # the kernels' own depth: 0 / 2 / 2 plain, 0 / 2 / 3 fused
        if not fuse and depth is not None and v and kt >= 2 and mode in (0, 1):
            assert p["pipe"] == depth and p["qt"] == 0, what             # another depth: plain, 16-byte path, modes 0 / 1, no quarter tiles
        else:
            assert p["pipe"] == own, what
        assert p["qt"] in (0, 1, 2) and (not p["qt"] or (1 <= k % 16 <= 8 and kt in (2, 3) and v)), what
        assert not (p["qt"] and knob == "no_quarter_tiles"), what
        # the one instance launch_gemm launches for it: no plan of the grid may reach "gemm: no kernel instance"
        assert rows.count((kt, 2 if v else 1, mode, p["inl"], fuse, p["pipe"], p["qt"], p["rtp"])) == 1, what
        assert p["inl"] == int(not packed and kt == 1 and p["l4"] <= 16), what
        assert 1 <= p["blocks"] <= NCU * p["per_cu"], what
        floor = 8 * p["l4"] * (16 * (kt - 1) + 8 if p["qt"] else 16 * kt)           # the LDS copy of C
        assert p["lds"] >= floor and (fuse or p["lds"] == floor), what


@pytest.mark.parametrize("knob", [0, 1, 4])
def test_ritz_plans_fit_the_kernels(knob):
    # (with extra products up to five column tiles, plain blocks up to three: m + k2 = 49 .. 80 are the four- and five-tile kernels)
    cases = [(l, m, k2, v) for l in (8, 13, 26, 104, 260, 520, 740) for m in range(1, 49) for k2 in (0, 5, 13, 24, 32, 37) for v in (0, 1)
             if m + k2 <= 80 and (k2 == 0 or v)]
    rows = listed_instances()["ritz_instances"]
    tiles_that_fit = set()
    res, _ = run_plans([env_line(t0=knob)] + [f"ritz {N_BENCH} {l} {m} {k2} {v} 1" for l, m, k2, v in cases])
    for (l, m, k2, v), (p, name) in zip(cases, res):
        what = (l, m, k2, v, p, name)
        kt = -(-(m + k2) // 16)
        assert p["kt"] == kt and p["xp"] == int(k2 > 0), what
        assert p["fits"] == int(p["lds_c"] <= p["dyn_limit"]) and p["dyn_limit"] <= LDS, what
        assert p["per_cu"] == per_cu_steps(p["lds"]), what
        own = 3 if kt >= 3 else 2 if kt >= 2 else 0
        if knob and not k2 and v and kt >= 2:
            assert p["pipe"] == {1: 0, 4: 4}[knob] and p["qt"] == 0, what      # RZ: ritz_kernel<KT, 2, 3, 0> / <KT, 2, 3, 4>
        else:
            assert p["pipe"] == own, what
        assert p["qt"] in (0, 1, 2) and (not p["qt"] or (1 <= (m + k2) % 16 <= 8 and kt in (2, 3) and v)), what
        assert 1 <= p["blocks"] <= NCU * p["per_cu"], what
        if p["fits"]:
            # the one instance ritz_residual_once launches for it: no plan that fits may reach "ritz: no kernel instance"
            assert rows.count((p["kt"], 2 if v else 1, p["pipe"], p["qt"], p["xp"])) == 1, what
            tiles_that_fit.add((p["kt"], p["xp"]))
    assert tiles_that_fit == {(kt, 0) for kt in (1, 2, 3)} | {(kt, 1) for kt in (1, 2, 3, 4, 5)}


@pytest.mark.parametrize("knob", [0, 6])
def test_ritz2_plans_fit_the_kernels(knob):
    """the RITZ2_INSTANCES ladder of ritz_residual2; knob 0 = 6 switches the sweep off"""
    cases = [(l, m, v) for l in (8, 13, 26, 104, 260, 520, 740) for m in range(1, 49) for v in (0, 1)]
    rows = listed_instances()["ritz2_instances"]
    res, _ = run_plans([env_line(t0=knob)] + [f"ritz2 {N_BENCH} {l} {m} {v} 1" for l, m, v in cases])
    tiles_that_fit = set()
    for (l, m, v), (p, name) in zip(cases, res):
        what = (l, m, v, p, name)
        if p["fits"]:
            # the one instance ritz_residual2 launches for it: no plan that fits may reach "ritz2: no kernel instance"
            assert p["kt"] == -(-m // 16) and rows.count((p["kt"], 2 if v else 1)) == 1, what
            tiles_that_fit.add(p["kt"])
    assert tiles_that_fit == (set() if knob == 6 else {1, 2, 3})


def test_pending_factor_sweeps_fit_the_kernels():
    """the WP_TILES ladder of gram_wp_once"""
    cases = [(m, k, pr) for m in range(0, 209) for k in range(1, 49) for pr in (0, 1) if not (pr and (k > 16 or m == 0)) and not (m == 0 and k > 16)]
    res, _ = run_plans([env_line()] + [f"wp {N_BENCH} {m} {k} {pr}" for m, k, pr in cases])
    lds, _ = run_plans([env_line()] + [f"wp_lds {N_BENCH} {m} {k} {pr}" for m, k, pr in cases])
    for (m, k, pr), (p, name), (b, _) in zip(cases, res, lds):
        what = (m, k, pr, p, name, b)
        assert (p["tlw"], p["kt"], p["R"]) in GWP and p["tlw"] <= p["max_tlw"], what
        assert p["passes"] * p["tlw"] >= -(-m // 16) and p["kt"] == -(-k // 16), what
        assert p["self"] == int(m == 0) and 1 <= p["blocks"] <= 2 * NCU, what
        assert 8 * 4 * 16 * (p["tlw"] + p["kt"]) * (p["R"] + 2) <= LDS, what
        assert name.endswith(", %d>" % (2 if pr else 1)), what
        # WpPlan::lds_bytes, the dynamic LDS of the launch, is the arithmetic launch_gram_wp used to write by hand
        assert b["lds_bytes"] == (8 * 4 * 16 * 34 if m == 0 else 8 * 4 * 16 * (p["tlw"] + p["kt"]) * (p["R"] + 2)), what


def test_fused_lds_is_the_formula_the_engine_had():
    """fused_lds, which can_combo, the fused updates and ChainIn::fused_lds_kk read, at (k, k), (m + k, k) and (l, k): packed C of l
    rows rounded to 4 and kt column tiles, 4 wave tiles of 16 x (16 kt + 9) doubles, at least 8 KiB"""
    shapes = sorted({(k, k) for k in range(1, 49)} | {(m + k, k) for m in (13, 16, 125, 192, 208, 500) for k in (8, 13, 16, 17, 32, 48)} |
                    {(l, k) for l in (1, 4, 13, 16, 17, 42, 63, 104, 208, 320, 512) for k in (1, 13, 16, 21, 33, 48)})
    res, _ = run_plans([f"fused {l} {k}" for l, k in shapes])
    for (l, k), (d, _) in zip(shapes, res):
        kt, l4 = -(-k // 16), -(-l // 4) * 4
        assert d["fused_lds"] == max(8 * (kt * l4 * 16 + 4 * 16 * (16 * kt + 9)), 8192), (l, k, d)


# ---------------------------------------------------------------- c. the chain schedule
def chain_line(m, k, vec2=1, bx_is_x=1, combo_ok=1, host_between=0, cooldown=0, dmat_cols=0, dmat_nontrivial=0, fused_lds_kk=8192):
    return f"chain {m} {k} {vec2} {bx_is_x} {combo_ok} {host_between} {cooldown} {dmat_cols} {dmat_nontrivial} {fused_lds_kk}"


POLICIES = {"plain": "policy 0 0 0 0 0", "rebuilt": "policy 1 1 0 0 0", "tight": "policy 1 1 0 0 1e-6", "basis_exact": "policy 1 1 1 0 0"}


@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("lds_limit", [64 * KIB, 160 * KIB])
def test_schedule_per_case(policy, lds_limit):
    cases = list(itertools.product((8, 16, 17, 32, 48), (0, 16, 125, 192, 208), (0, 1), (0, 2), (0, 1)))     # k, m, bx_is_x, cooldown, vec2
    lines = [env_line(lds=lds_limit), POLICIES[policy]]
    lines += [chain_line(m, k, vec2=v, bx_is_x=b, cooldown=cd, dmat_cols=m) for k, m, b, cd, v in cases]
    res, _ = run_plans(lines)
    for (k, m, b, cd, v), (c, _) in zip(cases, res):
        what = (policy, lds_limit, k, m, b, cd, v, c)
        big = lds_limit > 128 * KIB
        fold = (1 if (v and 0 < m <= 192 and big) else 2) if k <= 16 else 0
        if policy == "basis_exact" and m > 0 and fold == 0:
            assert c["take"] == "host_loop", what          # only the matrix-core tail projects with the caller's D
            continue
        assert c["take"] == "chain" and c["fold"] == fold, what
        assert c["x3"] == int(fold == 1 and b and (cd <= 0 or policy in ("rebuilt", "basis_exact"))), what
        kt = -(-k // 16)
        wide = fold == 0 and m > 0 and v and b and kt in (2, 3) and -(-(m + k) // 16) <= (8 if kt == 2 else 7) and big
        assert c["wide_gramx"] == int(wide), what
        assert c["wide_xw"] == int(wide and kt == 2 and -(-m // 16) <= 8 and (m + k) * k <= 640 * 16), what


def test_calls_no_chain_takes():
    lines = [env_line(), POLICIES["plain"], chain_line(16, 8, combo_ok=0), chain_line(16, 8, host_between=1), chain_line(16, 49), chain_line(16, 0),
             chain_line(0, 48, fused_lds_kk=LDS + 8), chain_line(0, 48, fused_lds_kk=LDS), "policy 0 0 0 1 0", chain_line(16, 8),
             POLICIES["basis_exact"], chain_line(16, 8, dmat_cols=3), chain_line(400, 8, dmat_cols=400, dmat_nontrivial=1), chain_line(400, 8, dmat_cols=400)]
    res, _ = run_plans(lines)
    assert [c["take"] for c, _ in res] == ["host_loop", "host_loop", "host_loop", "host_loop", "nothing", "chain", "host_loop", "host_loop", "host_loop", "chain"]


def test_chain_knobs_flip_the_field_they_document():
    narrow, two, three = dict(m=16, k=8), dict(m=16, k=32), dict(m=16, k=48)
    # knob 6 value: (case, cooldown, field -> (without, with))
    table = {3: (narrow, 2, {"take": ("chain", "host_loop"), "fold": (1, 0)}), 5: (narrow, 2, {"fold": (1, 0)}), 6: (narrow, 2, {"fold": (1, 2)}),
             7: (three, 0, {"wide_gramx": (1, 0)}), 9: (two, 0, {"wide_xw": (1, 0)}), 10: (three, 0, {"wide_xw": (0, 1)}),
             12: (narrow, 0, {"x3": (1, 0)}), 13: (narrow, 2, {"x3": (0, 1)})}
    lines = [POLICIES["plain"]]
    for knob, (case, cd, _) in table.items():
        lines += [env_line(), chain_line(cooldown=cd, **case), env_line(t6=knob), chain_line(cooldown=cd, **case)]
    res, _ = run_plans(lines)
    for i, (knob, (case, cd, flips)) in enumerate(table.items()):
        off, on = res[2 * i][0], res[2 * i + 1][0]
        for field in ("take", "fold", "x3", "wide_gramx", "wide_xw"):
            want = flips.get(field, (off[field], off[field]))
            assert (off[field], on[field]) == want, (knob, field, off, on)


def test_default_and_closed_plans():
    _, op = run_plans([env_line()])
    G, T, XU, C, F, GX, GW, XW, CX, CL, TC = (op[k] for k in ("GRAM_UU", "TRMMG", "XU", "COMBO", "FINAL", "GRAMX", "GRAMW", "XW", "COMBOX", "CLOSE", "TRMMC"))
    # ChainShape: k m fold vsx wide_gramx wide_xw dropf x3 -> the schedule its comments state
    shapes = {"13 26 1 1 0 0 0 1": [GX, CX, CX, CL, F], "13 26 1 1 0 0 0 0": [GX, C, T, XW, C, F], "32 16 0 1 1 1 0 0": [GX, C, XW, C, F],
              "48 16 0 1 1 0 0 0": [GX, C, T, XU, C, F], "32 16 0 1 0 0 0 0": [G, T, XU, C, T, XU, C, F], "13 0 2 0 0 0 0 0": [G, T, F]}
    res, _ = run_plans(["default " + s for s in shapes])
    assert [d["ops"] for d, _ in res] == list(shapes.values())
    # plans as chains remember them: the defaults, and executed lists that ended early, pending, or with the closing sweep
    plans = list(shapes.values()) + [[GX, CX], [GX, CX, CX], [GX, CX, CX, CL], [T, GW, CX, CX, CL, F], [TC, XW, XU, CX], [GX, C, T, XW, C], [G], [CL, F], [F]]
    cases = [(plan, lean, x3) for plan in plans for lean in (0, 1) for x3 in (0, 1)]
    res, _ = run_plans(["close %d %d %s" % (lean, x3, " ".join(map(str, plan))) for plan, lean, x3 in cases])
    for (plan, lean, x3), (d, _) in zip(cases, res):
        out = d["ops"]
        what = (plan, lean, x3, out)
        if lean:
            assert out and (len(out) == 1 or out[-1] not in (F, CL)), what
            assert out == plan[:len(out)] and all(o in (F, CL) for o in plan[len(out):]), what       # only the closing launches went
        else:
            assert out[-1] == F, what
            assert not x3 or CL in out, what
            kept = [o for o in out if o not in (F, CL)]
            assert kept == [o for o in plan if o not in (F, CL)], what                                # every measuring sweep stays, in order


def test_lean_predicate():
    """lean: the caller takes the closing block (rebuilt), the block fits the pending buffer, and every step reports in its reduction"""
    reqs = ["lean 26 13 0 1 0", "lean 0 13 0 1 0", "lean 630 13 0 1 0", "lean 26 13 0 2 0", "lean 26 13 0 1 1", "lean 26 13 1 4 0", "lean 500 40 1 4 0"]
    res, _ = run_plans([env_line(), POLICIES["rebuilt"]] + reqs + [POLICIES["plain"], reqs[0], POLICIES["tight"], reqs[0],
                                                                    env_line(t6=17), POLICIES["rebuilt"], reqs[0], env_line(t6=4), reqs[5]])
    assert [d["lean"] for d, _ in res] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0]
