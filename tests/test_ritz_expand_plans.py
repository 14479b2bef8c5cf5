"""CPU: the planner of the Ritz sweep that also forms and measures the next block (ritz_expand_plan of diaglib_amd/csrc/hip_plans.h)
against its own transcription.

tests/ritz_expand_plans_driver.cpp is compiled with g++ and no ROCm include, as tests/test_plans.py compiles its driver.  The
transcription below is the arithmetic of the kernel's comment: tx = ceil(m / 16) tiles of the basis, the same of its operator image and
one output tile are staged per wave, 16 rows of 18 doubles per column, four waves per block; the sweep takes even n on the 16-byte
path, blocks of one tile, up to seven basis tiles, and declines an image beyond the LDS limit or under knob 0 = 16."""
import itertools
import os
import subprocess

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "ritz_expand_plans_driver.cpp")
DEPS = [SRC, os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_plans.h"), os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "dla_internal.h"),
        os.path.join(hostsim.ROOT, "include", "diaglib_amd.h")]
EXE = os.path.join(hostsim.BUILD, "ritz_expand_plans_driver")
KIB = 1024
TILES = (1, 2, 3, 4, 5, 6, 7)


def run(lines):
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([EXE], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    res = []
    for ln in p.stdout.splitlines():
        fields, _, name = ln.partition(" | ")
        res.append(({kv.split("=")[0]: kv.split("=")[1] for kv in fields.split()}, name))
    return res


def transcription(ncu, lds_limit, knob0, n, m, nb, first0, vec2):
    tx = -(-m // 16)
    lds = 8 * 4 * 16 * (2 * tx + 1) * 18
    fits = bool(vec2 and n > 0 and n % 2 == 0 and m > 0 and 0 < nb <= 16 and 0 <= first0 < nb and tx in TILES and lds <= lds_limit and knob0 != 16)
    # the grid and the rows per step of the measuring sweep it stands in for (wp_plan): one block per CU, two up to five basis tiles, at
    # least sixteen 32-row chunks per block; 32 rows at a time up to two basis tiles (WP_TILES); widths without an instance there
    # (nine and eleven tiles round up) never fit here
    chunks = -(-n // 32)
    tlw = tx if tx <= 8 else 10 if tx <= 10 else 12
    blocks = max(1, min(ncu * (2 if tlw <= 5 else 1), -(-chunks // 16)))
    return {"tx": tx, "staged_tiles": 2 * tx + 1, "lds": lds, "fits": int(fits), "blocks": blocks, "rows": 32 if tx <= 2 else 16, "ncol": 16, "nslots": 1, "gram_slots": tx + 1,
            "small": 32}, f"davidson_expand_kernel<{tx}>"


def test_the_instance_list_is_the_transcribed_one():
    (fields, _), = run(["instances"])
    assert tuple(int(v) for v in fields["tiles"].split(",")) == TILES


def test_plans_against_the_transcription():
    shapes = list(itertools.product([66, 4098, 250_000, 2_000_000, 67], [1, 13, 16, 17, 48, 97, 105, 112, 113, 128], [(13, 0), (13, 4), (13, 12), (16, 0), (17, 0), (13, 13)],
                                    [1, 0]))
    envs = [(256, 160 * KIB, 0), (256, 135 * KIB, 0), (256, 64 * KIB, 0), (304, 160 * KIB, 0), (8, 160 * KIB, 0), (256, 160 * KIB, 16), (256, 160 * KIB, 17)]
    for ncu, lds, knob0 in envs:
        lines = [f"env {ncu} {lds} {knob0}"] + [f"plan {n} {m} {nb} {f0} {v}" for n, m, (nb, f0), v in shapes]
        got = run(lines)
        assert len(got) == len(shapes)
        for (n, m, (nb, f0), v), (fields, name) in zip(shapes, got):
            want, want_name = transcription(ncu, lds, knob0, n, m, nb, f0, v)
            assert {key: int(val) for key, val in fields.items()} == want and name == want_name, (ncu, lds, knob0, n, m, nb, f0, v, fields, want)


def test_the_limits_the_design_states():
    """seven basis tiles (m <= 112) fit 135 KiB exactly, the headline's 105 columns with them; 113 columns have no instance; under a
    refused LDS request (64 KiB) up to 48 columns still fit and 49 do not; odd n, a misaligned panel and a 17-column block decline"""
    def fits(lds, n, m, nb=13, f0=0, vec2=1, knob0=0):
        return int(run([f"env 256 {lds} {knob0}", f"plan {n} {m} {nb} {f0} {vec2}"])[0][0]["fits"])
    assert 8 * 4 * 16 * 15 * 18 == 135 * KIB
    assert fits(135 * KIB, 2_000_000, 112) and fits(135 * KIB, 2_000_000, 105) and not fits(135 * KIB - 1, 2_000_000, 112)
    assert fits(135 * KIB - 1, 2_000_000, 96) and not fits(160 * KIB, 2_000_000, 113)
    assert fits(64 * KIB, 2_000_000, 48) and not fits(64 * KIB, 2_000_000, 49)
    assert not fits(160 * KIB, 2_000_001, 48) and not fits(160 * KIB, 2_000_000, 48, vec2=0) and not fits(160 * KIB, 2_000_000, 48, nb=17)
    assert not fits(160 * KIB, 2_000_000, 48, knob0=16) and fits(160 * KIB, 2_000_000, 48, knob0=17)
