"""Failure contracts of the HIP engine's resource owners (diaglib_amd/csrc/hip_owned.h), on the CPU.

tests/owned_buffers_driver.cpp instantiates DeviceBuffer, MappedHostBuffer and the event owner with a counting fake runtime
that can fail its n-th allocation, and prints what it saw; the assertions are here.  The header is compiled with g++ and no
ROCm include, the way tests/hostsim.py compiles its library (tests/_build/, $DIAGLIB_HOSTSIM_SANITIZE honoured)."""
import os
import subprocess

import pytest

import hostsim

SRC = os.path.join(hostsim.ROOT, "tests", "owned_buffers_driver.cpp")
HDR = os.path.join(hostsim.ROOT, "diaglib_amd", "csrc", "hip_owned.h")
EXE = os.path.join(hostsim.BUILD, "owned_buffers_driver")


@pytest.fixture(scope="module")
def seen():
    os.makedirs(hostsim.BUILD, exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in (SRC, HDR)):
        p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + hostsim.SAN + [SRC, "-o", EXE],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
    p = subprocess.run([EXE], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {}
    for line in p.stdout.split():
        key, val = line.split("=")
        scen, name = key.split(".")
        out.setdefault(scen, {})[name] = int(val)
    return out


KINDS = ("dev", "map")
SCENARIOS = ("dev_grow", "dev_noop", "dev_move", "map_grow", "map_noop", "map_move", "map_alias", "event")


@pytest.mark.parametrize("kind", KINDS)
def test_failed_reserve_leaves_buffer_empty(seen, kind):
    s = seen[kind + "_grow"]
    assert s["first_ok"] == 1
    assert s["regrow_failed"] == 1
    assert s["empty_after_failure"] == 1          # null pointer (and null alias), capacity 0
    assert s["old_released"] == 1                 # exactly once ...
    assert s["old_still_live"] == 0               # ... and it was the old block


@pytest.mark.parametrize("kind", KINDS)
def test_reserve_after_failure_succeeds_and_releases_once(seen, kind):
    s = seen[kind + "_grow"]
    assert s["retry_ok"] == 1
    assert s["releases_before_exit"] == 1
    assert s["releases_after_exit"] == 2          # the old block at the regrow, the new one at destruction


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_allocations_and_releases_balance(seen, scenario):
    assert seen[scenario]["live_at_exit"] == 0
    assert seen[scenario]["bad_release"] == 0     # nothing released twice


@pytest.mark.parametrize("kind", KINDS)
def test_reserve_within_capacity_makes_no_runtime_call(seen, kind):
    s = seen[kind + "_noop"]
    assert s["ok"] == 1
    assert s["runtime_calls"] == 0
    assert s["unchanged"] == 1


def test_device_alias_follows_host_block(seen):
    s = seen["map_alias"]
    assert s["first"] == 1
    assert s["regrown"] == 1
    assert s["alias_calls"] == 2                  # re-derived at the regrow, not cached from the first block
    assert s["alias_failed"] == 1 and s["empty_after_failure"] == 1 and s["retry_ok"] == 1
    assert s["unmapped"] == 1
    # the grow and move scenarios check dev() against host() after every step as well
    assert seen["map_grow"]["retry_ok"] == 1 and seen["map_move"]["assigned"] == 1


@pytest.mark.parametrize("kind", KINDS)
def test_moved_from_releases_nothing(seen, kind):
    s = seen[kind + "_move"]
    assert s["constructed"] == 1
    assert s["assigned"] == 1
    assert s["releases_after_assignment"] == 1    # the target's own block
    assert s["moved_from_regrows"] == 1
    assert s["releases_after_exit"] == 3          # + the moved block once + the moved-from object's new block


def test_event_ensure_creates_once(seen):
    s = seen["event"]
    assert s["starts_empty"] == 1
    assert s["create_failed"] == 1
    assert s["ensure_twice"] == 1
    assert s["creates"] == 2                      # the failed attempt and one creation for two ensure() calls
    assert s["destroys_before_exit"] == 0
    assert s["destroys_after_exit"] == 1
