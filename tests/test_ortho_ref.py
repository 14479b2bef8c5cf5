"""CPU: what tests/test_ortho_ref_gpu.py rests on, shown without a GPU (tests/ortho_ref.py holds the reference, the cases, the checkers).

a. The long-double reference reproduces what the UNMODIFIED reference computed (the ocd* and ovx* entries of
   tests/golden/reference_fixtures.npz) within the checkers' own bounds.
b. Where the Cholesky-based reference of the metric module (ref_b_ortho_vs_x(x, x, u)) runs, the two references agree to 1e-16 a;
   on the blocks graded to condition 1e10 it does not run on every one, which is why it is not the reference here.
c. On every case of the GPU test the double-precision oracle (ortho_cd, ortho_vs_x) passes the same checkers with a worst ratio of
   0.25: the bounds leave the device a factor 4 over what double arithmetic in the reference's own order achieves.  A condition on
   the inputs, not on the library.
d. The generators deliver what they promise; in particular the double-precision Gram matrix of every graded1e10 and rank-deficient
   block has no Cholesky factorisation, so any correct implementation takes the level-shift ladder on them.
e. The same cases through the product's host logic on the host-memory engine, in a worker process (tests/hostsim.py; the library a
   process has loaded cannot be exchanged): the host-driven loop that k = 49 and separate panels take on the device.

$DIAGLIB_ORTHO_REF_RECORD names a file the worst ratios of every case are appended to (profiles/ortho_ref.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import metric_ortho_ref as M
import ortho_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.environ.get("DIAGLIB_ORTHO_REF_RECORD")


@pytest.fixture(scope="module")
def cases():
    """every case with its reference, built once (the worker of test e reads them from a file instead of computing them again)"""
    for key in R.ALL_CASES:
        R.case(*key).ref()
    return R


# ------------------------------------------------------------------------------------------------------------------ a. the golden fixture
def test_reference_reproduces_the_unmodified_reference():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "reference_fixtures.npz"))
    rows = []
    for i in range(int(gold["ocd_count"])):
        assert bool(gold[f"ocd{i}_ok"])
        c = R.Given(f"golden_ocd{i}", None, gold[f"ocd{i}_in"])
        rows.append(("reference " + c.name, R.check(gold[f"ocd{i}_out"], c)))
    for i in range(int(gold["ovx_count"])):
        c = R.Given(f"golden_ovx{i}", gold[f"ovx{i}_x"], gold[f"ovx{i}_u"])
        rows.append(("reference " + c.name, R.check(gold[f"ovx{i}_out"], c)))
    assert len(rows) == 8
    R.record(RECORD, rows)


# ------------------------------------------------------------------------------------------------------------------ b. the two references
def test_gram_schmidt_and_cholesky_references_agree_where_the_cholesky_one_runs(cases):
    ran, broke = [], []
    for key in R.ALL_CASES:
        c = R.case(*key)
        if not c.unique:
            continue
        try:
            q = M.ref_b_ortho_vs_x(c.x, c.x, c.u).q
        except (np.linalg.LinAlgError, RuntimeError):
            broke.append(c)
            continue
        ran.append(c)
        assert float(np.abs(q - c.ref().q).max()) <= 1e-16 * c.ref().a, c.name
    assert all(c.kind == "graded1e10" for c in broke), [c.name for c in broke]
    assert len(ran) >= sum(1 for key in R.ALL_CASES if not key[3] in R.NEEDS_SHIFT), (len(ran), len(broke))


# ------------------------------------------------------------------------------------------------------------------ c. the oracle at a quarter
def _oracle(oracle, c):
    if c.m == 0:
        q, _, ok, _ = oracle.ortho_cd(c.u)
        return q, 0 if ok else 1
    q, _, st = oracle.ortho_vs_x(c.x, c.u)
    return q, st


def test_oracle_meets_a_quarter_of_every_bound(cases, oracle):
    rows = []
    for key in R.ALL_CASES:
        c = R.case(*key)
        q, st = _oracle(oracle, c)
        assert st == 0, c.name
        rows.append(("oracle " + c.name, R.check(q, c, what=c.name, limit=0.25)))
    R.record(RECORD, rows)


# ------------------------------------------------------------------------------------------------------------------ d. the generators
def test_generators_deliver_what_they_promise(cases, oracle):
    seen = dict.fromkeys(("near_span", "colscaled", "graded1e6", "graded1e10", "rank_deficient", "x"), 0)
    for key in R.ALL_CASES:
        c = R.case(*key)
        r = c.ref()
        if c.kind == "near_span":
            assert r.a >= 1e5, (c.name, r.a)
        if c.kind == "colscaled":
            assert r.a > 1e15 and r.a_eq < 10, (c.name, r.a, r.a_eq)
        if c.kind.startswith("graded"):
            cond = R.graded_cond(c.kind)
            assert cond / 2 <= r.kappa_p <= cond * 2, (c.name, r.kappa_p)         # of P, not only of U
        if c.kind == "graded1e6":
            assert not R.cholesky_fails(R.first_gram(c)), c.name                # no shift needed
        if c.kind in R.NEEDS_SHIFT:
            g = R.first_gram(c)
            assert R.cholesky_fails(g) and oracle.potrf_lower(g)[1] != 0, c.name
        if c.kind == "rank_deficient":
            assert np.array_equal(c.u[:, -1], c.u[:, 0] + c.u[:, 1])
        if c.kind in seen:
            seen[c.kind] += 1
        if c.m:
            xl = np.asarray(c.x, R.LD)
            assert np.abs(xl.T @ xl - np.eye(c.m)).max() <= 8 * R.EPS, c.name
            assert abs(r.pi - 1) <= 4 * c.m * R.EPS, (c.name, r.pi)                # (a double-precision SVD of m columns)
            seen["x"] += 1
    assert seen == {"near_span": 6, "colscaled": 10, "graded1e6": 10, "graded1e10": 20, "rank_deficient": 20,
                    "x": sum(1 for key in R.ALL_CASES if key[1])}, seen


def test_the_case_table_is_the_one_the_gpu_test_needs():
    keys = set(R.ALL_CASES)
    assert len(R.ALL_CASES) == len(keys) == 140
    for k in R.WIDTHS:
        assert {(2000, 26, k, "random"), (2001, 26, k, "random"), (2000, 0, k, "random"), (2001, 0, k, "random")} <= keys
    # the block that follows a rank-deficient one, and the blocks between guard columns, have been through test c
    assert all(R.well_conditioned_twin(key) in keys for key in R.ALL_CASES if key[3] == "rank_deficient")
    assert set(R.GUARD_CASES) <= keys
    names = {f"std_n{n}_m{m}_k{k}_{kind}" for n, m, k, kind in R.ALL_CASES}
    assert set(R.DRAWS) <= names, set(R.DRAWS) - names


# ------------------------------------------------------------------------------------------------------------------ e. the host logic
WORKER = r"""
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import hostsim
import ortho_ref as R
from diaglib_amd import capi
capi.load(hostsim.build())
R.load_cases({cases!r})
ctx = capi.Context()
assert ctx.backend.startswith("hostsim")
out = {{}}
for key in {keys!r}:
    c = R.case(*key)
    if c.m == 0:
        p = ctx.panel(c.u)
        g, ok = ctx.ortho_cd(p)
        assert ok, c.name
        out["hostsim ortho_cd " + c.name] = R.check(p.download(), c, what=c.name)
        continue
    got = []
    for one_panel in (False, True):
        if one_panel:
            big = ctx.panel(np.asfortranarray(np.hstack([c.x, c.u]))); px, pu = big.col(0, c.m), big.col(c.m, c.k)
        else:
            px, pu = ctx.panel(c.x), ctx.panel(c.u)
        ctx.ortho_vs_x(px, pu)
        got.append(pu.download())
        out[f"hostsim vs_x panels={{2 - one_panel}} " + c.name] = R.check(got[-1], c, px.download(), what=c.name)
    if c.unique:
        assert np.abs(got[0] - got[1]).max() <= R.q_bound(c.ref()), c.name
with open({out!r}, "w") as f:
    json.dump(out, f)
print("host logic: ok")
"""


def test_the_host_logic_passes_the_same_checkers_on_the_host_engine(cases, tmp_path):
    cases_file, out_file = str(tmp_path / "cases.pkl"), str(tmp_path / "ratios.json")
    R.dump_cases(cases_file)
    script = tmp_path / "ortho_worker.py"
    script.write_text(WORKER.format(root=ROOT, cases=cases_file, out=out_file, keys=R.ALL_CASES))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "host logic: ok" in p.stdout
    with open(out_file) as f:
        ratios = json.load(f)
    assert len(ratios) == sum(2 if key[1] else 1 for key in R.ALL_CASES)
    R.record(RECORD, sorted(ratios.items()))
