#!/usr/bin/env python3
"""Golden fixture of tests/test_oracle.py::test_live_reference_if_present: what the UNMODIFIED reference (oracle/_ref built by
`make -C oracle ref`) returns on that test's inputs, so that the test compares the oracle with the reference also where the
reference cannot be built.

    python tests/golden/make_golden_live.py      ->  tests/golden/reference_live_fixtures.npz

Data only: the input is the test's seeded array (stored, and checked by the test), the outputs are what the reference returned.
"""
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "8")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
from make_golden import save_npz_lzma  # noqa: E402


def main():
    from oracle.pyoracle import Oracle, Reference
    o, ref = Oracle(), Reference()
    u = np.asfortranarray(np.random.default_rng(12345).standard_normal((500, 9)))     # tests/conftest.py: the `rng` fixture
    b, gb, okb = ref.ortho_cd(u)
    n, t, m = 800, 5, 9
    o.dense_setup(n)
    g = np.zeros((n, m), order="F"); g[np.arange(m), np.arange(m)] = 1.0
    er, _, okr = ref.davidson(n, t, m, 100, 1e-9, 20, 0.0, o.fn("orc_dense_matvec"), o.fn("orc_dense_precnd"), g)
    path = os.path.join(HERE, "reference_live_fixtures.npz")
    save_npz_lzma(path, u=u, ortho_cd_out=b, ortho_cd_g=gb, ortho_cd_ok=okb, dav_n800_eig=er, dav_n800_ok=okr)
    print("wrote", path, "ortho_cd ok", okb, "davidson ok", okr)


if __name__ == "__main__":
    main()
