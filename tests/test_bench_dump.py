"""CPU: bench.py --dump-outputs -- the row sample of the eigenvector block is fixed by the arguments, stays within the size
limit, and the shards of an N-rank run put together the same rows a 1-rank run writes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import DUMP_ROWS, dump_outputs, dump_rows, shard_rows  # noqa: E402


def test_row_sample_is_fixed_sorted_and_bounded():
    a, b = dump_rows(2_000_000, 13), dump_rows(2_000_000, 13)
    assert np.array_equal(a, b) and a.size == DUMP_ROWS
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 2_000_000
    assert np.array_equal(dump_rows(1000, 13), np.arange(1000))          # small problems are written whole
    for n_max in (13, 37, 69, 133):
        assert dump_rows(10_000_000, n_max).size * n_max * 8 + 8 * n_max <= 64 << 20


def test_dump_writes_float64_rows_of_the_block(tmp_path):
    n, n_max = 300_000, 13
    x = np.asfortranarray(np.random.default_rng(7).standard_normal((n, n_max)))
    eig = np.linspace(1.0, 2.0, n_max)
    dump_outputs(str(tmp_path), eig, x, n, 0, 1, 0)
    got_e = np.load(tmp_path / "eigenvalues.npy")
    got_v = np.load(tmp_path / "eigenvectors_sample.npy")
    assert got_e.dtype == np.float64 and np.array_equal(got_e, eig)
    assert got_v.dtype == np.float64 and np.array_equal(got_v, x[dump_rows(n, n_max)])
    # what every rank of a 4-rank run contributes, in rank order, is the same sample
    parts = []
    for r in range(4):
        r0, nl = shard_rows(n, 4, r)
        rows = dump_rows(n, n_max)
        mine = rows[(rows >= r0) & (rows < r0 + nl)]
        parts.append(x[r0:r0 + nl][mine - r0])
    assert np.array_equal(np.concatenate(parts), got_v)
