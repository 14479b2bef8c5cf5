"""One rank of a row-sharded run in ONE process: the test plays the other ranks.

With the hook transport (dla_set_allreduce_hook) every collective of an engine hands its buffer to fn(buf, count, op) and takes the
buffer back.  A test that knows the global problem can therefore be rank r of N: it sees what this rank contributed before the sum,
writes into the buffer what the N - 1 peers would have added, and holds every path that exists only for nranks > 1 -- the halo pack
and gather of the sharded ELLPACK product, the slot layout of the Ritz reduction, the sample operators at row0 != 0, the set-up
agreements and their refusals -- to an exact or np.longdouble reference of the global problem.  No child processes, no gloo; the
peer-to-peer mailboxes and RCCL cannot be played this way and stay with tests/test_multirank_gpu.py and tests/test_spmm_sharded.py.

  Peers        the scripted hook: a test queues the exchanges it expects, in order, as (count, op, player); player(buf) edits the buffer
               in place like the peers' part of the reduction.  A Python exception inside a ctypes callback is swallowed, so the hook
               never asserts: it records every call as (count, op, buffer as it arrived, buffer as it left), leaves the buffer alone on
               a mismatch and sets a flag.  peers.check() raises with the whole call list.
  players      the layouts are those of the comments in the code, which are the contract:
                 shard agreement  [row0 per rank | tag per rank | n_global per rank]            (host_logic.cpp: agree_on_shards)
                 sharded set-up   [need, bad] under max, then [row0, n] per rank under sum      (spmm_setup_csr_sharded)
                 halo             buf[((r 2 + side) m + c) halo + h]                            (halo_pack_kernel)
                 small products   column-major l x k, the peers' partial is added               (gram, W^T x)
                 Ritz             [ncol sums | nranks x ncol maxima], one sum                   (ritz_reduce_kernel); the host engine
                                  makes two exchanges instead (n_res sums, then n_res maxima under max)
                 nrm2             one double
  references   np.longdouble on the global problem
  checkers     plain functions of (ctx, case): tests/test_shard_peers_gpu.py calls them on the HIP context, tests/test_shard_peers.py
               runs this file as a program on the host-memory engine (python tests/shard_peers.py OUT.json) -- the library a process
               has loaded cannot be exchanged.  The case lists are module-level data and both files run the same lists.
WORST keeps the largest |got - ref| / bound per family."""
import json
import os
import sys
import zlib

import numpy as np
import scipy.sparse as sp

if __name__ == "__main__":          # (as a program: the package lives one directory up)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dense_ref as D
from diaglib_amd import capi
from test_operators_gpu import LD, Guarded, assert_within

EPS = D.EPS
SUM, MAX = 0, 1
P2P_MAX_DOUBLES = 16384            # a mailbox slot of the peer-to-peer transport: the column chunks of the sharded product are cut to it
NAN = float("nan")
WORST = {}


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


def is_hip(ctx):
    return ctx.backend.startswith("hip:")


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def zero_bits(a):
    """every entry is +0.0"""
    return not np.any(D.bits(np.ascontiguousarray(a, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------------------------ the layout
class Layout:
    """contiguous row shards in rank order, seen from `rank`"""

    def __init__(self, shards, rank):
        self.shards, self.rank, self.nranks = [int(s) for s in shards], int(rank), len(shards)
        self.row0 = [int(v) for v in np.concatenate([[0], np.cumsum(self.shards)[:-1]])]
        self.n_global = int(sum(self.shards))
        self.n, self.r0 = self.shards[rank], self.row0[rank]

    def rows(self, r=None):
        r = self.rank if r is None else r
        return slice(self.row0[r], self.row0[r] + self.shards[r])

    def others(self):
        mask = np.ones(self.n_global, bool)
        mask[self.rows()] = False
        return mask

    def __repr__(self):
        return f"rank {self.rank} of {self.shards}"


# ------------------------------------------------------------------------------------------------------------------ the scripted hook
class Peers:
    """with Peers(ctx, nranks, rank) as peers: the hook is installed; on exit it is removed and the shard is withdrawn"""

    def __init__(self, ctx, nranks, rank):
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        self.queue, self.calls, self.problems = [], [], []

    def __enter__(self):
        self.ctx.set_allreduce_hook(self._hook, self.nranks, self.rank)
        return self

    def __exit__(self, *exc):
        self.ctx.set_allreduce_hook(None, 1, 0)
        self.ctx.set_shard(-1, 0)
        return False

    def expect(self, *exchanges):
        for count, op, player in exchanges:
            self.queue.append((int(count), int(op), player))

    def announce(self, lay, **wrong):
        """dla_set_shard with the peers announcing theirs (wrong: see agreement)"""
        self.expect(agreement(lay, **wrong))
        self.ctx.set_shard(lay.n_global, lay.r0)

    def _hook(self, buf, op):
        before = buf.copy()
        try:
            if not self.queue:
                self.problems.append(f"call {len(self.calls)}: nothing was expected")
            elif (self.queue[0][0], self.queue[0][1]) != (len(buf), op):
                self.problems.append(f"call {len(self.calls)}: expected (count, op) = {self.queue[0][:2]}")
            else:
                _, _, player = self.queue.pop(0)
                try:
                    player(buf)
                except Exception as e:          # noqa: BLE001 -- (nothing may leave a ctypes callback)
                    buf[:] = before
                    self.problems.append(f"call {len(self.calls)}: the player raised {e!r}")
        finally:
            self.calls.append((len(buf), int(op), before, buf.copy()))

    def check(self):
        """raises unless every call was the expected one and every expected call came"""
        if self.queue:
            self.problems.append(f"{len(self.queue)} expected exchange(s) never came: {[q[:2] for q in self.queue]}")
            self.queue = []
        if self.problems:
            problems, self.problems = self.problems, []
            listing = "\n".join(f"  {i}: count {c} op {'sum' if o == SUM else 'max'} arrived {_short(b)} left {_short(a)}"
                                for i, (c, o, b, a) in enumerate(self.calls))
            raise AssertionError("; ".join(problems) + "\nthe calls of this rank:\n" + listing)


def _short(a):
    return np.array2string(a, threshold=12, edgeitems=4, precision=6)


# ------------------------------------------------------------------------------------------------------------------ players
def agreement(lay, row0_of=None, tag_shift=None, n_global_of=None):
    """agree_on_shards: [row0 of every rank | a tag per rank | n_global per rank]; the peers copy this rank's tag.
    row0_of / tag_shift / n_global_of: {peer: what it announces instead}"""
    row0_of, tag_shift, n_global_of = row0_of or {}, tag_shift or {}, n_global_of or {}
    nr, me = lay.nranks, lay.rank

    def play(buf):
        for r in range(nr):
            if r != me:
                buf[r] += row0_of.get(r, lay.row0[r])
                buf[nr + r] += buf[nr + me] + tag_shift.get(r, 0.0)
                buf[2 * nr + r] += n_global_of.get(r, lay.n_global)
    return (3 * nr, SUM, play)


def setup_exchanges(lay, peer_need=0, peer_bad=0, row0_of=None, n_of=None):
    """spmm_setup_csr_sharded: [max need | any failure] under max, then [row0, n] of every rank under sum"""
    row0_of, n_of = row0_of or {}, n_of or {}

    def play_max(buf):
        buf[0], buf[1] = max(buf[0], float(peer_need)), max(buf[1], float(peer_bad))

    def play_layout(buf):
        for r in range(lay.nranks):
            if r != lay.rank:
                buf[2 * r] += row0_of.get(r, lay.row0[r])
                buf[2 * r + 1] += n_of.get(r, lay.shards[r])
    return [(2, MAX, play_max), (2 * lay.nranks, SUM, play_layout)]


def halo_exchange(lay, halo, xc):
    """one exchange of the sharded product for the columns xc of the GLOBAL x: the neighbours' near sides are filled from x, every slot
    this rank must not read -- the neighbours' far sides and all other ranks -- becomes NaN"""
    nr, me, m = lay.nranks, lay.rank, xc.shape[1]

    def play(buf):
        b = buf.reshape(nr, 2, m, halo)
        for r in range(nr):
            if r == me:
                continue
            rows = np.arange(lay.row0[r], lay.row0[r] + lay.shards[r])
            for side in (0, 1):
                if (r == me - 1 and side == 1) or (r == me + 1 and side == 0):
                    b[r, side] += xc[rows[:halo] if side == 0 else rows[-halo:]].T
                else:
                    b[r, side] += NAN
    return (nr * 2 * m * halo, SUM, play)


def halo_columns(ctx, lay, halo, m):
    """the column chunks of one sharded product with m right-hand sides: spmm_matvec_sharded cuts to a mailbox slot, the host engine
    sends the block whole"""
    if halo == 0 or lay.nranks == 1:
        return []
    mc = max(1, min(m, P2P_MAX_DOUBLES // (lay.nranks * 2 * halo))) if is_hip(ctx) else m
    return [min(mc, m - c0) for c0 in range(0, m, mc)]


def halo_exchanges(ctx, lay, halo, xg):
    out, c0 = [], 0
    for mcur in halo_columns(ctx, lay, halo, xg.shape[1]):
        out.append(halo_exchange(lay, halo, xg[:, c0:c0 + mcur]))
        c0 += mcur
    return out


def small_sum(peer_partial):
    """a small product (gram, W^T x): column-major l x k, the peers' partial is added"""
    flat = np.asarray(peer_partial, dtype=np.float64).ravel(order="F")

    def play(buf):
        buf += flat
    return (flat.size, SUM, play)


def ritz_columns(m):
    """columns of the HIP engine's Ritz reduction: whole 16-column tiles (hip_plans.h: ritz_grid)"""
    return 16 * ((m + 15) // 16)


def ritz_exchanges(ctx, lay, m, n_res, peer_sums, peer_max):
    """the norms of a Ritz sweep.  HIP engine: [ncol sums | nranks x ncol maxima] in ONE sum; host engine: n_res sums, then n_res
    maxima under max.  peer_sums[j]: what the peers add to root j; peer_max[r][j]: the maximum of peer r (this rank's row is ignored)"""
    nr, me = lay.nranks, lay.rank
    if is_hip(ctx):
        ncol = ritz_columns(m)

        def play(buf):
            buf[:n_res] += peer_sums[:n_res]
            for r in range(nr):
                if r != me:
                    buf[ncol + r * ncol:ncol + r * ncol + n_res] += peer_max[r][:n_res]
        return [(ncol * (1 + nr), SUM, play)]

    def play_sum(buf):
        buf += peer_sums[:n_res]

    def play_max(buf):
        for r in range(nr):
            if r != me:
                np.maximum(buf, peer_max[r][:n_res], out=buf)
    return [(n_res, SUM, play_sum), (n_res, MAX, play_max)]


def ritz_views(ctx, lay, m, n_res, calls):
    """(this rank's sums, its maxima, the other ranks' slots, the summed sums, the maximum over what the hook left) of the exchanges"""
    nr, me = lay.nranks, lay.rank
    if is_hip(ctx):
        (_, _, before, after), = calls
        ncol = ritz_columns(m)
        slots_b, slots_a = before[ncol:].reshape(nr, ncol), after[ncol:].reshape(nr, ncol)
        return before[:n_res], slots_b[me, :n_res], np.delete(slots_b, me, 0), after[:n_res], slots_a.max(axis=0)[:n_res]
    (_, _, sb, sa), (_, _, mb, ma) = calls
    return sb, mb, np.zeros((nr - 1, 0)), sa, ma


def nrm2_exchange(peer_sumsq):
    def play(buf):
        buf[0] += peer_sumsq
    return (1, SUM, play)


# ------------------------------------------------------------------------------------------------------------------ the banded operator
def banded(lay, rng, hb, reach=(), ragged=False, blocks=False, integer=True):
    """a symmetric n_global x n_global band: the diagonal, hb pairs of diagonals and one more pair at every distance in `reach`.
    integer: entries from +-{1, 2, 3} (with an integer x every sum is exact in any order), else standard normal.  ragged: (i, i + d) is
    there iff d <= 1 + (i mod hb), mirrored -- the reach depends on the row and the rows are of different lengths.  blocks: every
    entry that couples two shards is dropped (halo = 0)."""
    n = lay.n_global
    draw = (lambda k: rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], k)) if integer else (lambda k: rng.standard_normal(k))
    owner = np.repeat(np.arange(lay.nranks), lay.shards)
    diags, offs = [draw(n)], [0]
    for d in list(range(1, hb + 1)) + list(reach):
        if d >= n:
            continue
        v = draw(n - d)
        if ragged and d <= hb:
            v = np.where(d <= 1 + (np.arange(n - d) % hb), v, 0.0)
        if blocks:
            v = np.where(owner[:n - d] == owner[d:], v, 0.0)
        diags += [v, v]
        offs += [d, -d]
    a = sp.diags(diags, offs, shape=(n, n), format="csr")
    a.eliminate_zeros()
    a.sort_indices()
    return a


def shard_need(a_rows, row0, n):
    """rows of the neighbours the columns of a shard reach into (dla_internal.h: sharded_ell_need)"""
    c = a_rows.indices.astype(np.int64)
    left, right = row0 - c[c < row0], c[c >= row0 + n] - (row0 + n - 1)
    return int(max(left.max(initial=0), right.max(initial=0)))


def ref_banded(a_rows, xg):
    """A x and |A| |x| of the rows of one shard, in long double, entry by entry"""
    coo = a_rows.tocoo()
    y, mag = np.zeros((a_rows.shape[0], xg.shape[1]), LD), np.zeros((a_rows.shape[0], xg.shape[1]), LD)
    prod = coo.data.astype(LD)[:, None] * xg.astype(LD)[coo.col]
    np.add.at(y, coo.row, prod)
    np.add.at(mag, coo.row, np.abs(prod))
    return y, mag


def call_matvec(ctx, name, n, m, xptr, yptr):
    ctx._chk(ctx.lib.dla_call_matvec(ctx.h, capi.fn_address(name), n, m, xptr, yptr))


def call_precnd(ctx, name, n, m, fac, xptr, yptr):
    ctx._chk(ctx.lib.dla_call_precnd(ctx.h, capi.fn_address(name), n, m, float(fac), xptr, yptr))


def pcase(name, shards, rank, m, hb=0, reach=(), ragged=False, blocks=False, w=None, halo=None, hip_chunks=None):
    return dict(name=name, shards=shards, rank=rank, m=m, hb=hb, reach=tuple(reach), ragged=ragged, blocks=blocks, w=w, halo=halo,
                hip_chunks=hip_chunks)


EIGHT = (40, 33, 64, 65, 41, 48, 37, 50)
# w: the stored width (the widest row of the shard) -- 3, 7, 13, 25, 33, 41 are the halo kernel's buckets 4, 8, 16, 32 and, twice, its
# runtime-width instance; halo: what the ranks agree on; hip_chunks: the columns per exchange on the HIP engine where the case is about them
PRODUCT_CASES = [
    pcase("w 3, middle of three, halo 1", (70, 65, 80), 1, 13, hb=1, w=3, halo=1),
    pcase("w 7, first of two, 63 rows", (63, 70), 0, 13, hb=3, w=7, halo=3),
    pcase("w 13, last of two, 65 rows", (70, 65), 1, 13, hb=6, w=13, halo=6),
    pcase("w 13, middle of three", (70, 65, 80), 1, 13, hb=6, w=13, halo=6),
    pcase("w 25, first of eight", EIGHT, 0, 13, hb=12, w=25, halo=12),
    pcase("w 33, middle of eight", EIGHT, 3, 13, hb=16, w=33, halo=16),
    pcase("w 41, last of eight", EIGHT, 7, 13, hb=20, w=41, halo=20),
    pcase("halo = n_local = 64, 48 columns in chunks of 42 and 6", (70, 64, 80), 1, 48, hb=2, reach=(64,), w=7, halo=64, hip_chunks=[42, 6]),
    pcase("halo = n_local, first of three", (64, 70, 66), 0, 13, hb=1, reach=(64,), w=4, halo=64),
    pcase("halo = n_local, last of three", (70, 66, 64), 2, 13, hb=1, reach=(64,), w=4, halo=64),
    pcase("one row, halo 1", (5, 1, 7), 1, 1, hb=1, w=3, halo=1),
    pcase("one row, last of eight", (3, 2, 4, 1, 5, 2, 3, 1), 7, 13, hb=1, w=2, halo=1),
    pcase("257 rows between 64 and 65", (64, 257, 65), 1, 13, hb=3, w=7, halo=3),
    pcase("one column", (70, 65, 80), 1, 1, hb=3, w=7, halo=3),
    # (ragged: the ranks need halos of different widths and agree on the widest; neither it nor the stored width is stated here)
    pcase("ragged, first of three", (70, 65, 80), 0, 13, hb=6, ragged=True),
    pcase("ragged, middle of three", (70, 65, 80), 1, 13, hb=6, ragged=True),
    pcase("ragged, last of three", (70, 65, 80), 2, 13, hb=6, ragged=True),
    pcase("block diagonal, middle of three: no exchange", (70, 65, 80), 1, 13, hb=2, blocks=True, w=5, halo=0, hip_chunks=[]),
    pcase("block diagonal, first of two: no exchange", (63, 70), 0, 48, hb=2, blocks=True, w=5, halo=0, hip_chunks=[]),
    # 3 x 2 x 4096 = 24576 doubles per column > 64 blocks x 256 threads of halo_pack_kernel: the second trip of its grid-stride loop,
    # and more than a mailbox slot: one column per exchange
    pcase("halo 4096: the second trip of the pack, one column per exchange", (4096, 4096, 4096), 1, 2, reach=(4096,), w=3, halo=4096,
          hip_chunks=[1, 1]),
]


def product_on_shard(ctx, peers, lay, case, integer):
    """inside `peers`: announce the shard, set the operator up on this rank's rows and multiply; the result, the references and the
    calls of the product.  Leaves the expected exchanges checked."""
    rng = rng_of("product", case["name"], integer)
    a = banded(lay, rng, case["hb"], case["reach"], case["ragged"], case["blocks"], integer)
    m = case["m"]
    xg = rng.choice([-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0], (lay.n_global, m)) if integer else rng.standard_normal((lay.n_global, m))
    xg = np.asfortranarray(xg)
    needs = [shard_need(a[lay.rows(r)], lay.row0[r], lay.shards[r]) for r in range(lay.nranks)]
    halo = max(needs)
    a_loc = a[lay.rows()]
    lens = np.diff(a_loc.indptr)
    w = int(lens.max())
    if case["halo"] is not None:
        assert halo == case["halo"], (case["name"], "the case is not what it says: halo", halo)
    if case["w"] is not None:
        assert w == case["w"], (case["name"], "the case is not what it says: stored width", w)
    if case["ragged"]:
        assert lens.min() < w and len(set(needs)) > 1, (case["name"], "rows of one length, or one reach on every rank")
    peers.announce(lay)
    peers.expect(*setup_exchanges(lay, peer_need=max(needs[:lay.rank] + needs[lay.rank + 1:])))
    ctx.spmm_setup_sharded(a_loc, lay.r0, lay.n_global)
    first = len(peers.calls)
    peers.expect(*halo_exchanges(ctx, lay, halo, xg))
    x_loc = xg[lay.rows()]
    gx, gy = D.NanGuarded(ctx, lay.n, m, x_loc), Guarded(ctx, lay.n, m)
    try:
        call_matvec(ctx, "dla_spmm_matvec", lay.n, m, gx.ptr, gy.ptr)
        got = gy.body()
        gx.assert_unchanged()
    finally:
        D.free(gx, gy)
    calls = peers.calls[first:]
    peers.check()
    ref, mag = ref_banded(a_loc, xg)
    return dict(got=got, ref=ref, mag=mag, w=w, halo=halo, calls=calls, x_loc=x_loc)


def check_halo_calls(ctx, lay, case, res):
    """what this rank sent: its own two slots bit-equal to the first and last `halo` rows of x, every other slot +0.0; on the HIP
    engine the columns per exchange the case names"""
    halo, what = res["halo"], case["name"]
    cols = halo_columns(ctx, lay, halo, case["m"])
    assert [c for c, _, _, _ in res["calls"]] == [lay.nranks * 2 * mc * halo for mc in cols], (what, [c for c, _, _, _ in res["calls"]], cols)
    if is_hip(ctx) and case["hip_chunks"] is not None:
        assert cols == case["hip_chunks"], (what, cols)
    c0 = 0
    for mc, (_, op, before, _) in zip(cols, res["calls"]):
        assert op == SUM, what
        b = before.reshape(lay.nranks, 2, mc, halo)
        xc = res["x_loc"][:, c0:c0 + mc]
        assert D.same_bits(b[lay.rank, 0], np.ascontiguousarray(xc[:halo].T)), (what, "side 0 is not the first rows of x")
        assert D.same_bits(b[lay.rank, 1], np.ascontiguousarray(xc[lay.n - halo:].T)), (what, "side 1 is not the last rows of x")
        assert zero_bits(np.delete(b, lay.rank, 0)), (what, "a slot of another rank is not +0.0")
        c0 += mc


def check_product(ctx, case, integer):
    """a. integer data: bit-equal to the reference, NaN-free (every slot this rank must not read arrives as NaN)
       b. random data: |got - ref| <= (w + 2) eps (|A||x|)_i, the dense operator's bound with the stored width for n"""
    lay = Layout(case["shards"], case["rank"])
    with Peers(ctx, lay.nranks, lay.rank) as peers:
        res = product_on_shard(ctx, peers, lay, case, integer)
    check_halo_calls(ctx, lay, case, res)
    got, what = res["got"], f"sharded product, {case['name']}, {'integer' if integer else 'random'} data"
    assert np.all(np.isfinite(got)), what + ": a NaN of a slot this rank must not read reached the product"
    if integer:
        assert D.same_bits(got, res["ref"].astype(np.float64)), what + ": not bit-equal to the exact product"
        return 0.0
    return note("sharded product", assert_within(got, res["ref"], {"(w + 2) eps |A||x|": (res["w"] + 2) * EPS * res["mag"], "tiny": D.TINY}, what))


# ------------------------------------------------------------------------------------------------------------------ set-up refusals
ARG, COMM = 3, 7
BASE = (70, 65, 80)
FOLLOW_UP = PRODUCT_CASES[3]           # after every refusal: a valid set-up and an exact product on the same context
assert FOLLOW_UP["shards"] == BASE and FOLLOW_UP["rank"] == 1


def rcase(name, status, text, shards=BASE, hb=6, exchanges=2, shard=None, **wrong):
    return dict(name=name, status=status, text=text, shards=shards, hb=hb, exchanges=exchanges, shard=shard, wrong=wrong)


# every case is the middle rank of three.  exchanges: how many of the set-up's two exchanges happen before the refusal;
# shard: the refusal is dla_set_shard's, with these wrong announcements
REFUSALS = [
    rcase("halo wider than this rank's shard", ARG, "spmm_setup_csr_sharded: a shard reaches beyond its neighbour (halo wider than a shard)",
          shards=(70, 4, 80)),
    rcase("halo wider than a peer's shard", ARG, "spmm_setup_csr_sharded: a shard reaches beyond its neighbour (halo wider than a shard)",
          shards=(70, 65, 4)),
    rcase("shards not contiguous", ARG, "spmm_setup_csr_sharded: the shards are not contiguous in rank order", row0_of={2: 140}),
    rcase("shards that do not cover n_global", ARG, "spmm_setup_csr_sharded: the shards do not cover n_global rows", n_of={2: 70}),
    rcase("halo above 4096", ARG, "spmm_setup_csr_sharded: halo wider than 4096 rows (not a banded matrix)", shards=(5000, 5000, 5000), hb=1,
          peer_need=4097),
    rcase("a peer reports bad = 1", ARG, "spmm_setup_csr_sharded: another rank rejected its shard", exchanges=1, peer_bad=1),
    rcase("a peer announces another n_global", ARG, "dla_set_shard: the ranks announce different global row counts", shard=dict(n_global_of={0: 216})),
    rcase("a peer with another tag", COMM,
          "dla_set_shard: the ranks are not at the same agreement (shards announced / transports attached in different orders)", shard=dict(tag_shift={2: 1.0})),
    rcase("an empty peer shard", ARG, "dla_set_shard: a rank holds no rows (fewer rows than the layout needs for this many ranks)",
          shard=dict(row0_of={2: 70})),
]


def check_refusal(ctx, case):
    """the status and the full text of a refused set-up -- a return, nothing is left waiting -- and then, on the same context and under
    the same hook, a valid set-up whose product is exact"""
    lay, what = Layout(case["shards"], 1), "refusal: " + case["name"]
    with Peers(ctx, lay.nranks, lay.rank) as peers:
        try:
            if case["shard"] is not None:
                peers.announce(lay, **case["shard"])
            else:
                a = banded(lay, rng_of("refusal", case["name"]), case["hb"])
                peers.announce(lay)
                wrong = dict(case["wrong"])
                wrong.setdefault("peer_need", case["hb"])
                peers.expect(*setup_exchanges(lay, **wrong)[:case["exchanges"]])
                ctx.spmm_setup_sharded(a[lay.rows()], lay.r0, lay.n_global)
            refused = None
        except capi.DlaError as e:
            refused = str(e)
        peers.check()
        assert refused == f"status {case['status']}: {case['text']}", (what, refused)
        good = Layout(FOLLOW_UP["shards"], FOLLOW_UP["rank"])
        res = product_on_shard(ctx, peers, good, FOLLOW_UP, True)
    check_halo_calls(ctx, good, FOLLOW_UP, res)
    assert D.same_bits(res["got"], res["ref"].astype(np.float64)), what + ": the product after the refusal is not exact"


# ------------------------------------------------------------------------------------------------------------------ Ritz slots
POSITIONS = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (8, 0), (8, 3), (8, 7)]
RITZ_N, RITZ_M, RITZ_L = [257, 1000, 999], [1, 13, 37, 48], 24


def ritz_options(m):
    """(n_res, skip): n_res = 0, 1, m with no, one or all roots skipped"""
    return [(0, "none"), (1, "none"), (1, "all"), (m, "none"), (m, "one"), (m, "all")]


RITZ_CASES = [dict(two=two, n=n, m=m, n_res=n_res, skip=skip) for two in (False, True) for n in RITZ_N for m in RITZ_M for n_res, skip in ritz_options(m)]
for _i, _c in enumerate(RITZ_CASES):
    _c["nranks"], _c["rank"] = POSITIONS[_i % len(POSITIONS)]


def peer_shards(n, nranks, rank):
    """this rank's n rows among peers of other heights"""
    return [n if r == rank else 100 + 7 * r for r in range(nranks)]


def check_ritz(ctx, case):
    """dla_ritz_residual / dla_ritz_residual2 as one rank of several.
    Before the hook: the sums are this rank's local sums of squares (check_norms' bound against the stored r), its maxima slot holds
    its local maxima (equal), every other rank's slot is +0.0.  After it: the rms norm is sqrt(what the hook left in buf[j]) / sqrt(n_global)
    bit for bit -- the entry point's own two operations on the engine's out[2 j] -- and the maximum is the maximum over all slots: a
    peer's larger maximum wins (odd roots), smaller ones lose (even roots)."""
    two, n, m, n_res, l = case["two"], case["n"], case["m"], case["n_res"], RITZ_L
    lay = Layout(peer_shards(n, case["nranks"], case["rank"]), case["rank"])
    what = f"{'ritz2' if two else 'ritz'} n={n} m={m} n_res={n_res} skip={case['skip']} as {lay}"
    rng = rng_of("ritz", *sorted(case.items()))
    v, av = np.asfortranarray(rng.standard_normal((n, l))), np.asfortranarray(rng.standard_normal((n, l)))
    y1, y2, eig = rng.standard_normal((l, m)), rng.standard_normal((l, m)), rng.standard_normal(m)
    if not two:
        y2 = y1
    sk = D.skip_pattern(m, case["skip"])
    _, _, r_ref, open_, m1, m2 = D.ref_ritz2(v, av, y1, y2, eig, n_res, sk)
    act = open_[:n_res]
    local_max = np.abs(r_ref).max(axis=0).astype(np.float64)
    # the peers: sums of the size of the local ones; maxima half the local one, and on odd roots one peer with twice it
    peer_sums = np.where(act, (lay.nranks - 1) * 0.75 * (r_ref ** 2).sum(axis=0).astype(np.float64)[:n_res], 0.0)
    odd, loud = np.arange(n_res) % 2 == 1, (lay.rank + 1) % lay.nranks
    peer_max = [np.where(act, local_max[:n_res] * np.where(odd & (r == loud), 2.0, 0.5), 0.0) for r in range(lay.nranks)]
    gv, gav = D.NanGuarded(ctx, n, l, v), D.NanGuarded(ctx, n, l, av)
    ge, gr = Guarded(ctx, n, m), Guarded(ctx, n, m)
    try:
        with Peers(ctx, lay.nranks, lay.rank) as peers:
            peers.announce(lay)
            first = len(peers.calls)
            peers.expect(*ritz_exchanges(ctx, lay, m, n_res, peer_sums, peer_max))
            if two:
                rn = ctx.ritz_residual2(D.view(gv), D.view(gav), y1, y2, eig, n_res, sk, D.view(ge), D.view(gr))
            else:
                rn = ctx.ritz_residual(D.view(gv), D.view(gav), y1, eig, n_res, sk, D.view(ge), D.view(gr), m=m)
            calls = peers.calls[first:]
            peers.check()
        r_got = D.written(gr.body(), what + " r")
        gv.assert_unchanged(); gav.assert_unchanged()
    finally:
        D.free(gv, gav, ge, gr)
    terms = {"b2": 64 * EPS * m2, "|eig| b1": np.where(open_, np.abs(eig), 0.0)[None, :] * 64 * EPS * m1, "4 eps |r|": 4 * EPS * np.abs(r_ref), "tiny": D.TINY}
    ratio = note("ritz r on a shard", assert_within(r_got, r_ref, terms, what + " r"))
    sums_b, max_b, others, sums_a, max_a = ritz_views(ctx, lay, m, n_res, calls)
    assert zero_bits(others), what + ": a maxima slot of another rank is not +0.0 before the sum"
    if n_res:
        local = np.zeros((2, n_res), order="F")
        local[0], local[1] = np.sqrt(sums_b / n), max_b
        D.check_norms(local, r_got, open_, n_res, what + ", this rank's part before the hook")
    got_local_max = np.abs(r_got).max(axis=0)
    for j in range(n_res):
        if not open_[j]:
            assert rn[0, j] == 0.0 and rn[1, j] == 0.0, (what, j, "the norms of a skipped root were touched")
            continue
        assert D.same_bits(rn[0:1, j], np.sqrt(sums_a[j:j + 1]) / np.sqrt(float(lay.n_global))), (what, j, rn[0, j], sums_a[j])
        assert D.same_bits(rn[1:2, j], max_a[j:j + 1]), (what, j, rn[1, j], max_a[j])
        want = max(got_local_max[j], max(peer_max[r][j] for r in range(lay.nranks) if r != lay.rank))
        assert rn[1, j] == want, (what, j, "larger peer maximum must win, smaller lose", rn[1, j], want)
        if lay.nranks > 1:
            assert (rn[1, j] > got_local_max[j]) == (j % 2 == 1), (what, j)
    return ratio


NRM2_CASES = [dict(n=n, m=m, nranks=nr, rank=rk) for (n, m), (nr, rk) in zip([(257, 1), (1000, 13), (999, 48), (1, 1), (4097, 3)], POSITIONS[1::2] + POSITIONS[:1])]


def check_nrm2(ctx, case):
    """dla_nrm2: one double.  Before the hook this rank's sum of squares (check_norms' bound), after it sqrt(what the hook left)"""
    n, m = case["n"], case["m"]
    lay = Layout(peer_shards(n, case["nranks"], case["rank"]), case["rank"])
    x = np.asfortranarray(rng_of("nrm2", n, m).standard_normal((n, m)))
    peer = 0.75 * float((x ** 2).sum()) + 1.0
    gx = D.NanGuarded(ctx, n, m, x)
    try:
        with Peers(ctx, lay.nranks, lay.rank) as peers:
            peers.announce(lay)
            first = len(peers.calls)
            peers.expect(nrm2_exchange(peer))
            got = ctx.nrm2(D.view(gx))
            (count, op, before, after), = peers.calls[first:] or [(0, 0, None, None)]
            peers.check()
        gx.assert_unchanged()
    finally:
        D.free(gx)
    want = (D.ld(x) ** 2).sum()
    assert abs(np.sqrt(LD(before[0])) - np.sqrt(want)) <= LD(1e-13) * np.sqrt(want), (case, before[0], float(want))
    assert D.same_bits(np.array([got]), np.sqrt(after)), (case, got, after)
    assert after[0] == before[0] + peer
    return 0.0


# ------------------------------------------------------------------------------------------------------------------ sample operators
SIGMA, TAU = 0.5, 0.05
KINDS = [("dla_synth_matvec", 0), ("dla_synth_apbmul", 1), ("dla_synth_ambmul", 2), ("dla_synth_spdmul", 3), ("dla_synth_smdmul", 4), ("dla_synth_metric", 5)]
SYNTH_N, SYNTH_M = [1, 2, 255, 256, 257, 999, 1000], [1, 7, 48, 64]
# row0 > 0 in every case: the middle of three, the last of two, the sixth of eight
SYNTH_LAYOUTS = [lambda n: ((300, n, 200), 1), lambda n: ((301, n), 1), lambda n: ((40, 33, 64, 65, 41, n, 37, 50), 5)]
SYNTH_CASES = [dict(n=n, layout=i % len(SYNTH_LAYOUTS)) for i, n in enumerate(SYNTH_N)]
_GLOBAL = {}


def synth_s(gi):
    """s(i) = 1 + 0.5 / (1 + (i mod 7)) in float64, the engine's own two operations (hip_engine.hip: synth_s): data of the reference"""
    return 1.0 + 0.5 / (1.0 + (gi % 7).astype(np.float64))


def synth_global(oracle, n_global):
    """W, the diagonal of A and s of the global sample problem (read only; kept per n_global)"""
    if n_global not in _GLOBAL:
        oracle.synth_setup(n_global, 0, n_global)
        gi = np.arange(1, n_global + 1)
        res = (oracle.synth_w(), oracle.synth_diag(), synth_s(gi), gi.astype(np.float64))
        for a in res:
            a.setflags(write=False)
        _GLOBAL[n_global] = res
    return _GLOBAL[n_global]


def synth_coupling(kind):
    """the 4 x 4 block C of y = d x + W C W^T x (hip_engine.hip: SynthKind)"""
    j = np.array([[0.0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1], [0, 0, -1, 0]])
    return {0: SIGMA * np.eye(4), 1: SIGMA * np.eye(4), 2: 0.2 * SIGMA * np.eye(4), 3: TAU * j, 4: -TAU * j, 5: 0.1 * np.eye(4)}[kind]


def synth_d(kind, gi, s):
    return {0: gi + 1.0, 1: gi + 5.0, 2: gi + 2.0}.get(kind, s)


def ulps(got, ref):
    """|got - ref| in units of the spacing of float64 at ref"""
    ref64 = ref.astype(np.float64)
    return np.abs(got.astype(LD) - ref) / np.spacing(np.abs(ref64)).astype(LD)


def rel_ulps(got, ref):
    """|got - ref| in units of eps |ref|, the unit of the suite's "4 eps |want|" for this kernel family (tests/test_operators_gpu.py):
    between one and two spacings"""
    return np.abs(got.astype(LD) - ref) / (EPS * np.abs(ref))


def synth_layout(case):
    shards, rank = SYNTH_LAYOUTS[case["layout"]](case["n"])
    return Layout(shards, rank)


def check_synth_products(ctx, oracle, case):
    """The six sample operators y = d x + W C W^T x on a shard with row0 > 0.  The only exchange is t = W^T x (4 x m): the player adds the
    peers' part, formed in long double from the global W and rounded once.

    The bound, per element: eps [2 |d x| + (n_global + 16) (|W| |C| |W|^T |x|)].
      t is a dot product over the n_global rows in some order of additions, partly on this rank, partly the peers' rounded partial:
      |fl(t) - t| <= (n_global + 2) eps |W|^T|x| (n_global - 1 additions and one rounding per product, one more for the peers' partial and one
      for the sum of the two parts).  C t and W (C t) are two contractions over 4 terms: 4 + 1 roundings each at most, and the sum
      s = W C t is added to d x with one more: (n_global + 2) + 5 + 5 + 1 = n_global + 13 <= n_global + 16 on |W||C||W|^T|x|.  d x is one product
      and takes part in that last addition: 2 eps |d x|.  d is exact for A, A + B, A - B (i + 1, i + 5, i + 2) and for the others the
      float64 s(i) the engine itself forms with the same two IEEE operations, so it is data here.  First order in eps."""
    lay, n = synth_layout(case), case["n"]
    wg, _, sg, gi = synth_global(oracle, lay.n_global)
    rows, others = lay.rows(), lay.others()
    ctx.synth_setup(lay.n_global, lay.r0, n)
    worst = 0.0
    for m in SYNTH_M:
        xg = np.asfortranarray(rng_of("synth", n, m).standard_normal((lay.n_global, m)))
        t_all = D.ld(wg).T @ D.ld(xg)
        t_peers = (D.ld(wg[others]).T @ D.ld(xg[others])).astype(np.float64)
        t_mag = np.abs(D.ld(wg)).T @ np.abs(D.ld(xg))
        gx = D.NanGuarded(ctx, n, m, xg[rows])
        try:
            for name, kind in KINDS:
                what = f"{name} n={n} m={m} as {lay}"
                cpl, d = D.ld(synth_coupling(kind)), D.ld(synth_d(kind, gi, sg)[rows])[:, None]
                ref = d * D.ld(xg[rows]) + D.ld(wg[rows]) @ (cpl @ t_all)
                mag = np.abs(D.ld(wg[rows])) @ (np.abs(cpl) @ t_mag)
                gy = Guarded(ctx, n, m)
                try:
                    with Peers(ctx, lay.nranks, lay.rank) as peers:
                        peers.expect(small_sum(t_peers))
                        call_matvec(ctx, name, n, m, gx.ptr, gy.ptr)
                        (_, _, before, _), = peers.calls or [(0, 0, None, None)]
                        peers.check()
                    got = D.written(gy.body(), what)
                finally:
                    D.free(gy)
                # what this rank sent is its own part of W^T x
                t_own = D.ld(wg[rows]).T @ D.ld(xg[rows])
                own_mag = np.abs(D.ld(wg[rows])).T @ np.abs(D.ld(xg[rows]))
                note("sample W^T x, this rank's part", assert_within(before.reshape(m, 4).T, t_own, {"(n + 2) eps |W|^T|x|": (n + 2) * EPS * own_mag, "tiny": D.TINY},
                                                                     what + " W^T x before the hook"))
                terms = {"2 eps |d x|": 2 * EPS * np.abs(d * D.ld(xg[rows])), "(n_global + 16) eps |W||C||W|^T|x|": (lay.n_global + 16) * EPS * mag, "tiny": D.TINY}
                worst = max(worst, note("sample products on a shard", assert_within(got, ref, terms, what)))
            gx.assert_unchanged()
        finally:
            D.free(gx)
    return worst


def ref_lrprec(variant, fac, aa, sg, xp, xm):
    """lrprec_1 / lrprec_2 in the operation order of synth_lrprec_kernel (den first); works in the dtype of its arguments"""
    fac = aa.dtype.type(fac)
    one = aa.dtype.type(1)
    if variant == 1:
        den = -one / (aa * aa - fac * fac * sg * sg)
        return den * (aa * xp + fac * sg * xm), den * (aa * xm + fac * sg * xp)
    den = one / (fac * fac * aa * aa - sg * sg)
    return den * (fac * aa * xp + sg * xm), den * (fac * aa * xm + sg * xp)


def lr_diagonals(w_rows, gi_rows):
    """the reference diagonals of A + B and A - B in float64: (i + 5) + sigma wsq and (i + 2) + 0.2 sigma wsq with wsq the sum of the
    squares of W's row in column order, the operations of synth_build_kernel and synth_lrprec_kernel.  Data of the reference, like the
    diagonal of A for the preconditioner"""
    wsq = np.zeros(w_rows.shape[0])
    for q in range(w_rows.shape[1]):
        wsq = wsq + w_rows[:, q] * w_rows[:, q]
    return (gi_rows + 5.0) + SIGMA * wsq, (gi_rows + 2.0) + 0.2 * SIGMA * wsq


def lrprec_operands(oracle, lay, m):
    """aa = ((A+B)_ii + (A-B)_ii) / 2 in long double on the reference diagonals, s(i), and two POSITIVE blocks: with fac > 0 neither
    numerator cancels, so an error in units of the result's spacing is a statement about the kernel and not about the data"""
    wg, _, sg, gi = synth_global(oracle, lay.n_global)
    rows = lay.rows()
    apb, amb = lr_diagonals(wg[rows], gi[rows])
    aa = LD(0.5) * (D.ld(apb) + D.ld(amb))
    rng = rng_of("lrprec", lay.n, m)
    xp, xm = np.asfortranarray(rng.uniform(0.5, 1.5, (lay.n, m))), np.asfortranarray(rng.uniform(0.5, 1.5, (lay.n, m)))
    return aa[:, None], D.ld(sg[rows])[:, None], xp, xm


LRPREC_FACS = [(1, 0.37), (2, 2.5)]


def check_synth_lrprec(ctx, oracle, case, apply=None):
    """dla_synth_lrprec1 / 2 on a shard: at most 4 ulp per element against the long-double expression in the device's operation order
    (den first) on the reference diagonals.  The ulp is eps |ref| here: nine roundings lie between the diagonals and a result (aa, aa^2,
    the difference, the reciprocal; a product, a sum; the last product -- aa counts twice in aa^2 and once more in the numerator), and
    the plain float64 evaluation of the kernel's own expression (emulate_lrprec, what the CPU file runs) is 4.7 spacings and 2.8 eps |ref|
    away from the long-double one on these inputs: 4 spacings is not a bound a correct kernel can meet, 4 eps |ref| is.
    apply(variant, fac, lay, xp, xm) -> (yp, ym) replaces the engine (the float64 emulation of the CPU file)"""
    lay, n = synth_layout(case), case["n"]
    if apply is None:
        ctx.synth_setup(lay.n_global, lay.r0, n)
    worst = 0.0
    for m in SYNTH_M:
        aa, sg, xp, xm = lrprec_operands(oracle, lay, m)
        for variant, fac in LRPREC_FACS:
            what = f"synth_lrprec{variant} n={n} m={m} as {lay}"
            if apply is not None:
                yp, ym = apply(variant, fac, lay, xp, xm)
            else:
                gp, gm, gyp, gym = D.NanGuarded(ctx, n, m, xp), D.NanGuarded(ctx, n, m, xm), Guarded(ctx, n, m), Guarded(ctx, n, m)
                try:
                    with Peers(ctx, lay.nranks, lay.rank) as peers:
                        ctx._chk(ctx.lib.dla_call_lrprec(ctx.h, capi.fn_address(f"dla_synth_lrprec{variant}"), n, m, fac, gp.ptr, gm.ptr, gyp.ptr, gym.ptr))
                        peers.check()                        # (elementwise: no exchange)
                    yp, ym = D.written(gyp.body(), what), D.written(gym.body(), what)
                    gp.assert_unchanged(); gm.assert_unchanged()
                finally:
                    D.free(gp, gm, gyp, gym)
            rp, rm = ref_lrprec(variant, fac, aa, sg, D.ld(xp), D.ld(xm))
            u = max(float(rel_ulps(yp, rp).max()), float(rel_ulps(ym, rm).max()))
            worst = max(worst, note("sample lrprec on a shard (ulp / 4)", u / 4))
            assert u <= 4, (what, u)
    return worst


def emulate_lrprec(oracle):
    """synth_lrprec_kernel in float64 numpy, operation by operation (no fused multiply-add)"""
    def apply(variant, fac, lay, xp, xm):
        wg, _, sg, gi = synth_global(oracle, lay.n_global)
        rows = lay.rows()
        apb, amb = lr_diagonals(wg[rows], gi[rows])
        aa = 0.5 * (apb + amb)
        return ref_lrprec(variant, fac, aa[:, None], sg[rows][:, None], xp, xm)
    return apply


def booked_precnd(ctx):
    return {k: v["launches"] for k, v in ctx.kernel_stats().items() if v["launches"] and k.startswith("synth_precnd_kernel")}


def check_synth_precnd(ctx, oracle, case):
    """dla_synth_precnd on a shard with row0 > 0: x / (diag + fac) on the reference diagonal, at most 4 ulp per element; fac = -diag_ref[i]
    passes row i through bit for bit while its neighbours are divided; fac = -diag_ref[i] + 2e-5 divides row i, whose bound is the
    conditioned one |x| (4 eps |diag| + 2 eps |den|) / den^2: the device's diagonal may differ from the reference's by its roundings
    (4 eps |diag| covers the four additions of its sum of squares and the two of the diagonal), den is one rounded addition and the
    quotient one rounded division."""
    lay, n = synth_layout(case), case["n"]
    _, diag_g, _, _ = synth_global(oracle, lay.n_global)
    diag = diag_g[lay.rows()]
    ctx.synth_setup(lay.n_global, lay.r0, n)
    worst = 0.0
    i = n // 2
    for m in SYNTH_M:
        x = np.asfortranarray(rng_of("precnd", n, m).standard_normal((n, m)))
        gx = D.NanGuarded(ctx, n, m, x)
        try:
            for which, fac in [("plain", 0.37), ("guard", -diag[i]), ("beside the guard", -diag[i] + 2e-5)]:
                what = f"synth_precnd {which} n={n} m={m} as {lay}"
                gp = Guarded(ctx, n, m)
                try:
                    with Peers(ctx, lay.nranks, lay.rank) as peers:
                        call_precnd(ctx, "dla_synth_precnd", n, m, fac, gx.ptr, gp.ptr)
                        peers.check()                        # (elementwise: no exchange)
                    got = D.written(gp.body(), what)
                finally:
                    D.free(gp)
                den = D.ld(diag) + LD(fac)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ref = D.ld(x) / den[:, None]
                keep = np.ones(n, bool)
                if which != "plain":
                    keep[i] = False
                    if which == "guard":
                        assert D.same_bits(got[i], x[i]), what + ": the row inside the guard must pass through bit for bit"
                    else:
                        bound = np.abs(D.ld(x[i])) * (4 * EPS * abs(LD(diag[i])) + 2 * EPS * abs(den[i])) / den[i] ** 2
                        err = np.abs(D.ld(got[i]) - ref[i])
                        assert np.all(err <= bound), (what, float((err / bound).max()))
                        worst = max(worst, note("sample precnd beside the guard", float((err / bound).max())))
                    for k in (i - 1, i + 1):
                        if 0 <= k < n:
                            assert abs(diag[k] + fac) > 1e-3 and not np.array_equal(got[k], x[k]), (what, "the neighbours of the guarded row are divided", k)
                if keep.any():
                    u = float(ulps(got[keep], ref[keep]).max())
                    worst = max(worst, note("sample precnd on a shard (ulp / 4)", u / 4))
                    assert u <= 4, (what, u)
            gx.assert_unchanged()
        finally:
            D.free(gx)
    return worst


# ------------------------------------------------------------------------------------------------------------------ the host engine's run
FAMILIES = {
    "product exact": lambda ctx, oracle: [check_product(ctx, c, True) for c in PRODUCT_CASES],
    "product random": lambda ctx, oracle: [check_product(ctx, c, False) for c in PRODUCT_CASES],
    "refusals": lambda ctx, oracle: [check_refusal(ctx, c) for c in REFUSALS],
    "ritz": lambda ctx, oracle: [check_ritz(ctx, c) for c in RITZ_CASES],
    "nrm2": lambda ctx, oracle: [check_nrm2(ctx, c) for c in NRM2_CASES],
    "sample products": lambda ctx, oracle: [check_synth_products(ctx, oracle, c) for c in SYNTH_CASES],
    "sample precnd": lambda ctx, oracle: [check_synth_precnd(ctx, oracle, c) for c in SYNTH_CASES],
    "sample lrprec (float64 emulation)": lambda ctx, oracle: [check_synth_lrprec(ctx, oracle, c, apply=emulate_lrprec(oracle)) for c in SYNTH_CASES],
}


def main(out_path):
    """every shared case list on the host-memory engine; one record per family: the cases run, the failure if any, and WORST"""
    import traceback

    import hostsim
    from oracle.pyoracle import Oracle
    capi.load(hostsim.build())
    ctx = capi.Context()
    assert ctx.backend.startswith("hostsim"), ctx.backend
    ctx.set_option(capi.OPT_CALLBACKS_ON_DEVICE, 1)
    oracle = Oracle()
    report = {}
    for family, run in FAMILIES.items():
        try:
            report[family] = dict(cases=len(run(ctx, oracle)), failure=None)
        except Exception:        # noqa: BLE001
            report[family] = dict(cases=0, failure=traceback.format_exc()[-4000:])
        assert ctx.comm_info() == (1, 0)
    report["worst"] = dict(WORST)
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
