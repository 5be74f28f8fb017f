"""The single-MSM bucket reduction (k_msm_reduce_lanes + k_msm_reduce_fold,
the host Horner over their terms) bit-exact at the 32-byte encoding against
oracle.cport.msm, on both of its shapes: the lone MSM (ctx.msm_table,
msm_table_dev_partial: 2^RWAVE_LOG_LONE buckets a lane) and the stream
(ctx.msm_submit / msm_collect: 2^RWAVE_LOG).

  size    c   B      lanes per window (lone / stream)
  16384   11  1024   128 / 64: fold blocks narrower than RFOLD_T, no upper-bit blocks
  26331   12  2048   256 / 128
  47394   13  4096   512 / 256: exactly one full fold block in either shape
  262144  15  16384  2048 / 1024: four lane sums per fold lane, two upper-bit blocks
"""
import hashlib
from collections import namedtuple

import pytest

import fe10_model as m
import msm_shapes as ms
from oracle import cport, ristretto as r255

pytestmark = pytest.mark.gpu
L = r255.L
NMAX = 1 << 18
SIZES = [(16384, 11), (26331, 12), (47394, 13), (262144, 15)]

Table = namedtuple("Table", "gpu points")


def _sb(sc):
    return b"".join(s.to_bytes(32, "little") for s in sc)


@pytest.fixture(scope="module")
def table(ctx):
    raw = hashlib.shake_256(b"msm-reduce-points").digest(64 * NMAX)
    t = ctx.from_uniform(raw)
    yield Table(t, cport.from_uniform_threads(raw))
    t.close()


@pytest.fixture(scope="module")
def random_scalars():
    raw = hashlib.shake_256(b"msm-reduce-scalars").digest(40 * NMAX)
    return [int.from_bytes(raw[40 * i: 40 * i + 40], "little") % L for i in range(NMAX)]


def _want(table, sb):
    n = len(sb) // 32
    ref = cport.msm if n <= 1 << 16 else cport.msm_threads
    return ref(sb, table.points[: 32 * n])


class Dev:
    """Scalars on the device for the submit / partial entry points."""

    def __init__(self, ctx, sb):
        self.ctx, self.n = ctx, len(sb) // 32
        self.d = ctx.dev_alloc(len(sb))
        ctx.htod(self.d, sb)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.dev_free(self.d)


def _both_paths(ctx, table, sc):
    """The lone MSM and one MSM through a stream slot == the C port's."""
    sb = _sb(sc)
    want = _want(table, sb)
    assert ctx.msm_table(sb, table.gpu, len(sc)) == want
    with Dev(ctx, sb) as d:
        assert ctx.msm_collect(ctx.msm_submit(d.d, table.gpu, d.n)) == want


@pytest.mark.parametrize("n,c", SIZES)
def test_random_scalars(ctx, table, random_scalars, n, c):
    import bpperm
    assert bpperm.msm_windows(n) == (c, m.windows(c))
    _both_paths(ctx, table, random_scalars[:n])


@pytest.mark.parametrize("n,c", [(26331, 12), (47394, 13)])
def test_every_window_alone_and_top_split(ctx, table, random_scalars, n, c):
    """One launch per window and the split [0, W - 1) + [W - 1, W), through
    the lone partial entry point and through the stream's: the launch of the
    narrow top window alone leaves most lanes empty."""
    import bpperm
    W = m.windows(c)
    assert bpperm.msm_windows(n) == (c, W)
    sb = _sb(random_scalars[NMAX - n:])
    want = _want(table, sb)
    with Dev(ctx, sb) as d:
        lone = [ctx.msm_table_dev_partial(d.d, table.gpu, n, w, w + 1) for w in range(W)]
        assert bpperm.partials_finish(lone) == want
        stream = [ctx.msm_collect(ctx.msm_submit(d.d, table.gpu, n, w, w + 1), partial=True) for w in range(W)]
        assert bpperm.partials_finish(stream) == want
        two = [ctx.msm_table_dev_partial(d.d, table.gpu, n, 0, W - 1),
               ctx.msm_table_dev_partial(d.d, table.gpu, n, W - 1, W)]
        assert bpperm.partials_finish(two) == want
        t0, t1 = ctx.msm_submit(d.d, table.gpu, n, 0, W - 1), ctx.msm_submit(d.d, table.gpu, n, W - 1, W)
        assert bpperm.partials_finish([ctx.msm_collect(t0, partial=True), ctx.msm_collect(t1, partial=True)]) == want


@pytest.mark.parametrize("n", [16384, 26331])
def test_all_scalars_equal(ctx, table, random_scalars, n):
    """One heavy bucket per window: every lane but one stores the identity."""
    _both_paths(ctx, table, [random_scalars[7]] * n)


@pytest.mark.parametrize("case", ["plus", "plus_minus"])
def test_scalars_one_and_minus_one(ctx, table, case):
    """s = 1: bucket 0 of window 0 alone, every other window empty; with
    s = l - 1 on the odd terms, whose digits fill the upper windows too."""
    n = 16384
    sc = [1] * n if case == "plus" else [1 if i % 2 == 0 else L - 1 for i in range(n)]
    _both_paths(ctx, table, sc)


@pytest.mark.parametrize("n", [16384, 26331])
def test_designed_buckets_across_workgroup_borders(ctx, table, n, monkeypatch):
    """msm_shapes.mixed_scalars at BPP_MSM_ACC_K = 4: every fourth term
    follows the borders profile in window 1 (buckets over lane and workgroup
    borders, heavy ones among them), so bucket_total's head / tail assembly
    feeds the lane sums."""
    monkeypatch.setenv("BPP_MSM_ACC_K", "4")
    _, sc = ms.mixed_scalars(n)
    _both_paths(ctx, table, sc)


def test_two_slots_back_to_back(ctx, table, random_scalars):
    """Two different scalar vectors in flight on two slots == each alone."""
    n = 26331
    a, b = _sb(random_scalars[:n]), _sb(random_scalars[n: 2 * n])
    with Dev(ctx, a) as da, Dev(ctx, b) as db:
        alone = [ctx.msm_collect(ctx.msm_submit(d.d, table.gpu, n)) for d in (da, db)]
        ta = ctx.msm_submit(da.d, table.gpu, n)
        tb = ctx.msm_submit(db.d, table.gpu, n)
        assert [ctx.msm_collect(ta), ctx.msm_collect(tb)] == alone
    assert alone == [_want(table, a), _want(table, b)]
