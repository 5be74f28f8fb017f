"""The MSM bucket engine on designed bucket shapes, every window width and
every sort front end, bit-exact at the 32-byte encoding.

The reference is oracle.cport.msm (the serial C restatement) over points from
cport.from_uniform, and oracle.ristretto.msm for the small degenerate tables;
no result is compared with another GPU result.  msm_shapes.py designs the
inputs and test_msm_shapes.py shows, on the CPU, where each lands in
k_msm_accumulate's lane partition.

  size    c   front end               tfb (radix: top window's fine bits)
  427     7   atomic
  2855    9   atomic
  14485   11  atomic (below 16384)
  16384   11  LDS
  26331   12  radix                   0
  47394   13  radix                   1
  262144  15  radix                   6
  (2^20   16  radix                   5: test_gpu_msm_large.py)
"""
import hashlib
from collections import namedtuple
from contextlib import contextmanager

import pytest

import fe10_model as m
import msm_shapes as ms
from oracle import cport, ristretto as r255
from oracle.merlin import Rng

pytestmark = pytest.mark.gpu
L = r255.L
NMAX = 1 << 18

Table = namedtuple("Table", "gpu points")


def _sb(sc):
    return b"".join(s.to_bytes(32, "little") for s in sc)


@pytest.fixture(scope="module")
def table(ctx):
    """2^18 points: the GPU's table and the C port's encodings of the same
    uniform bytes (every test uses a prefix)."""
    raw = hashlib.shake_256(b"msm-shapes-points").digest(64 * NMAX)
    t = ctx.from_uniform(raw)
    yield Table(t, cport.from_uniform_threads(raw))
    t.close()


@pytest.fixture(scope="module")
def random_scalars():
    raw = hashlib.shake_256(b"msm-shapes-scalars").digest(40 * NMAX)
    return [int.from_bytes(raw[40 * i: 40 * i + 40], "little") % L for i in range(NMAX)]


@contextmanager
def profiled(ctx):
    """Stage launch counts of what runs inside; -> a function naming the sort
    front end that ran."""
    ctx.profile(True)
    ctx.profile_reset()

    def ran():
        digits, count = ctx.profile_get("msm_digits")[1], ctx.profile_get("msm_count")[1]
        return {(False, True): "atomic", (True, True): "lds", (True, False): "radix"}.get((digits > 0, count > 0))
    try:
        yield ran
    finally:
        ctx.profile(False)
        ctx.profile_reset()


def _check(ctx, table, sc, front=None):
    """One MSM over the table's first len(sc) points == the C port's, and
    (front given) the front end that ran."""
    n = len(sc)
    sb = _sb(sc)
    with profiled(ctx) as ran:
        got = ctx.msm_table(sb, table.gpu, n)
        front_ran = ran()
    # (above 2^16 terms the C port runs on chunks of the terms in parallel,
    # their results added by the Python oracle: seconds less, as exact)
    ref = cport.msm if n <= 1 << 16 else cport.msm_threads
    assert got == ref(sb, table.points[: 32 * n])
    if front:
        assert front_ran == front


# ---------------------------------------------------------------- front end by size
FRONT_ENDS = [(427, 7, "atomic"), (2855, 9, "atomic"), (14485, 11, "atomic"),
              (16383, 11, "atomic"), (16384, 11, "lds"), (16385, 11, "lds"),
              (26330, 11, "lds"), (26331, 12, "radix"),
              (4096 * 7 + 1, 12, "radix"),  # one term in the last RS_CHUNK
              (47393, 12, "radix"), (47394, 13, "radix"),  # the c = 12 / 13 threshold
              (65535, 13, "radix"), (65536, 13, "radix"),
              (262144, 15, "radix")]


@pytest.mark.parametrize("n,c,front", FRONT_ENDS)
def test_front_end_by_size(ctx, table, random_scalars, n, c, front):
    import bpperm
    assert bpperm.msm_windows(n) == (c, m.windows(c))
    _check(ctx, table, random_scalars[:n], front)


def test_top_window_fine_bits():
    """msm_geom's tfb for every width (through the arithmetic probe, which
    builds its MsmGeom where msm.hip does): 0, 1, 6 and 5 at c = 12, 13, 15
    and 16.  A wider value still sorts correctly but packs the top window into
    a few coarse bins, which only a timing shows."""
    for c in range(2, 17):
        g = m.probe().geom(c)
        assert g["tfb"] == ms.top_fine_bits(c), c
        assert g["tfb"] == ms.TFB.get(c, g["tfb"])


# ---------------------------------------------------------------- every window alone
@pytest.mark.parametrize("n,c", [(26331, 12), (65536, 13)])
def test_every_window_alone(ctx, table, random_scalars, n, c):
    """One launch per window (nseg = 1, the lone-MSM reduction shape, and a
    launch that holds only the narrow top window), and the split
    [0, W - 1) + [W - 1, W)."""
    import bpperm
    W = m.windows(c)
    assert bpperm.msm_windows(n) == (c, W)
    sb = _sb(random_scalars[NMAX - n:])
    want = cport.msm(sb, table.points[: 32 * n])
    d = ctx.dev_alloc(32 * n)
    try:
        ctx.htod(d, sb)
        parts = [ctx.msm_table_dev_partial(d, table.gpu, n, w, w + 1) for w in range(W)]
        assert bpperm.partials_finish(parts) == want
        two = [ctx.msm_table_dev_partial(d, table.gpu, n, 0, W - 1), ctx.msm_table_dev_partial(d, table.gpu, n, W - 1, W)]
        assert bpperm.partials_finish(two) == want
    finally:
        ctx.dev_free(d)


# ---------------------------------------------------------------- adversarial digits
@pytest.mark.parametrize("lds", [False, True])
@pytest.mark.parametrize("n,c", [(16384, 11), (26331, 12)])
def test_adversarial_digits_on_sort_paths(ctx, table, n, c, lds, monkeypatch):
    """Every window at the recoding threshold, carries arriving exactly at it,
    l - 1, 2^252 ... (fe10_model.digit_scalars) through k_msm_digits and the
    radix sort's closed-form recoding, at full size."""
    if lds:
        monkeypatch.setenv("BPP_MSM_LDS_SORT", "1")
    assert ms.choose_c(n) == c
    _check(ctx, table, ms.adversarial_digit_scalars(c, n, 50 + n), ms.front_end(n, lds))


# ---------------------------------------------------------------- designed occupancy
@pytest.mark.parametrize("which", [0, 1], ids=["spans", "borders"])
@pytest.mark.parametrize("K", [4, 12])
def test_designed_occupancy(ctx, table, K, which, monkeypatch):
    """msm_shapes.profile_set(K) at BPP_MSM_ACC_K = K: buckets of 1, K - 1,
    K, K + 1 and 2K entries, buckets touching 7..10 lanes from a lane's
    first, second and last entry, light and heavy buckets over a workgroup
    border, bucket 0 and the top bucket, both signs in one bucket, runs of
    empty buckets, a last lane that is not full."""
    import bpperm
    monkeypatch.setenv("BPP_MSM_ACC_K", str(K))
    p = ms.profile_set(K)[which]
    assert bpperm.msm_windows(p.n)[0] == p.c
    _check(ctx, table, ms.spread(ms.profile_scalars(p)), "atomic")


@pytest.mark.parametrize("n", [16384, 26331])
def test_designed_quarter_among_random(ctx, table, n, monkeypatch):
    """Each sort path: every fourth term follows the borders profile in
    window 1, the rest are random; K = 4."""
    monkeypatch.setenv("BPP_MSM_ACC_K", "4")
    _, sc = ms.mixed_scalars(n)
    _check(ctx, table, sc, ms.front_end(n))


def test_eight_distinct_scalars(ctx, table):
    """n = 26331 scalars drawn from 8 values: 8 heavy buckets in every window."""
    n = 26331
    _check(ctx, table, ms.few_value_scalars(n), "radix")


@pytest.mark.parametrize("lds", [False, True])
def test_every_scalar_with_bit_252(ctx, table, lds, monkeypatch):
    """c = 12: the top window is one bit (tfb = 0, one fine slot; k_rsort_fine
    fills boff from bucket NC up); here all n terms sit in its bucket 0."""
    if lds:
        monkeypatch.setenv("BPP_MSM_LDS_SORT", "1")
    n = 26331
    assert ms.TFB[ms.choose_c(n)] == 0
    _check(ctx, table, ms.top_bit_scalars(n), ms.front_end(n, lds))


# ---------------------------------------------------------------- degenerate tables
@pytest.fixture(scope="module")
def degenerate(ctx):
    """msm_shapes.degenerate_points() tiled to the largest size, on the GPU
    (ctx.decompress) and as the C port's point bytes (the same encodings)."""
    nmax = 26331
    out = {}
    for name, (enc, pts) in ms.degenerate_points().items():
        tiled = [enc[i % len(enc)] for i in range(nmax)]
        out[name] = (ctx.decompress(tiled), b"".join(tiled), pts)
    yield out
    for t, _, _ in out.values():
        t.close()


def _degenerate_scalars(case, n):
    rng = Rng(1000 + n, b"msm-shapes-degenerate")
    if case == "equal_scalars":
        return [rng.scalar()] * n
    sc = [rng.scalar() for _ in range(n)]
    if case == "pairs":  # P and -P with the same scalar; a term left over gets 0
        sc = [sc[i // 2] for i in range(n)]
        if n % 2:
            sc[-1] = 0
    return sc


DEGENERATE_CASES = {"mixed": "mixed", "same": "same", "pairs": "pairs", "identity4": "identity4",
                    "equal_scalars": "same"}


@pytest.mark.parametrize("n", [64, 300, 16384, 26331])
@pytest.mark.parametrize("case", list(DEGENERATE_CASES))
def test_degenerate_tables(ctx, degenerate, case, n):
    """Tables with the identity, one point many times and P beside -P: the
    mixed additions, ge_add in the fold and fixup and the reduction's running
    sums meet doublings and cancellations.  n <= 300 against the Python
    oracle, the tiled sizes against the C port over the same encodings."""
    tbl, enc, pts = degenerate[DEGENERATE_CASES[case]]
    sc = _degenerate_scalars(case, n)
    got = ctx.msm_table(_sb(sc), tbl, n)
    if n <= ms.DEGENERATE_N:
        want = r255.encode(r255.msm(sc, pts[:n]))
    else:
        want = cport.msm(_sb(sc), enc[: 32 * n])
    assert got == want
    if case in ("same", "equal_scalars"):  # (sum s_i mod l) P
        assert got == r255.encode(r255.ed_mul(sum(sc) % L, pts[0]))
    if case == "pairs":
        assert got == bytes(32)


# ---------------------------------------------------------------- bpp_msm_batch with skew
def test_msm_batch_skewed_sizes(ctx):
    """M = 10 MSMs (k_msm_horner) of very unequal sizes over a 40-point table
    that includes the identity: c follows the average term count, so MSM 0's
    3000 terms over 40 points make heavy buckets; empty MSMs between."""
    import bpperm
    sizes = [3000, 0, 1, 1, 0, 17, 2, 1, 1, 1]
    rng = Rng(40, b"msm-shapes-batch")
    pts = [r255.IDENTITY if k in (0, 13) else rng.point() for k in range(40)]
    enc = [r255.encode(p) for p in pts]
    tbl = ctx.decompress(enc)
    offs, idx, scal = [0], [], []
    for k, size in enumerate(sizes):
        for j in range(size):
            idx.append((7 * j + k) % 40)
            scal.append(rng.scalar())
        offs.append(len(idx))
    assert bpperm.msm_windows(offs[-1] // len(sizes))[0] == 6
    got = ctx.msm_batch(offs, _sb(scal), idx, tbl)
    tbl.close()
    for k, size in enumerate(sizes):
        a, b = offs[k], offs[k + 1]
        if size > 64:
            want = cport.msm(_sb(scal[a:b]), b"".join(enc[i] for i in idx[a:b]))
        else:
            want = r255.encode(r255.msm(scal[a:b], [pts[i] for i in idx[a:b]]))
        assert got[k] == want, k
