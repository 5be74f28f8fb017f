"""The MSM input designer (msm_shapes.py) held to its purpose, on the CPU:
its constants are the kernels', its window table is the library's, every
profile the GPU tests run (test_gpu_msm_shapes.py) lands where it is meant to
in k_msm_accumulate's lane partition, and its digit rows are the recoding
reference's."""
import re
from pathlib import Path

import pytest

import fe10_model as m
import msm_shapes as ms
from oracle import ristretto as r255
from oracle.merlin import Rng

CSRC = Path(__file__).resolve().parent.parent / "bulletproof-perm_amd" / "csrc"
GPU_KS = (4, 12)  # the BPP_MSM_ACC_K values test_gpu_msm_shapes.py sets
# single-MSM sizes of test_gpu_msm_shapes.py with the width the engine picks
GPU_SIZES = {427: 7, 2855: 9, 14485: 11, 16383: 11, 16384: 11, 16385: 11, 26330: 11, 26331: 12, 4096 * 7 + 1: 12,
             47393: 12, 47394: 13, 65535: 13, 65536: 13, 262144: 15}


def _define(name: str) -> int:
    text = (CSRC / "msm_kernels.cuh").read_text()
    hits = re.findall(rf"^#define {name} (\d+)\b", text, flags=re.M)
    assert len(hits) == 1, (name, hits)
    return int(hits[0])


def test_partition_constants_are_the_kernels():
    assert _define("ACC_T") == ms.LANES_PER_WG
    assert _define("FIX_MAX") == ms.HEAVY_LANES
    assert _define("RS_FINE_BITS") == 7 and _define("RS_CHUNK") == 4096


def _cost_choose_c(n: int) -> int:
    """msm_choose_c's cost model, restated."""
    best, bestc = 4, float("inf")
    for c in range(2, 17):
        W = (254 + c - 1) // c
        cost = W * (7.0 * n + 9.0 * (1 << c)) + 8.0 * c * (W - 1)
        if cost < bestc:
            best, bestc = c, cost
    return best


def test_window_table_is_the_librarys():
    """The table, the cost model it comes from and bpp_msm_windows agree at
    every size the GPU tests use and on both sides of every threshold
    (loads the library; opens no GPU)."""
    import bpperm
    sizes = set(GPU_SIZES) | {p.n for K in GPU_KS for p in ms.profile_set(K)} | {64, 300, 1 << 17, 1 << 20}
    for first, _ in ms.CHOOSE_C:
        sizes |= {max(1, first - 1), first}
    for n in sorted(sizes):
        c, W = bpperm.msm_windows(n)
        assert c == ms.choose_c(n) == _cost_choose_c(n), n
        assert W == m.windows(c)
        if n in GPU_SIZES:
            assert c == GPU_SIZES[n], n
    assert 14 not in {c for _, c in ms.CHOOSE_C}


def test_front_end_by_size():
    fe = {n: ms.front_end(n) for n in GPU_SIZES}
    assert [n for n in sorted(fe) if fe[n] == "atomic"] == [427, 2855, 14485, 16383]
    assert [n for n in sorted(fe) if fe[n] == "lds"] == [16384, 16385, 26330]
    assert all(ms.front_end(n, lds_env=True) == "lds" for n in GPU_SIZES if n >= 16384)


def test_top_window_fine_bits_table():
    """msm_geom's tfb rule restated: the top window's bits less log2 of the
    coarse bins, floored at 0, when the top window is narrow."""
    assert _define("RS_FINE_BITS") == ms.RS_FINE_BITS
    for c, want in ms.TFB.items():
        top, lognc = 253 - c * (m.windows(c) - 1), c - 1 - ms.RS_FINE_BITS
        assert top < c - 1 and max(top - lognc, 0) == want == ms.top_fine_bits(c), c
    assert all(ms.top_fine_bits(c) == ms.RS_FINE_BITS for c in range(2, 8))  # fewer than 2^7 buckets


@pytest.mark.parametrize("K", GPU_KS)
def test_profile_set_covers_every_case(K):
    """Across the profile set of K: all five classes, every designed
    placement, a run of >= 3 empty buckets between occupied ones, a last lane
    that is not full.  Each profile alone misses something the set needs, so
    dropping one fails here."""
    profiles = ms.profile_set(K)
    need = ms.required_features(K)
    feats = [ms.features(p) for p in profiles]
    missing = need - set().union(*feats)
    assert not missing, sorted(missing)
    for i, p in enumerate(profiles):
        rest = set().union(*(f for j, f in enumerate(feats) if j != i))
        assert need - rest, f"{p.name} adds nothing to the set"
    for p in profiles:
        assert ms.front_end(p.n) == "atomic" and ms.choose_c(p.n) == p.c
    if K == 4:
        assert [p.c for p in profiles] == [8, 9] and all(1500 <= p.n <= 4000 for p in profiles)


def test_profile_scalars_are_what_was_designed():
    for K in GPU_KS:
        for p in ms.profile_set(K):
            sc = ms.profile_scalars(p)
            assert len(sc) == p.n == sum(p.sizes.values()) and all(0 <= s < r255.L for s in sc)
            got = ms.bucket_sizes(p.c, sc)[p.window]
            assert {b: k for b, k in enumerate(got) if k} == p.sizes
            assert sorted(ms.spread(sc)) == sorted(sc)


@pytest.mark.parametrize("n", [16384, 26331])
def test_mixed_and_special_scalars(n):
    c = ms.choose_c(n)
    p, sc = ms.mixed_scalars(n)
    assert len(sc) == n and p.c == c and p.n == n // 4 and all(0 <= s < r255.L for s in sc)
    got = ms.bucket_sizes(c, sc, 1, 2)[0]
    assert all(got[b] >= k for b, k in p.sizes.items())
    few = ms.few_value_scalars(n)
    assert len(few) == n and len(set(few)) == 8
    assert all(sum(1 for k in row if k) <= 8 for row in ms.bucket_sizes(c, sorted(set(few))))
    top = ms.top_bit_scalars(n)
    assert len(top) == n and all(1 << 252 <= s < r255.L for s in top)
    assert ms.bucket_sizes(c, top[:64], m.windows(c) - 1)[0][0] == 64


@pytest.mark.parametrize("c", [8, 11, 12, 13, 15, 16])
def test_scalars_from_digits_round_trip(c):
    fams = m.digit_scalars(c, Rng(c, b"test-scalars"), nrand=16)
    rows = [m.ref_digits(s, c) for s in fams]
    assert ms.scalars_from_digits(c, rows) == fams


def test_scalars_from_digits_rejects_what_is_no_recoding():
    c, Wn = 8, m.windows(8)
    row = [0] * Wn
    row[3] = 128  # 2^(c-1) below the top window recodes as -128 with a carry
    with pytest.raises(ValueError):
        ms.scalars_from_digits(c, [row])
    row[3], row[4] = -128, 1
    assert ms.scalars_from_digits(c, [row]) == [128 << 24]
    row = [0] * Wn
    row[0] = -1  # negative
    with pytest.raises(ValueError):
        ms.scalars_from_digits(c, [row])
    row = [0] * Wn
    row[Wn - 1] = 1 << (253 - c * (Wn - 1))  # 2^253 >= l
    with pytest.raises(ValueError):
        ms.scalars_from_digits(c, [row])
    with pytest.raises(ValueError):
        ms.scalars_from_digits(c, [[0] * (Wn - 1)])


def test_occupancy_signs_top_bucket_and_top_window():
    c, Wn = 9, m.windows(9)
    B = 1 << (c - 1)
    sc = ms.occupancy(c, 2, {0: 3, 5: 4, B - 1: 2}, {0: "-", 5: "+-", B - 1: "-"})
    rows = [m.ref_digits(s, c) for s in sc]
    assert [r[2] for r in rows] == [-1, -1, -1, 6, -6, 6, -6, -B, -B]
    assert [r[3] for r in rows] == [1, 1, 1, 0, 1, 0, 1, 1, 1]
    with pytest.raises(ValueError):  # +2^(c-1) exists only in the top window
        ms.occupancy(c, 2, {B - 1: 1})
    with pytest.raises(ValueError):  # no borrow above the top window
        ms.occupancy(c, Wn - 1, {0: 1}, {0: "-"})
    assert ms.occupancy(c, Wn - 1, {0: 2}) == [1 << (c * (Wn - 1))] * 2


def test_classify_small_cases():
    K = 4
    wg = ms.LANES_PER_WG * K
    part = ms.classify([[4, 0, 0, 0, 5, 28, 1, 33], [0] * 8, [wg - 71 - 36, 34, 8, 0, 1]], K)
    assert [b.cls for b in part.buckets] == [
        "in_lane", "in_workgroup", "in_workgroup", "in_lane", "heavy_mid_lane",
        "heavy_mid_lane", "heavy_at_lane_start", "crosses_workgroup", "in_lane"]
    assert part.buckets[5].start == 71 and part.buckets[6].start == wg - 36 and part.buckets[7].start == wg - 2
    assert part.empty_runs == [3, 1] and part.entries == wg + 7 and part.last_lane_entries == 3
    # 8 lanes past the first is heavy, 7 is not; from a lane's first entry
    assert ms.classify([[7 * K + 1]], K).buckets[0].cls == "in_workgroup"
    assert ms.classify([[8 * K + 1]], K).buckets[0].cls == "heavy_at_lane_start"
    assert ms.classify([[1, 8 * K]], K).buckets[1].cls == "heavy_mid_lane"
    assert ms.classify([[1, 7 * K]], K).buckets[1].cls == "in_workgroup"


def test_degenerate_tables():
    tabs = ms.degenerate_points()
    assert set(tabs) == {"mixed", "same", "pairs", "identity4"}
    ident = r255.encode(r255.IDENTITY)
    assert ident == bytes(32)
    for name, (enc, pts) in tabs.items():
        assert len(enc) == len(pts) == ms.DEGENERATE_N and all(len(e) == 32 for e in enc)
    enc, pts = tabs["mixed"]
    assert enc[0] == ident and enc[1] == r255.encode(r255.BASEPOINT) and enc.count(enc[2]) >= 60
    assert sum(1 for a, b in zip(pts, pts[1:]) if r255.equal(r255.ed_add(a, b), r255.IDENTITY) and a != b) >= 60
    assert len(set(tabs["same"][0])) == 1
    enc, pts = tabs["pairs"]
    assert all(r255.encode(r255.ed_add(pts[i], pts[i + 1])) == ident and enc[i] != enc[i + 1]
               for i in range(0, ms.DEGENERATE_N, 50))
    assert all(e == ident for e in tabs["identity4"][0][3::4])
