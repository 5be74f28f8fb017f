"""The four implementations of the signed-window recoding (for_each_digit,
k_msm_digits, the closed form of k_rsort_digits_count, DtLane::row_of) and
the two constructions of its offset K, through the arithmetic probe, against
the reference recoding of fe10_model.ref_digits for every window width."""
import functools

import pytest

import fe10_model as m
from oracle.merlin import Rng

pytestmark = pytest.mark.gpu
WIDTHS = list(range(2, 17))


@functools.lru_cache(maxsize=None)
def cases(c):
    sc = m.digit_scalars(c, Rng(40 + c, b"digit-cases"))
    return sc, [m.ref_digits(s, c) for s in sc]


def ranges(c):
    Wn = m.windows(c)
    return [(0, Wn), (0, Wn // 3), (Wn // 3, Wn - Wn // 3)]  # (wb, windows)


@pytest.mark.parametrize("c", WIDTHS)
def test_reference_recoding_properties(c):
    sc, ref = cases(c)
    half = 1 << (c - 1)
    for s, d in zip(sc, ref):
        assert sum(x << (c * w) for w, x in enumerate(d)) == s
        assert all(abs(x) <= half for x in d) and d[-1] >= 0
    # the cases reach both ends of a window's digit range and a carry into the top window
    flat = [x for d in ref for x in d[:-1]]
    assert -half in flat and half - 1 in flat and 0 in flat


@pytest.mark.parametrize("c", WIDTHS)
def test_window_geometry(c):
    g = m.probe().geom(c)
    Wn = m.windows(c)
    assert (g["W"], g["B"], g["K"]) == (Wn, 1 << (c - 1), m.ref_K(c))
    assert (g["dt_W"], g["dt_H"], g["dt_K"]) == (Wn, 1 << (c - 1), m.ref_K(c))
    assert g["NC"] == (1 << (c - 1)) >> 7 and g["tfb"] <= 7


@pytest.mark.parametrize("c", WIDTHS)
def test_for_each_digit_full_and_split(c):
    sc, ref = cases(c)
    for wb, n in ranges(c):
        got = m.probe().for_each_digit(c, wb, n, sc)
        assert got == [d[wb: wb + n] for d in ref], (wb, n)


@pytest.mark.parametrize("c", WIDTHS)
def test_msm_digits_codes(c):
    sc, ref = cases(c)
    for wb, n in ranges(c):
        got = m.probe().msm_digits(c, wb, n, sc)
        assert got == [[m.dig16(x) for x in d[wb: wb + n]] for d in ref], (wb, n)


@pytest.mark.parametrize("c", range(12, 17))
def test_rsort_digits_count_codes_and_coarse_counts(c):
    """The closed form (s + K) >> cw of the radix path's first kernel: the
    same codes, and per window a coarse histogram whose counts sum to the
    number of non-zero digits with every digit in the bin rs_bin gives."""
    sc, ref = cases(c)
    g = m.probe().geom(c)
    NC, Wn = g["NC"], m.windows(c)
    for wb, n in ranges(c):
        dig, cnt, bins = m.probe().rsort_digits_count(c, wb, n, sc, NC)
        assert dig == [[m.dig16(x) for x in d[wb: wb + n]] for d in ref], (wb, n)
        for ww in range(n):
            fbits = g["tfb"] if wb + ww + 1 == Wn else 7
            hist = [0] * NC
            for i, d in enumerate(ref):
                x = d[wb + ww]
                if x == 0:
                    assert bins[i][ww] == 0xFFFFFFFF
                    continue
                assert bins[i][ww] == min((abs(x) - 1) >> fbits, NC - 1) < NC
                hist[bins[i][ww]] += 1
            assert cnt[ww] == hist, (wb, ww)
            assert sum(cnt[ww]) == sum(1 for d in ref if d[wb + ww] != 0)


@pytest.mark.parametrize("c", WIDTHS)
def test_dt_lane_row_of(c):
    sc, ref = cases(c)
    Wn, H = m.windows(c), 1 << (c - 1)
    for gen in (0, 3):
        got = m.probe().dt_rows(c, gen, sc)
        for s, d, rows in zip(sc, ref, got):
            want = [((gen * Wn + w) * H + (abs(x) - 1 if x else 0), int(x < 0), int(x == 0)) for w, x in enumerate(d)]
            assert rows == want, hex(s)
