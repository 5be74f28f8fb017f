"""Designed inputs for the MSM bucket engine's tests (pure Python: no GPU, no
ctypes).

The engine sorts every (term, window) digit into its bucket, lays the buckets
of all windows end to end in one entry array, and gives lane l of
k_msm_accumulate entries [l K, (l + 1) K).  What a lane does with a bucket
depends only on where the bucket's entries fall in that partition, so an
input is designed as bucket sizes:

  scalars_from_digits  signed radix-2^c digit rows -> canonical scalars, each
                       checked against fe10_model.ref_digits
  occupancy            bucket sizes and signs of one window -> scalars
  classify             the lane partition alone: which of the accumulate's
                       cases each non-empty bucket is
  profile_set          the bucket layouts the GPU tests run, built for a
                       given K so that every case sits where it is meant to
  degenerate_points    tables holding the identity, repeats and P beside -P

test_msm_shapes.py holds the designs to their purpose on the CPU;
test_gpu_msm_shapes.py runs them.
"""
from __future__ import annotations

from collections import Counter, namedtuple

import fe10_model as m
from oracle import ristretto as r255
from oracle.merlin import Rng

L = r255.L

# The lane partition's two constants, stated once (test_msm_shapes.py parses
# msm_kernels.cuh and compares):
LANES_PER_WG = 256  # ACC_T: lanes (threads) of one k_msm_accumulate workgroup
HEAVY_LANES = 8     # FIX_MAX: a bucket ending this many lanes past its first is heavy

CLASSES = ("in_lane", "in_workgroup", "crosses_workgroup", "heavy_at_lane_start", "heavy_mid_lane")

# msm_choose_c as a table: first n of each window width.  c = 14 never wins.
CHOOSE_C = ((1, 2), (6, 3), (22, 4), (60, 5), (181, 6), (426, 7), (888, 8), (2855, 9), (5047, 10), (14485, 11),
            (26331, 12), (47394, 13), (168519, 15), (631955, 16))
# radix sort: fine bits of the narrow top window (msm_geom's tfb) per width
TFB = {12: 0, 13: 1, 15: 6, 16: 5}
RS_FINE_BITS = 7


def top_fine_bits(c: int) -> int:
    """msm_geom's rule: a top window narrower than the others is spread over
    all 2^(c - 1 - RS_FINE_BITS) coarse bins."""
    top, lognc = 253 - c * (m.windows(c) - 1), c - 1 - RS_FINE_BITS
    return RS_FINE_BITS if top >= c - 1 or lognc < 0 else max(top - lognc, 0)


LDS_MIN_N = 16384 # single MSMs below this use the global-atomic count / scatter
RADIX_MIN_C = 12   # from here (n >= 26331) the two-pass radix sort, unless BPP_MSM_LDS_SORT


def choose_c(n: int) -> int:
    c = CHOOSE_C[0][1]
    for first, width in CHOOSE_C:
        if n >= first:
            c = width
    return c


def front_end(n: int, lds_env: bool = False) -> str:
    """Which sort front end a single MSM of n terms runs."""
    if n < LDS_MIN_N:
        return "atomic"
    return "radix" if choose_c(n) >= RADIX_MIN_C and not lds_env else "lds"


# ---------------------------------------------------------------- scalars
def scalars_from_digits(c: int, rows) -> list[int]:
    """rows[i][w] = signed radix-2^c digit of window w.  Returns the scalars;
    raises ValueError when a row is not the recoding of a scalar in [0, l)."""
    Wn = m.windows(c)
    out = []
    for row in rows:
        row = list(row)
        if len(row) != Wn:
            raise ValueError(f"{len(row)} digits, {Wn} windows at c = {c}")
        s = sum(d << (c * w) for w, d in enumerate(row))
        if not 0 <= s < L:
            raise ValueError("digits do not describe a scalar in [0, l)")
        if m.ref_digits(s, c) != row:
            raise ValueError(f"{row} is not the signed recoding of {s}")
        out.append(s)
    assert all(m.ref_digits(s, c) == list(row) for s, row in zip(out, rows))
    return out


def occupancy(c: int, window: int, sizes, signs=None) -> list[int]:
    """Scalars whose only digit in `window` puts sizes[b] terms into bucket b
    (bucket b holds |digit| = b + 1), bucket by bucket.  sizes: {bucket: count}
    or a list; signs[b]: '+', '-' or '+-' (alternating, '+' first), default
    '+'.  A negative digit borrows: its scalar has digit +1 in the next
    window.  The top bucket 2^(c-1) - 1 is digit -2^(c-1) (a window value of
    exactly 2^(c-1) recodes with a carry), so it takes '-' below the top
    window."""
    Wn = m.windows(c)
    if isinstance(sizes, (list, tuple)):
        sizes = {b: k for b, k in enumerate(sizes) if k}
    signs = signs or {}
    rows = []
    for b in sorted(sizes):
        pattern = signs.get(b, "+")
        for j in range(sizes[b]):
            sg = pattern[j % len(pattern)]
            row = [0] * Wn
            if sg == "+":
                row[window] = b + 1
            else:
                if window + 1 >= Wn:
                    raise ValueError("no negative digit in the top window")
                row[window] = -(b + 1)
                row[window + 1] = 1
            rows.append(row)
    return scalars_from_digits(c, rows)


def bucket_sizes(c: int, scalars, wb: int = 0, we: int | None = None) -> list[list[int]]:
    """Per window of [wb, we): terms per bucket, from fe10_model.ref_digits."""
    Wn = m.windows(c)
    we = Wn if we is None else we
    out = [[0] * (1 << (c - 1)) for _ in range(wb, we)]
    for s in scalars:
        d = m.ref_digits(s, c)
        for w in range(wb, we):
            if d[w]:
                out[w - wb][abs(d[w]) - 1] += 1
    return out


# ---------------------------------------------------------------- lane partition
Bucket = namedtuple("Bucket", "segment bucket start size first_lane last_lane cls")
Partition = namedtuple("Partition", "buckets classes empty_runs entries last_lane_entries")


def classify(sizes_per_segment, K: int) -> Partition:
    """The lane partition of the bucket-sorted entry array: segments
    (windows) follow each other, lane l owns entries [l K, (l + 1) K).
    -> buckets: one Bucket per non-empty bucket with its class;
       classes: Counter of the classes;
       empty_runs: lengths of the runs of empty buckets that lie between two
                   occupied buckets of one segment;
       entries: all entries; last_lane_entries: entries in the last lane used
                (K when it is full)."""
    buckets, runs = [], []
    pos = 0
    for seg, sizes in enumerate(sizes_per_segment):
        gap, seen = 0, False
        for b, n in enumerate(sizes):
            if n == 0:
                gap += 1
                continue
            if seen and gap:
                runs.append(gap)
            gap, seen = 0, True
            l0, l1 = pos // K, (pos + n - 1) // K
            if l1 - l0 >= HEAVY_LANES:
                cls = "heavy_at_lane_start" if pos % K == 0 else "heavy_mid_lane"
            elif l0 == l1:
                cls = "in_lane"
            elif l0 // LANES_PER_WG == l1 // LANES_PER_WG:
                cls = "in_workgroup"
            else:
                cls = "crosses_workgroup"
            buckets.append(Bucket(seg, b, pos, n, l0, l1, cls))
            pos += n
    return Partition(buckets, Counter(x.cls for x in buckets), runs, pos, (pos % K or K) if pos else 0)


# ---------------------------------------------------------------- designed layouts
Profile = namedtuple("Profile", "name K c window n sizes signs")

_SIGNS = ("+", "-", "+-")
SPAN_LANES = (7, 8, 9, 10)  # lanes a span bucket touches; 9 and up is heavy


def span_offsets(K: int):
    """A lane's first, second and last entry."""
    return (0, 1, K - 1)


class _Layout:
    """Consecutive buckets of one window, tracked by entry position."""

    def __init__(self, K):
        self.K, self.pos, self.b = K, 0, 0
        self.sizes, self.signs = {}, {}

    def add(self, size, sign=None):
        assert size > 0
        self.sizes[self.b] = size
        self.signs[self.b] = sign or _SIGNS[self.b % 3]
        self.b += 1
        self.pos += size

    def gap(self, k):
        self.b += k

    def align(self, off):
        """One filler bucket (none if already there) so the next bucket starts
        at entry `off` of a lane."""
        d = (off - self.pos) % self.K
        if d:
            self.add(d)

    def fill_to(self, target):
        """Filler buckets of mixed sizes (from one entry to 29 lanes) up to
        entry position `target`."""
        K = self.K
        cyc = (17 * K + 3, 5 * K + 1, 29 * K, 2 * K - 1, 11 * K + 2, 3, 6 * K, 1, 8 * K + 1, 7 * K)
        assert target >= self.pos, (target, self.pos)
        i = 0
        while self.pos < target:
            self.add(min(cyc[i % len(cyc)], target - self.pos))
            i += 1

    def negatives(self):
        per = {"+": lambda n: 0, "-": lambda n: n, "+-": lambda n: n // 2}
        return sum(per[self.signs[b]](n) for b, n in self.sizes.items())

    def finish(self, name, c, window, total, exact):
        """Pads to `total` terms, then the top bucket.  Unless `exact`, one
        more term joins the top bucket when the entries (the terms and the
        borrow digits of the negative ones) would fill the last lane."""
        K = self.K
        top = K + 2
        self.fill_to(total - top)
        if not exact and (self.pos + top + self.negatives() + top) % K == 0:
            top += 1
        n = self.pos + top
        c = c or choose_c(n)
        B = 1 << (c - 1)
        assert self.b + 4 <= B - 1, f"{name}: {self.b} buckets do not fit c = {c}"
        self.sizes[B - 1] = top  # after a run of empty buckets
        self.signs[B - 1] = "-"
        Wn = m.windows(c)
        window = Wn + window if window < 0 else window
        return Profile(name, K, c, window, n, dict(self.sizes), dict(self.signs))


def spans_profile(K: int, c: int | None = None, window: int = 1, total: int | None = None) -> Profile:
    """Small buckets, then buckets touching exactly 7, 8, 9 and 10 lanes from
    each alignment, a light bucket over the first workgroup border and a heavy
    one starting in mid-lane."""
    lay = _Layout(K)
    lay.add(1, "+")            # bucket 0
    lay.add(K - 1, "-")
    lay.add(K, "+-")
    lay.add(K + 1, "+")
    lay.add(2 * K, "+-")
    lay.gap(3)
    for lanes in SPAN_LANES:
        d = lanes - 1  # last lane - first lane
        for off in span_offsets(K):
            lay.align(off)
            # smallest such bucket (one entry in its last lane); from a
            # lane's second entry the largest (its last lane full)
            lay.add((d + 1) * K - off if off == 1 else d * K - off + 1)
    border = LANES_PER_WG * K
    lay.fill_to(border - K - 1)
    lay.add(3 * K, "+-")        # lanes 254..257: leaves the workgroup, not heavy
    lay.gap(5)
    lay.align(2 % K)
    lay.add(11 * K + 1)         # heavy, starts in mid-lane
    return lay.finish(f"spans-K{K}", c, window, total or border + 120 * K, exact=total is not None)


def borders_profile(K: int, c: int | None = None, window: int = -2, total: int | None = None) -> Profile:
    """The three first workgroup borders: a heavy bucket from mid-lane over
    the first, a heavy bucket from a lane's first entry over the second, a
    two-lane bucket over the third.  window = -2: the borrow digits of its
    negative terms land in the top window."""
    lay = _Layout(K)
    border = LANES_PER_WG * K
    lay.add(2 * K + 1, "+-")    # bucket 0
    lay.fill_to(border - 3 * K - 2)
    lay.add(13 * K, "+-")       # heavy, mid-lane, over the border
    lay.gap(4)
    lay.fill_to(2 * border - 2 * K)
    lay.add(12 * K, "-")        # heavy, from a lane's first entry, over the border
    lay.fill_to(3 * border - 1)
    lay.add(K + 1, "+")         # last entry of lane 767 and all of lane 768
    lay.fill_to(3 * border + 5 * K)
    lay.add(7 * K + 2)
    return lay.finish(f"borders-K{K}", c, window, total or 3 * border + 57 * K, exact=total is not None)


def profile_set(K: int) -> list[Profile]:
    """The designed profiles the GPU tests run with BPP_MSM_ACC_K = K."""
    return [spans_profile(K), borders_profile(K)]


def profile_scalars(p: Profile) -> list[int]:
    return occupancy(p.c, p.window, p.sizes, p.signs)


def features(p: Profile) -> set[str]:
    """What a profile's scalars hit at its K, judged from the scalars alone
    (their ref_digits, then classify): the five classes and the placements
    that profile_set is designed to contain."""
    K = p.K
    scalars = profile_scalars(p)
    part = classify(bucket_sizes(p.c, scalars), K)
    mine = [b for b in part.buckets if b.segment == p.window]
    out = {f"class:{b.cls}" for b in part.buckets}
    names = {1: "1", K - 1: "K-1", K: "K", K + 1: "K+1", 2 * K: "2K"}
    out |= {f"size:{names[b.size]}" for b in mine if b.size in names}
    where = dict(zip(span_offsets(K), ("first", "second", "last")))
    for b in mine:
        lanes = b.last_lane - b.first_lane + 1
        if lanes in SPAN_LANES and b.start % K in where:
            out.add(f"span:{lanes}-lanes-from-{where[b.start % K]}-entry")
        over = b.first_lane // LANES_PER_WG != b.last_lane // LANES_PER_WG
        if over:
            out.add("over-border:heavy" if b.cls.startswith("heavy") else "over-border:light")
        if b.bucket == 0:
            out.add("bucket:0")
        if b.bucket == (1 << (p.c - 1)) - 1:
            out.add("bucket:top")
    digits = Counter(m.ref_digits(s, p.c)[p.window] for s in scalars)
    if any(d > 0 and digits[-d] for d in digits):
        out.add("both-signs-in-one-bucket")
    if any(r >= 3 for r in part.empty_runs):
        out.add("empty-run>=3")
    if part.last_lane_entries < K:
        out.add("last-lane-not-full")
    return out


def required_features(K: int) -> set[str]:
    req = {f"class:{c}" for c in CLASSES}
    req |= {f"size:{s}" for s in ("1", "K-1", "K", "K+1", "2K")}
    req |= {f"span:{lanes}-lanes-from-{w}-entry" for lanes in SPAN_LANES for w in ("first", "second", "last")}
    req |= {"over-border:heavy", "over-border:light", "bucket:0", "bucket:top", "both-signs-in-one-bucket",
            "empty-run>=3", "last-lane-not-full"}
    return req


def mixed_scalars(n: int, K: int = 4, seed: int = 5) -> tuple[Profile, list[int]]:
    """n terms for the width the engine picks at n: every fourth follows
    borders_profile(K) in window 1, the rest are random."""
    p = borders_profile(K, c=choose_c(n), window=1, total=n // 4)
    designed = profile_scalars(p)
    rng = Rng(seed, b"msm-shapes-mixed")
    out = [rng.scalar() for _ in range(n)]
    out[::4] = designed + out[4 * len(designed)::4]
    return p, out


def few_value_scalars(n: int, values: int = 8, seed: int = 6) -> list[int]:
    """n scalars drawn from `values` distinct ones: at most that many
    occupied (heavy) buckets in every window."""
    rng = Rng(seed, b"msm-shapes-few")
    vals = [rng.scalar() for _ in range(values)]
    return [vals[rng.bytes(1)[0] % values] for _ in range(n)]


def top_bit_scalars(n: int, seed: int = 12) -> list[int]:
    """Every scalar in [2^252, l): bit 252 set, so the one-bit top window of
    c = 12 has all n terms in its bucket 0."""
    rng = Rng(seed, b"msm-shapes-top")
    return [(1 << 252) + rng.scalar() % (L - (1 << 252)) for _ in range(n)]


def spread(items: list, stride: int = 7) -> list:
    """A fixed permutation (i -> i * stride mod n, stride made coprime), so
    that designed scalars do not meet the point table bucket by bucket."""
    n = len(items)
    from math import gcd
    while gcd(stride, n) != 1:
        stride += 1
    return [items[(i * stride) % n] for i in range(n)]


def adversarial_digit_scalars(c: int, n: int, seed: int) -> list[int]:
    """fe10_model.digit_scalars(c) ordered as test_msm_adversarial_window_scalars
    orders them (whole-scalar patterns, the longest carry chains, the rest),
    cycled to n."""
    Wn = m.windows(c)
    fams = m.digit_scalars(c, Rng(seed, b"test-scalars"), nrand=8)
    order = fams[5:11] + fams[11:11 + Wn][::-1] + fams[:5] + fams[11 + Wn:]
    return [order[i % len(order)] for i in range(n)]


# ---------------------------------------------------------------- points
DEGENERATE_N = 300


def degenerate_points() -> dict:
    """Tables of DEGENERATE_N encodings each (r255.encode; load them with
    ctx.decompress), with the points behind them:
      mixed      the identity, the basepoint, one point 60 times, 60 (P, -P)
                 pairs over 6 points, random points between
      same       one point everywhere
      pairs      P_j, -P_j alternating over 5 points
      identity4  random points, every fourth entry the identity
    -> {name: (encodings, points)}"""
    rng = Rng(300, b"msm-shapes-points")
    rnd = [rng.point() for _ in range(24)]
    P = rnd[0]
    mixed = [r255.IDENTITY, r255.BASEPOINT] + [P] * 60
    for j in range(60):
        mixed += [rnd[1 + j % 6], r255.ed_neg(rnd[1 + j % 6])]
    while len(mixed) < DEGENERATE_N:
        k = len(mixed)
        mixed.append(r255.IDENTITY if k % 11 == 0 else rnd[7 + k % 17])
    pairs = []
    for j in range(DEGENERATE_N // 2):
        pairs += [rnd[j % 5], r255.ed_neg(rnd[j % 5])]
    ident4 = [r255.IDENTITY if k % 4 == 3 else rnd[k % 23] for k in range(DEGENERATE_N)]
    tables = {"mixed": mixed, "same": [P] * DEGENERATE_N, "pairs": pairs, "identity4": ident4}
    out = {}
    for name, pts in tables.items():
        assert len(pts) == DEGENERATE_N
        enc = {}
        for p in pts:  # (each distinct point encoded once)
            if p not in enc:
                enc[p] = r255.encode(p)
        out[name] = ([enc[p] for p in pts], pts)
    return out
