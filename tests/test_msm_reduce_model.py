"""The level algebra of the single-MSM bucket reduction (msm_kernels.cuh
k_msm_reduce_lanes + k_msm_reduce_fold, msm.hip horner_host_terms) with
integers mod a prime in place of points: the terms the two kernels write,
pushed through a copy of the host Horner rule, are sum_b (b+1) s_b 2^(c w)
over the windows.

The model follows the kernels index by index: the peeled descending running
sums of a lane, the fold's lane-to-sum map j = i nt + t, its block roles and
the in-place bit tree with its slot arithmetic.  L, the fold's block size and
the bounds of the path are read from the header."""
import random
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "bulletproof-perm_amd" / "csrc"
P = (1 << 61) - 1  # the "group": integers mod a prime


def _define(name: str) -> int:
    text = (CSRC / "msm_kernels.cuh").read_text()
    hits = re.findall(rf"^#define {name} (\d+)\b", text, flags=re.M)
    assert len(hits) == 1, (name, hits)
    return int(hits[0])


RWAVE_LOG, RWAVE_LOG_LONE = _define("RWAVE_LOG"), _define("RWAVE_LOG_LONE")
NW_MAX = _define("RWAVE_NW_MAX")
LOGS = sorted({RWAVE_LOG, RWAVE_LOG_LONE})
# lanes of a fold block, by the reduction shape (msm.hip)
FOLD_T = {RWAVE_LOG_LONE: _define("RFOLD_T_LONE"), RWAVE_LOG: _define("RFOLD_T")}


class Adds:
    """Counts additions and the longest dependent chain."""

    def __init__(self):
        self.n = 0

    def add(self, a, b):
        self.n += 1
        return ((a[0] + b[0]) % P, max(a[1], b[1]) + 1)


def lanes(s, log, ops):
    """k_msm_reduce_lanes<log> over one segment's bucket sums s (None =
    empty): (acc_j, run_j) per lane; values are (integer, chain depth)."""
    L = 1 << log
    out = []
    for j in range(len(s) // L):
        run = acc = (0, 0)
        have = False
        for i in range(L - 1, -1, -1):
            v = s[L * j + i]
            ne = v is not None
            if ne:
                run = ops.add(run, (v, 0)) if have else (v, 0)
            if have:
                acc = ops.add(acc, run)
            elif ne:
                acc = run
            have = have or ne
        out.append((acc, run))
    return out


def block_tree(vals, ops):
    vals = list(vals)
    while len(vals) > 1:
        h = len(vals) // 2
        vals = [ops.add(vals[i], vals[i + h]) for i in range(h)]
    return vals[0]


def fold(part, ops, nt_max):
    """k_msm_reduce_fold over one segment in blocks of min(nt_max, J) lanes:
    [X, Y_0, Y_1, ...]."""
    J = len(part)
    nt = min(nt_max, J)
    q = J // nt
    ln, lq = nt.bit_length() - 1, q.bit_length() - 1
    assert nt << lq == J
    terms = [None] * (1 + ln + lq)
    for role in range(2 + lq):
        src = [p[0 if role == 0 else 1] for p in part]
        if role >= 2:
            bit = 1 << (role - 2)
            v = []
            for t in range(nt):
                x = src[bit * nt + t]
                for i in range(bit + 1, q):
                    if i & bit:
                        x = ops.add(x, src[i * nt + t])
                v.append(x)
            terms[1 + ln + role - 2] = block_tree(v, ops)
            continue
        v = []
        for t in range(nt):
            x = src[t]
            for i in range(1, q):
                x = ops.add(x, src[i * nt + t])
            v.append(x)
        if role == 0:
            terms[0] = block_tree(v, ops)
            continue
        tl = list(v)  # the bit tree, in place
        s, h = 0, nt >> 1
        while h > 0:
            new = {}
            for t in range((s + 1) * h):
                row, m = t >> (ln - 1 - s), t & (h - 1)
                p = ((nt >> row) if row else 0) + m
                new[p] = ops.add(tl[p], tl[p + h])
            assert not any(p + h in new for p in new)  # no slot read and written in one level
            for p, x in new.items():
                tl[p] = x
            s, h = s + 1, h >> 1
        for k in range(ln):
            terms[1 + k] = tl[1 << k]
    return terms


def horner(terms, Wn, nterms, c, wb, rshift):
    """horner_host_terms: window j = term 0 + sum_k 2^(rshift + k) term 1+k,
    one pass in descending bit position."""
    acc, started, pos = 0, False, 0
    for j in range(Wn - 1, -1, -1):
        for k in range(nterms - 1, -1, -1):
            off = c * j + (rshift + k - 1 if k else 0)
            v = terms[j * nterms + k]
            if started:
                assert pos >= off
                acc = acc * pow(2, pos - off, P) % P
            acc = (acc + v) % P if started else v
            started, pos = True, off
    return acc * pow(2, pos + c * wb, P) % P


def reduce_windows(windows, c, log, wb=0):
    ops = Adds()
    B = 1 << (c - 1)
    assert (64 << log) <= B <= (NW_MAX << (log + 6))  # the path's bounds (msm.hip)
    terms = []
    for s in windows:
        assert len(s) == B
        terms += [x for x, _ in fold(lanes(s, log, ops), ops, FOLD_T[log])]
    nterms = len(terms) // len(windows)
    assert nterms == 1 + (c - 1 - log)
    got = horner(terms, len(windows), nterms, c, wb, log)
    want = sum(pow(2, c * (wb + j), P) * sum((b + 1) * v for b, v in enumerate(s) if v is not None)
               for j, s in enumerate(windows)) % P
    return got, want, ops


def _window(rng, B, live=None, p_empty=0.2):
    live = B if live is None else live
    return [rng.randrange(1, P) if b < live and rng.random() >= p_empty else None for b in range(B)]


@pytest.mark.parametrize("log", LOGS)
@pytest.mark.parametrize("c", range(11, 17))
def test_terms_through_horner_give_the_bucket_sum(c, log):
    rng = random.Random(100 * c + log)
    B = 1 << (c - 1)
    top_bits = 253 - c * ((254 + c - 1) // c - 1)  # the narrow top window: digits < 2^top_bits
    windows = [_window(rng, B), _window(rng, B, p_empty=0.9), _window(rng, B, live=min(B, 1 << top_bits))]
    got, want, _ = reduce_windows(windows, c, log, wb=(254 + c - 1) // c - 3)
    assert got == want


@pytest.mark.parametrize("log", LOGS)
@pytest.mark.parametrize("c", [11, 13, 16])
@pytest.mark.parametrize("which", ["bucket0", "top", "both", "none", "full"])
def test_single_buckets(c, log, which):
    B = 1 << (c - 1)
    s = [None] * B
    if which in ("bucket0", "both"):
        s[0] = 12345
    if which in ("top", "both"):
        s[B - 1] = 777
    if which == "full":
        s = list(range(1, B + 1))
    got, want, _ = reduce_windows([s], c, log)
    assert got == want
    if which == "top":
        assert want == B * 777 % P


def test_budget_of_the_stream_shape():
    """The counts the kernel's header states, on the 2^20 stream's window
    (c = 16, every bucket occupied): lane-additions per lane of L buckets and
    the dependent chain from a bucket to the last term."""
    c = 16
    for log in LOGS:
        L, B = 1 << log, 1 << (c - 1)
        ops = Adds()
        part = lanes(list(range(1, B + 1)), log, ops)
        J = len(part)
        assert ops.n == (2 * L - 2) * J
        terms = fold(part, ops, FOLD_T[log])
        # X and r_t take every lane once, a lane's run joins half of the
        # log2 q upper-bit sums, the bit tree is < 2 nt
        nt = min(FOLD_T[log], J)
        lq = (J // nt).bit_length() - 1
        assert ops.n - (2 * L - 2) * J <= (4 + lq) * J // 2 + 2 * nt
        assert ops.n <= (2 * L + 5) * J
        chain = max(d for _, d in terms)
        assert chain <= (2 * L - 2) + (J // nt - 1) + (nt.bit_length() - 1)
        assert chain <= 2 * L + 24
