"""Device scalar arithmetic mod l (sc25519.cuh) at its edges, through the
arithmetic probe: the canonical integer, equal as 8 words, against Python
integers and oracle.ristretto.scalar_from_wide."""
import pytest

import fe10_model as m
from oracle import ristretto as r255
from oracle.merlin import Rng

pytestmark = pytest.mark.gpu
L = r255.L
R = 1 << 256
RINV = pow(R, -1, L)
R2 = R * R % L
E = m.sc_edge_values()


def rand_scalars(seed, n):
    rng = Rng(seed, b"sc-cases")
    return [rng.scalar() for _ in range(n)]


def rand_u256(seed, n):
    rng = Rng(seed, b"sc-cases-u256")
    return [int.from_bytes(rng.bytes(32), "little") for _ in range(n)]


def canonical_pairs(seed):
    a = [x for x in E for _ in E] + rand_scalars(seed, 512)
    b = [y for _ in E for y in E] + rand_scalars(seed + 1, 512)
    return a, b


def test_sc_add_sub_neg_half():
    a, b = canonical_pairs(1)
    # sums that land on 0 (a = b = 0), l - 1, l, l + 1 and differences on 0, +-1
    for x in E + rand_scalars(3, 32):
        for t in (L - 1, L, L + 1):
            if 0 <= t - x < L:
                a.append(x)
                b.append(t - x)
        for y in (x, x + 1, x - 1):
            if 0 <= y < L:
                a.append(x)
                b.append(y)
    assert {(x + y) for x, y in zip(a, b)} >= {0, L - 1, L, L + 1}
    assert {(x - y) for x, y in zip(a, b)} >= {0, 1, -1, L - 1, 1 - L}
    p = m.probe()
    assert p.sc("add", a, b) == [(x + y) % L for x, y in zip(a, b)]
    assert p.sc("sub", a, b) == [(x - y) % L for x, y in zip(a, b)]
    assert p.sc("neg", a) == [(-x) % L for x in a]
    inv2 = (L + 1) // 2
    got = p.sc("half", a)
    assert got == [x * inv2 % L for x in a]
    assert {0, L - 1, inv2, (L - 1) // 2} <= set(got)


def test_sc_mont_matches_cios_and_integers():
    """a * b * R^-1 mod l with the non-reduced operand the contract admits
    (a * b < l * R: one operand < l, the other up to 2^256 - 1), in both
    orders; sc_mont (radix 2^29) equals sc_mont_cios (its reference)."""
    wide = [R - 1, R - 2, L, L + 1, 2 * L, 15 * L, 2**255, 2**253, 2**253 - 1, 16 * 2**252 - 1] + rand_u256(5, 64)
    small = E + [R2, R % L] + rand_scalars(6, 32)
    a, b = canonical_pairs(7)
    a += [x for x in wide for _ in small] + [y for _ in wide for y in small]
    b += [y for _ in wide for y in small] + [x for x in wide for _ in small]
    assert (R - 1, L - 1) in set(zip(a, b)) and (R - 1, R2) in set(zip(a, b))
    assert all(x * y < L * R for x, y in zip(a, b))
    p = m.probe()
    want = [x * y * RINV % L for x, y in zip(a, b)]
    got = p.sc("mont", a, b)
    assert got == want
    assert p.sc("mont_cios", a, b) == got
    c = E + wide + rand_scalars(8, 256)
    assert p.sc("to_mont", c) == [x * R % L for x in c]
    assert p.sc("from_mont", c) == [x * RINV % L for x in c]


def test_sc_reduce256_both_sides_of_the_add_back():
    """w - q l with one conditional add-back: w = q 2^252 + r on both sides of
    r = q delta for every q, where random input never lands."""
    w = m.reduce256_cases() + rand_u256(9, 512)
    got = m.probe().sc("reduce256", w)
    for x, g in zip(w, got):
        assert g == x % L, hex(x)
    # the cases do take the add-back branch, and do not
    assert any((x & (2**252 - 1)) < (x >> 252) * m.DELTA for x in w[:97])
    assert any((x & (2**252 - 1)) >= (x >> 252) * m.DELTA > 0 for x in w[:97])


def test_sc_from_wide():
    lo = [0, R - 1] + m.reduce256_cases()
    hi = [0, R - 1, 1, L - 1, L, 2**252]
    cases = [(x, y) for y in hi for x in lo]
    rng = Rng(10, b"sc-cases-wide")
    cases += [(int.from_bytes(rng.bytes(32), "little"), int.from_bytes(rng.bytes(32), "little")) for _ in range(512)]
    got = m.probe().sc("from_wide", [x for x, _ in cases], [y for _, y in cases])
    for (x, y), g in zip(cases, got):
        assert g == r255.scalar_from_wide((x + (y << 256)).to_bytes(64, "little")), (hex(x), hex(y))


def test_sc_wave_sum_and_shfl():
    waves = [[L - 1] * 64, [0] * 64, [L - 1] * 63 + [1], [1] + [0] * 63, [0] * 63 + [1]]
    waves += [rand_scalars(20 + k, 64) for k in range(4)]
    waves += [[E[(i + k) % len(E)] for i in range(64)] for k in range(2)]
    flat = [x for w in waves for x in w]
    p = m.probe()
    got = p.sc("wave_sum", flat)
    for k, w in enumerate(waves):
        assert got[64 * k] == sum(w) % L, k
    src = [(5 * i + k) % 64 for k in range(len(waves)) for i in range(64)]
    got = p.sc("shfl", flat, src)
    assert got == [flat[64 * (i // 64) + s] for i, s in enumerate(src)]
