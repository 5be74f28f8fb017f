"""The helpers of fe10_model.py against oracle.ristretto (no GPU): limb round
trips, the named bounds and values, the reference window recoding, and the
generated field multiplier being what its generator writes today."""
import subprocess
import sys
from pathlib import Path

import fe10_model as m
from oracle import ristretto as r255
from oracle.merlin import Rng

ROOT = Path(__file__).resolve().parent.parent


def test_limb_round_trips():
    rng = Rng(1, b"fe10-model")
    vals = m.AROUND_MODULUS + [int.from_bytes(rng.bytes(32), "little") for _ in range(64)]
    for v in vals:
        limbs = m.exact_limbs(v)
        assert m.raw_value(limbs) == v and m.value(limbs) == v % r255.P
        assert m.from_words(m.words8(v)) == v
        if v < 2**255:
            assert m.within(limbs, m.EXACT)


def test_named_bounds_are_the_headers():
    hdr = (ROOT / "bulletproof-perm_amd" / "csrc" / "fe25519.cuh").read_text()
    for text in ("limb i < 2^{w_i} + 2^18", "fe_add_nc < 2^27 + 2^19", "fe_sub_nc < 2^27 + 2^26 + 2^18",
                 "limbs < 2^27.6", "limbs < 2^32 - 2^7 in", "limb 0 < 2^26 + 19 * 2^7"):
        assert text in hdr, text
    inc = (ROOT / "bulletproof-perm_amd" / "csrc" / "fe10_ops.inc").read_text()
    assert "Inputs: limbs < 2^27.6; outputs: limbs < 2^26 (limb 1 < 2^25 + 2^18)." in inc
    # the sums of the widest (even) tight limbs give the uniform bounds
    assert m.ADD_NC[0] == 2 * m.TIGHT[0] and m.SUB_NC[0] >= m.TIGHT[0] + m.TWO_P[2]
    assert m.G_BOUND[0] == m.ADD_NC[0] + m.TIGHT[0]  # G = (Z + Z) + C, all three tight
    assert all(g < mi for g, mi in zip(m.G_BOUND, m.MUL_IN))
    assert m.MUL_IN[0] < 2**27.6 < m.MUL_IN[0] + 1
    assert m.MUL_IN[0] <= 2**32 // 19  # b19_j = 19 b_j in 32 bits is the binding limit


def test_loose_representations():
    rng = Rng(2, b"fe10-model")
    for name, bound in m.NAMED_BOUNDS.items():
        if name == "exact":
            continue
        for v in [0, 1, r255.P - 1, 19, 2**254] + [int.from_bytes(rng.bytes(32), "little") % r255.P for _ in range(16)]:
            reps = m.loose_any(v, bound)
            for x in reps:
                assert m.within(x, bound) and m.value(x) == v
            assert len({m.raw_value(x) for x in reps}) == len(reps)
    for cls in m.field_classes(rng, nrand=4):
        name = cls[0].split("/")[0]
        assert m.within(cls[1], m.NAMED_BOUNDS[name]), cls[0]
    assert m.all_at(m.TIGHT)[0] == 2**26 + 2**18 - 1 and m.all_at(m.TIGHT)[1] == 2**25 + 2**18 - 1
    assert len(m.one_hot(m.TIGHT)) == 20
    rip = m.ripple_cases()
    assert rip[0][0] == 2**26 - 20 and rip[-1][0] == 2**26 + 19 * 128 and all(x[1:] == rip[0][1:] for x in rip)


def test_scalar_cases():
    ev = m.sc_edge_values()
    assert all(0 <= x < r255.L for x in ev)
    for x in (0, 1, 2, r255.L - 1, r255.L - 2, 2**252, 2**252 - 1, (r255.L + 1) // 2, 2**224 - 1, 2**29 - 1):
        assert x in ev
    rc = m.reduce256_cases()
    assert 2**256 - 1 in rc and all(0 <= x < 2**256 for x in rc)
    # both sides of the add-back threshold for every q >= 1
    for q in range(1, 16):
        assert q * 2**252 + q * m.DELTA - 1 in rc and q * 2**252 + q * m.DELTA in rc
        assert (q * 2**252 + q * m.DELTA - 1) % r255.L == r255.L - 1 and (q * 2**252 + q * m.DELTA) % r255.L == 0


def test_reference_digits_reconstruct_every_c():
    rng = Rng(3, b"fe10-model")
    for c in range(2, 17):
        Wn = m.windows(c)
        assert Wn == -(-254 // c)
        half = 1 << (c - 1)
        K = m.ref_K(c)
        for s in m.digit_scalars(c, rng, nrand=16):
            d = m.ref_digits(s, c)
            assert len(d) == Wn and sum(x << (c * w) for w, x in enumerate(d)) == s
            assert all(-half <= x < half for x in d[:-1]) and 0 <= d[-1] <= half
            # the closed form of dt_walk.cuh / k_rsort_digits_count gives the same digits
            t = s + K
            cf = [((t >> (c * w)) & ((1 << c) - 1)) - half for w in range(Wn - 1)] + [t >> (c * (Wn - 1))]
            assert cf == d
            # where both recodings have the same window count they agree
            if (256 + c - 1) // c == Wn:
                assert r255.signed_digits(s, c) == d
            assert [m.dig16(x) for x in d].count(0x7FFF) == d.count(0)


def test_small_order_points_and_torsion():
    so = m.small_order_points()
    assert len({r255.ed_affine(p) for p in so}) == 8
    for p in so:
        assert r255.ed_on_curve(p) and r255.ed_affine(r255.ed_mul(8, p)) == (0, 1)
    t4 = m.four_torsion()
    assert len(t4) == 4
    B = r255.BASEPOINT
    for t in t4:
        assert r255.encode(r255.ed_add(B, t)) == r255.encode(B)
        assert r255.equal(r255.ed_add(B, t), B)
    words = m.p3_limbs(m.scale(B, 12345))
    assert len(words) == 40 and r255.ed_affine(m.p3_point(words)) == r255.ed_affine(B)
    nl = m.niels_limbs(m.niels_of(B))
    assert len(nl) == 32 and m.value(nl[:10]) == (r255.BY + r255.BX) % r255.P


def test_generated_multiplier_is_current(tmp_path):
    """tools/gen_fe10.py reproduces the committed csrc/fe10_ops.inc byte for byte."""
    out = tmp_path / "fe10_ops.inc"
    subprocess.run([sys.executable, str(ROOT / "tools" / "gen_fe10.py"), str(out)], check=True, capture_output=True)
    assert out.read_bytes() == (ROOT / "bulletproof-perm_amd" / "csrc" / "fe10_ops.inc").read_bytes()
