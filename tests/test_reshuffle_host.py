"""bpp_reshuffle_* without a GPU: the proof length against the reference helper
(tests/reshuffle_ref.py), every argument check that needs no device with its
code and in its order, nothing written by a refused call, the Python binding's
own refusals, and the committed fixtures (tests/golden/reshuffle.json) against
the reference that wrote them."""
import ctypes
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import reshuffle_ref as rr  # noqa: E402

HERE = Path(__file__).resolve().parent
GOLDEN = json.loads((HERE / "golden" / "reshuffle.json").read_text())["cases"]
L = rr.L
ARG, LEN, NONCANONICAL = 1, 2, 4
BAD_SCALAR = L.to_bytes(32, "little")


@pytest.fixture(scope="module")
def lib():
    from bpperm import _lib
    return _lib.load()


def test_proof_len_matches_the_reference(lib):
    for k in list(range(2, 40)) + [52, 64, 65, 66, 129, 130, 257, 258, 341, 342]:
        assert lib.bpp_reshuffle_proof_len(k) == rr.proof_len(k), k
    assert lib.bpp_reshuffle_proof_len(52) == 9280
    for k in (0, 1, 343, 1 << 20, (1 << 32) - 1):
        assert lib.bpp_reshuffle_proof_len(k) == 0, k


def u32s(xs):
    return (ctypes.c_uint32 * len(xs))(*xs)


def test_prover_checks_in_their_order(lib):
    """count = 2, k = 3.  Null arrays and k < 2 (ARG) first; a perm that is no
    bijection (ARG) wins over a blind >= l (NONCANONICAL), which wins over k >
    342 (LEN), the null handles (ARG) last.  No output byte is written."""
    k, count = 3, 2
    cards = b"".join(rr.rand_cards(k * count, b"host"))
    good = [2, 0, 1, 1, 2, 0]
    blinds = b"".join(rr.sb(rr.rand_scalar(b"hb%d" % i)) for i in range(k * count))
    seeds = rr.seed32(b"h0") + rr.seed32(b"h1")
    out = ctypes.create_string_buffer(b"\xaa" * (32 * k * count))
    pf = ctypes.create_string_buffer(b"\xaa" * (rr.proof_len(k) * count))

    def prove(perms=good, blinds_=blinds, k_=k, cards_=cards, out_=out, pf_=pf, count_=count, label=b"x", llen=1):
        return lib.bpp_reshuffle_prove_batch(None, None, k_, count_, cards_, u32s(perms), blinds_, seeds, label, llen,
                                             out_, pf_)

    assert prove(cards_=None) == ARG and prove(out_=None) == ARG and prove(pf_=None) == ARG
    assert prove(label=None) == ARG and prove(k_=1) == ARG and prove(k_=0) == ARG
    assert lib.bpp_reshuffle_prove_batch(None, None, k, count, cards, None, None, seeds, b"x", 1, out, pf) == ARG
    bad_blinds = blinds[:32 * 4] + BAD_SCALAR + blinds[32 * 5:]  # in proof 1
    assert prove([2, 0, 1, 1, 1, 0]) == ARG                      # a repeat, in proof 1
    assert prove([2, 0, 3, 1, 2, 0]) == ARG                      # an index out of range, in proof 0
    assert prove([2, 0, 1, 1, 1, 0], bad_blinds) == ARG          # the perm wins
    assert prove(good, bad_blinds) == NONCANONICAL
    assert prove(good, b"\xff" * 32 + blinds[32:]) == NONCANONICAL
    # k > 342: after the witness checks, before the handles
    kk = 343
    big = list(range(kk)) * 2
    assert lib.bpp_reshuffle_prove_batch(None, None, kk, 2, bytes(32 * kk * 2), u32s(big), None, seeds, b"x", 1, out,
                                         pf) == LEN
    assert prove(good, blinds) == ARG and prove(good, None) == ARG  # all fine: now the null context
    assert prove(count_=0) == ARG                                    # (the handles are checked before count == 0)
    assert out.raw[:32 * k * count] == b"\xaa" * (32 * k * count)
    assert pf.raw[:rr.proof_len(k) * count] == b"\xaa" * (rr.proof_len(k) * count)


def test_verifier_checks_in_their_order(lib):
    """Null arrays and k (ARG / LEN), then a response scalar >= l
    (NONCANONICAL: z_0, om_{k-1} and z_R, in the first and in the last proof),
    then the null handles (ARG); ok_out is zeroed by every refusal."""
    k = 3
    case = next(c for c in GOLDEN if c["k"] == k)
    ci, co = bytes.fromhex("".join(case["cards_in"])), bytes.fromhex("".join(case["cards_out"]))
    pf = bytes.fromhex(case["proof"])
    pl = rr.proof_len(k)
    lab = case["label"].encode()
    o = {name: off for name, off, _ in rr.regions(k)}

    def single(pf_=pf, k_=k, ci_=ci, co_=co, n=None):
        return lib.bpp_reshuffle_verify(None, None, k_, lab, len(lab), ci_, co_, pf_, len(pf_) if n is None else n)

    def batch(pfs, count, k_=k, each=False):
        ok = ctypes.create_string_buffer(b"\x01" * max(count, 1))
        if each:
            rc = lib.bpp_reshuffle_verify_batch_each(None, None, k_, count, lab, len(lab), ci * count, co * count, pfs, ok)
            assert ok.raw[:count] == b"\0" * count
            return rc
        return lib.bpp_reshuffle_verify_batch(None, None, k_, count, lab, len(lab), ci * count, co * count, pfs)

    assert single(ci_=None) == ARG and single(co_=None) == ARG
    assert lib.bpp_reshuffle_verify(None, None, k, lab, len(lab), ci, co, None, pl) == ARG
    assert single(k_=1) == ARG and single(k_=343) == LEN
    for where in (o["z"], o["om"] + 32 * (k - 1), o["zR"]):
        bad = pf[:where] + BAD_SCALAR + pf[where + 32:]
        assert single(bad) == NONCANONICAL, where
        assert batch(pf + pf + bad, 3) == NONCANONICAL
        assert batch(bad + pf + pf, 3, each=True) == NONCANONICAL
    assert single() == ARG and batch(pf * 2, 2) == ARG and batch(pf * 2, 2, each=True) == ARG  # the null context
    assert single(n=pl - 32) == ARG  # (a wrong length is a verdict, reached only with a context)
    assert lib.bpp_reshuffle_verify_batch_each(None, None, k, 2, lab, len(lab), ci * 2, co * 2, pf * 2, None) == ARG
    assert batch(b"", 0) == ARG


def test_python_binding_refuses_malformed_arguments():
    import bpperm

    class FakeLib:
        @staticmethod
        def bpp_reshuffle_proof_len(k):
            return rr.proof_len(k)

    class Fake:
        h = None
        lib = FakeLib()

    class FakeGens:
        h = None
        ctx = Fake()

    rs = bpperm.Reshuffler(FakeGens(), 3)
    assert rs.proof_len == rr.proof_len(3) and rs.label == b"bp-perm"
    cards = rr.rand_cards(3, b"py")
    with pytest.raises(ValueError):
        rs.shuffle_batch([cards[:2]], [[0, 1, 2]])
    with pytest.raises(ValueError):
        rs.shuffle_batch([cards], [[0, 1]])
    with pytest.raises(ValueError):
        rs.shuffle_batch([cards], [[0, 1, 2]], seeds32=b"short")
    with pytest.raises(ValueError):
        rs.shuffle_batch([cards], [[0, 1, 2]], blinds=[[rr.sb(1)] * 2])
    with pytest.raises(ValueError):
        rs.verify_batch([cards], [cards], [b"\0" * (rs.proof_len - 1)])


def test_signatures_are_bound():
    from bpperm import _lib
    for name in ("bpp_reshuffle_proof_len", "bpp_reshuffle_prove_batch", "bpp_reshuffle_verify",
                 "bpp_reshuffle_verify_batch", "bpp_reshuffle_verify_batch_each"):
        assert name in _lib.SIGNATURES, name


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: "k%d" % c["k"])
def test_golden_fixtures_are_the_reference(case):
    """k = 2, 3, 5: the reference reproduces the committed bytes; every case
    (k = 52 too) verifies in the reference and has the stated length."""
    k = case["k"]
    ci = [bytes.fromhex(h) for h in case["cards_in"]]
    co = [bytes.fromhex(h) for h in case["cards_out"]]
    pf = bytes.fromhex(case["proof"])
    lab = case["label"].encode()
    assert len(pf) == rr.proof_len(k) and len(ci) == len(co) == k and sorted(case["perm"]) == list(range(k))
    assert rr.verify(ci, co, pf, lab)
    if k <= 5:
        blinds = [int.from_bytes(bytes.fromhex(h), "little") for h in case["blinds"]] if case["blinds"] else None
        out, proof = rr.prove(ci, case["perm"], bytes.fromhex(case["seed"]), blinds, lab)
        assert out == co and proof == pf
