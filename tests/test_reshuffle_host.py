"""bpp_reshuffle_* and bpp_masked_reshuffle_* without a GPU: for both kinds the
proof length against the reference helper (tests/reshuffle_ref.py,
tests/masked_reshuffle_ref.py), every argument check that needs no device with
its code and in its order, and nothing written by a refused call; the Python
binding's own refusals, and the committed fixtures (tests/golden/reshuffle.json)
against the reference that wrote them."""
import ctypes
import json
import sys
from pathlib import Path
from typing import NamedTuple

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import masked_reshuffle_ref as mr  # noqa: E402
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


class Kind(NamedTuple):
    """One kind of re-shuffle at the C ABI: the exports' stem, the bytes of a
    card, the key every call takes behind count (None: the kind has none), its
    reference module and its committed cases."""
    stem: str
    card: int
    key: "bytes | None"
    ref: object
    golden: list
    len52: int

    def fn(self, lib, name):
        return getattr(lib, "%s_%s" % (self.stem, name))

    def keyed(self, key="own"):
        """the key argument(s) of one call: none, this kind's key, or the one given"""
        return () if self.key is None else (self.key if key == "own" else key,)


MASKED_GOLDEN = json.loads((HERE / "golden" / "masked_reshuffle.json").read_text())["cases"]
KINDS = [Kind("bpp_reshuffle", 32, None, rr, GOLDEN, 9280),
         Kind("bpp_masked_reshuffle", 64, mr.rand_point(b"host-key"), mr, MASKED_GOLDEN, 9312)]
kinds = pytest.mark.parametrize("kind", KINDS, ids=lambda kd: kd.stem[4:])


@kinds
def test_proof_len_matches_the_reference(lib, kind):
    proof_len = kind.fn(lib, "proof_len")
    for k in list(range(2, 40)) + [52, 64, 65, 66, 129, 130, 257, 258, 341, 342]:
        assert proof_len(k) == kind.ref.proof_len(k), k
    assert proof_len(52) == kind.len52
    for k in (0, 1, 343, 1 << 20, (1 << 32) - 1):
        assert proof_len(k) == 0, k


def u32s(xs):
    return (ctypes.c_uint32 * len(xs))(*xs)


@kinds
def test_prover_checks_in_their_order(lib, kind):
    """count = 2, k = 3.  Null arrays (the key among them, where the kind has
    one) and k < 2 (ARG) first; a perm that is no bijection (ARG) wins over a
    blind >= l (NONCANONICAL), which wins over k > 342 (LEN), the null handles
    (ARG) last.  No output byte is written."""
    k, count, ref = 3, 2, kind.ref
    cards = b"".join(ref.rand_cards(k * count, b"host"))
    assert len(cards) == kind.card * k * count
    good = [2, 0, 1, 1, 2, 0]
    blinds = b"".join(ref.sb(ref.rand_scalar(b"hb%d" % i)) for i in range(k * count))
    seeds = ref.seed32(b"h0") + ref.seed32(b"h1")
    out = ctypes.create_string_buffer(b"\xaa" * (kind.card * k * count))
    pf = ctypes.create_string_buffer(b"\xaa" * (ref.proof_len(k) * count))
    prove_batch = kind.fn(lib, "prove_batch")

    def prove(perms=good, blinds_=blinds, k_=k, cards_=cards, out_=out, pf_=pf, count_=count, label=b"x", llen=1,
              key="own"):
        return prove_batch(None, None, k_, count_, *kind.keyed(key), cards_, u32s(perms), blinds_, seeds, label, llen,
                           out_, pf_)

    assert prove(cards_=None) == ARG and prove(out_=None) == ARG and prove(pf_=None) == ARG
    assert prove(label=None) == ARG and prove(k_=1) == ARG and prove(k_=0) == ARG
    assert prove_batch(None, None, k, count, *kind.keyed(), cards, None, None, seeds, b"x", 1, out, pf) == ARG
    bad_blinds = blinds[:32 * 4] + BAD_SCALAR + blinds[32 * 5:]  # in proof 1
    assert prove([2, 0, 1, 1, 1, 0]) == ARG                      # a repeat, in proof 1
    assert prove([2, 0, 3, 1, 2, 0]) == ARG                      # an index out of range, in proof 0
    assert prove([2, 0, 1, 1, 1, 0], bad_blinds) == ARG          # the perm wins
    assert prove(good, bad_blinds) == NONCANONICAL
    assert prove(good, b"\xff" * 32 + blinds[32:]) == NONCANONICAL
    assert prove(good, bad_blinds, cards_=None) == ARG           # a null array: the first check, before the witness
    # k > 342: after the witness checks, before the handles
    kk = 343
    big = list(range(kk)) * 2

    def prove_big(key="own", blinds_=None):
        return prove_batch(None, None, kk, 2, *kind.keyed(key), bytes(kind.card * kk * 2), u32s(big), blinds_, seeds,
                           b"x", 1, out, pf)

    assert prove_big() == LEN
    assert prove_big(blinds_=BAD_SCALAR + bytes(32 * (2 * kk - 1))) == NONCANONICAL
    if kind.key is not None:  # a null key with count != 0: ARG, in the first check with the other arrays
        assert prove(key=None) == ARG and prove(good, bad_blinds, key=None) == ARG and prove_big(key=None) == ARG
    assert prove(good, blinds) == ARG and prove(good, None) == ARG  # all fine: now the null context
    assert prove(count_=0) == ARG                                    # (the handles are checked before count == 0)
    assert prove(count_=0, key=None) == ARG
    assert out.raw[:kind.card * k * count] == b"\xaa" * (kind.card * k * count)
    assert pf.raw[:ref.proof_len(k) * count] == b"\xaa" * (ref.proof_len(k) * count)


@kinds
def test_verifier_checks_in_their_order(lib, kind):
    """Null arrays (the key among them, where the kind has one) and k (ARG /
    LEN), then a response scalar >= l (NONCANONICAL: z_0, om_{k-1} and z_R, in
    the first and in the last proof), then the null handles (ARG); ok_out is
    zeroed by every refusal."""
    k, ref = 3, kind.ref
    case = next(c for c in kind.golden if c["k"] == k)
    ci, co = bytes.fromhex("".join(case["cards_in"])), bytes.fromhex("".join(case["cards_out"]))
    assert len(ci) == len(co) == kind.card * k
    pf = bytes.fromhex(case["proof"])
    pl = ref.proof_len(k)
    lab = case["label"].encode()
    o = {name: off for name, off, _ in ref.regions(k)}
    verify, verify_batch, verify_each = (kind.fn(lib, n) for n in ("verify", "verify_batch", "verify_batch_each"))

    def single(pf_=pf, k_=k, ci_=ci, co_=co, n=None, key="own"):
        return verify(None, None, k_, *kind.keyed(key), lab, len(lab), ci_, co_, pf_, len(pf_) if n is None else n)

    def batch(pfs, count, k_=k, each=False, key="own"):
        ok = ctypes.create_string_buffer(b"\x01" * max(count, 1))
        if each:
            rc = verify_each(None, None, k_, count, *kind.keyed(key), lab, len(lab), ci * count, co * count, pfs, ok)
            assert ok.raw[:count] == b"\0" * count
            return rc
        return verify_batch(None, None, k_, count, *kind.keyed(key), lab, len(lab), ci * count, co * count, pfs)

    assert single(ci_=None) == ARG and single(co_=None) == ARG
    assert verify(None, None, k, *kind.keyed(), lab, len(lab), ci, co, None, pl) == ARG
    assert single(k_=1) == ARG and single(k_=343) == LEN
    for where in (o["z"], o["om"] + 32 * (k - 1), o["zR"]):
        bad = pf[:where] + BAD_SCALAR + pf[where + 32:]
        assert single(bad) == NONCANONICAL, where
        assert batch(pf + pf + bad, 3) == NONCANONICAL
        assert batch(bad + pf + pf, 3, each=True) == NONCANONICAL
        assert single(bad, ci_=None) == ARG  # a null array: the first check, before the scalars
        if kind.key is not None:
            assert single(bad, key=None) == ARG and batch(bad + pf, 2, key=None) == ARG
            assert batch(bad + pf, 2, each=True, key=None) == ARG
    if kind.key is not None:  # a null key with count != 0: ARG, in the first check with the other arrays
        assert single(key=None) == ARG and single(k_=343, key=None) == ARG
        assert batch(pf * 2, 2, key=None) == ARG and batch(pf * 2, 2, each=True, key=None) == ARG
    assert single() == ARG and batch(pf * 2, 2) == ARG and batch(pf * 2, 2, each=True) == ARG  # the null context
    assert single(n=pl - 32) == ARG  # (a wrong length is a verdict, reached only with a context)
    assert verify_each(None, None, k, 2, *kind.keyed(), lab, len(lab), ci * 2, co * 2, pf * 2, None) == ARG
    assert batch(b"", 0) == ARG and batch(b"", 0, key=None) == ARG


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
