"""Public-deck shuffle proofs without a GPU: the reference helper
(tests/deck_ref.py) checks its own circuit, witness, proofs and the separation
from the two-half proof of the same shape, and the bpp_deck_* entry points
refuse a bad witness before any device work."""
import ctypes
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import deck_ref as dr  # noqa: E402
import shuffle_ref as sr  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

L = bp.L
KS = [2, 3, 5, 6, 9]
GOLDEN = Path(__file__).resolve().parent / "golden" / "deck.json"


def with_V(pf, V):
    return bp.PermProof(V, pf.A_I, pf.A_O, pf.S, pf.T, pf.tau_x, pf.mu, pf.t_hat, pf.ipa)


@pytest.mark.parametrize("k", KS)
def test_circuit_shape(k):
    C = dr.deck_circuit(k)
    assert (C.n, C.Q, C.m) == (k - 1, 2 * k, k + 1)
    assert C.n_p == {2: 4, 3: 4, 5: 4, 6: 8, 9: 8}[k]
    assert dr.deck_circuit(52).n_p == 64 and dr.deck_proof_len(52) == 800


@pytest.mark.parametrize("k", KS + [52])
def test_witness_satisfies_every_row(k):
    """Every permutation tried satisfies all Q rows; one output card changed
    violates row 2k - 2 (a_O[k-2] = D) and nothing else."""
    C = dr.deck_circuit(k)
    x = sr.rand_scalar(b"deck-x-%d" % k)
    for i, deck in enumerate(sr.edge_decks(k) + [dr.default_deck(k)]):
        perm = sr.rand_perm(k, b"deck-w-%d-%d" % (k, i))
        v, aL, aR, aO = dr.deck_witness(deck, perm, x)
        assert not dr.check_deck_constraints(C, deck, v, aL, aR, aO, x)
        out = [deck[p] for p in perm]
        out[k - 1] = (out[k - 1] + 1) % L  # no longer a permutation of the deck
        v2, aL2, aR2, aO2 = dr.deck_witness(out, list(range(k)), x)
        assert dr.check_deck_constraints(C, deck, v2, aL2, aR2, aO2, x) == [2 * k - 2]


@pytest.mark.parametrize("k", KS)
def test_prove_verify_and_reject(k):
    deck = sr.edge_decks(k)[0]
    perm = sr.rand_perm(k, b"deck-p-%d" % k)
    gam = [sr.rand_scalar(b"deck-g-%d-%d" % (k, j)) for j in range(k)]
    pf = dr.prove_deck(deck, perm, sr.seed32(b"deck-%d" % k), gam)
    assert len(pf.V) == k + 1 and len(pf.to_bytes()) == dr.deck_proof_len(k)
    assert dr.verify_deck(deck, pf)
    other = list(deck)
    other[k - 1] = (other[k - 1] + 1) % L  # one card of the deck changed
    assert not dr.verify_deck(other, pf)
    assert not dr.verify_deck(deck, pf, label=b"another")
    # V_0 replaced by V_1 (V_1 twice): the committed values are no longer the deck's multiset
    assert pf.V[0] != pf.V[1]
    assert not dr.verify_deck(deck, with_V(pf, [pf.V[1]] + pf.V[1:]))
    # a permutation of the commitments IS still a shuffle of the deck, but not this proof's
    sw = list(pf.V)
    sw[0], sw[1] = sw[1], sw[0]
    assert not dr.verify_deck(deck, with_V(pf, sw))
    # drawn blindings and the default deck
    pf2 = dr.prove_deck(None, perm, 7)
    assert dr.verify_deck(dr.default_deck(k), pf2)


def test_same_shape_as_a_two_half_proof_but_separate():
    """k' = 3 two-half and k = 6 deck: the same m, n_p and byte length; the
    "deck" transcript message keeps one from verifying as the other."""
    two, _ = bp.ac_prove(3, 5)
    assert bp.ac_verify(3, two)
    deck = dr.default_deck(6)
    pf = dr.prove_deck(deck, sr.rand_perm(6, b"sep"), 5)
    assert dr.verify_deck(deck, pf)
    C2, C6 = bp.perm_circuit(3), dr.deck_circuit(6)
    assert (C2.m, C2.n_p) == (C6.m, C6.n_p) == (7, 8)
    assert len(two.to_bytes()) == len(pf.to_bytes()) and len(two.V) == len(pf.V)
    assert not dr.verify_deck(deck, two)
    assert not bp.ac_verify(3, pf)


def test_golden_file_is_the_helpers():
    """tests/golden/deck.json: the k = 9 case regenerated here equals the file;
    the k = 52 proofs have the documented sizes."""
    cases = json.loads(GOLDEN.read_text())["cases"]
    assert [(c["k"], len(c["proofs"])) for c in cases] == [(52, 2), (9, 1)]
    c52, c9 = cases
    assert c52["deck"] is None and all(len(p) == 2 * 800 for p in c52["proofs"])
    assert all(len(v) == 53 for v in c52["V"])
    deck = [int.from_bytes(bytes.fromhex(h), "little") for h in c9["deck"]]
    gam = [int.from_bytes(bytes.fromhex(h), "little") for h in c9["gammas"][0]]
    pf = dr.prove_deck(deck, c9["perms"][0], bytes.fromhex(c9["seeds"][0]), gam, label=c9["label"].encode())
    assert pf.to_bytes().hex() == c9["proofs"][0] and [v.hex() for v in pf.V] == c9["V"][0]


# ------------------------------------------------------------------ the C ABI
def _lib():
    from bpperm import _lib as L_
    return ctypes.CDLL(str(L_.LIB_PATH))


def test_deck_proof_len():
    lib = _lib()
    f, g = lib.bpp_deck_proof_len, lib.bpp_perm_proof_len
    f.restype = g.restype = ctypes.c_size_t
    assert f(ctypes.c_uint32(1)) == 0 and f(ctypes.c_uint32((1 << 20) + 1)) == 0 and f(ctypes.c_uint32(0)) == 0
    assert f(ctypes.c_uint32(52)) == 800
    assert f(ctypes.c_uint32(6)) == g(ctypes.c_uint32(3))
    for k in (2, 3, 5, 6, 9, 10, 17, 18, 65, 66, 1 << 20):
        assert f(ctypes.c_uint32(k)) == dr.deck_proof_len(k), k


def test_deck_argument_checks_without_device():
    """bpp_deck_prove_batch checks its witness before any device call and before
    it writes an output byte: a perm that is not a bijection -> BPP_ERR_ARG (1)
    before anything else, a deck card or blinding >= l -> BPP_ERR_NONCANONICAL
    (4), then a null context -> BPP_ERR_ARG.  The verifiers refuse a
    non-canonical deck card too."""
    lib = _lib()
    fn = lib.bpp_deck_prove_batch
    fn.restype = ctypes.c_int
    ARG, NONCANON = 1, 4
    k, count = 4, 2
    good_deck = b"".join(sr.scalar_bytes(c) for c in [3, 0, L - 1, 3])
    bad_deck = good_deck[:64] + L.to_bytes(32, "little") + good_deck[96:]
    good_perm = [2, 0, 3, 1, 0, 1, 2, 3]
    bad_perm = [2, 0, 3, 1, 0, 1, 1, 3]
    good_gam = b"".join(sr.scalar_bytes(sr.rand_scalar(b"dg%d" % j)) for j in range(count * k))
    fill = b"\xa5" * 4096

    def call(kk, deck, perm, gammas):
        pf = ctypes.create_string_buffer(fill, len(fill))
        V = ctypes.create_string_buffer(fill, len(fill))
        pm = (ctypes.c_uint32 * len(perm))(*perm)
        rc = fn(None, None, ctypes.c_uint32(kk), ctypes.c_size_t(count), ctypes.c_char_p(deck) if deck else None, pm,
                ctypes.c_char_p(gammas) if gammas is not None else None, None, None, ctypes.c_size_t(0), pf, V)
        assert pf.raw == fill and V.raw == fill, "outputs written on a refused call"
        return rc

    assert call(k, good_deck, good_perm, None) == ARG      # a valid witness, no context
    assert call(k, None, good_perm, good_gam) == ARG
    for kk in (0, 1, (1 << 20) + 1):
        assert call(kk, good_deck, good_perm, None) == ARG
    assert call(k, good_deck, bad_perm, None) == ARG
    assert call(k, bad_deck, bad_perm, None) == ARG         # the perm before the deck
    assert call(k, good_deck, [2, 0, 3, 1, 0, 1, 2, 0xFFFFFFFF], None) == ARG
    assert call(k, bad_deck, good_perm, None) == NONCANON
    assert call(k, b"\xff" * 128, good_perm, None) == NONCANON
    badg = bytearray(good_gam)
    badg[32 * 5: 32 * 6] = L.to_bytes(32, "little")
    assert call(k, good_deck, good_perm, bytes(badg)) == NONCANON
    pf = ctypes.create_string_buffer(64)
    assert fn(None, None, ctypes.c_uint32(k), ctypes.c_size_t(1), None, None, None, None, None, ctypes.c_size_t(0),
              pf, pf) == ARG
    # verifiers: null context first (ARG), as their two-half counterparts
    for name in ("bpp_deck_verify_batch", "bpp_deck_verify_batch_each"):
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        assert f(None, None, ctypes.c_uint32(k), ctypes.c_size_t(0), None, None, ctypes.c_size_t(0), None, None,
                 None) == ARG


def test_python_wrapper_names_the_entries():
    import bpperm
    from bpperm import _lib as L_
    for name in ("bpp_deck_proof_len", "bpp_deck_prove_batch", "bpp_deck_verify", "bpp_deck_verify_batch",
                 "bpp_deck_verify_batch_each"):
        assert name in L_.SIGNATURES
    for meth in ("prove_batch", "verify", "verify_batch", "verify_batch_each"):
        assert callable(getattr(bpperm.DeckProver, meth))
