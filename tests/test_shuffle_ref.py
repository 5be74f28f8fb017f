"""Caller-supplied shuffles without a GPU: the reference helper
(tests/shuffle_ref.py) is pinned to the oracle's ac_prove, its proofs over
custom decks verify with the oracle's ac_verify, and
bpp_perm_prove_shuffle_batch refuses a bad witness before any device work."""
import ctypes
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import shuffle_ref as sr  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402
from oracle.merlin import Rng  # noqa: E402

L = bp.L


@pytest.mark.parametrize("k,seed", [(2, 1), (5, 4), (5, sr.seed32(b"pin"))], ids=["k2-u64", "k5-u64", "k5-seed32"])
def test_helper_equals_oracle_on_the_seeded_witness(k, seed):
    """cards = 1..k, perm = fisher_yates(seed), gammas = None: ac_prove's
    exact bytes (u64 test seeds and a 32-byte entropy seed)."""
    want, perm = bp.ac_prove(k, seed)
    assert perm == bp.fisher_yates(k, Rng(seed, b"bpperm-prove"))
    got = sr.prove_shuffle(list(range(1, k + 1)), perm, seed)
    assert got.V == want.V
    assert got.to_bytes() == want.to_bytes()


@pytest.mark.parametrize("k", [2, 3, 5])
def test_helper_proofs_over_custom_decks_verify(k):
    """0, l - 1, repeated and 252-bit cards, drawn and supplied blindings:
    the oracle's verifier accepts, and rejects the proof once two output
    commitments are swapped or paired with another deck's V."""
    proofs = []
    for i, deck in enumerate(sr.edge_decks(k)):
        perm = sr.rand_perm(k, b"cpu-%d-%d" % (k, i))
        gam = [sr.rand_scalar(b"gam-%d-%d-%d" % (k, i, j)) for j in range(2 * k)] if i != 1 else None
        pf = sr.prove_shuffle(deck, perm, sr.seed32(b"cpu-%d-%d" % (k, i)), gam)
        assert bp.ac_verify(k, pf)
        proofs.append(pf)
    a, b = proofs[0], proofs[1]
    assert a.V[k] != a.V[k + 1]
    sw = list(a.V)
    sw[k], sw[k + 1] = sw[k + 1], sw[k]
    assert not bp.ac_verify(k, bp.PermProof(sw, a.A_I, a.A_O, a.S, a.T, a.tau_x, a.mu, a.t_hat, a.ipa))
    assert not bp.ac_verify(k, bp.PermProof(b.V, a.A_I, a.A_O, a.S, a.T, a.tau_x, a.mu, a.t_hat, a.ipa))


def test_helper_witness_is_checked_by_the_oracle_constraints():
    """The generalised witness satisfies the oracle's circuit for a true
    shuffle and violates it when the output is not a permutation of the deck."""
    k, x = 5, sr.rand_scalar(b"x")
    deck = sr.edge_decks(k)[0]
    perm = sr.rand_perm(k, b"w")
    C = bp.perm_circuit(k)
    v, aL, aR, aO = sr.perm_witness(deck, perm, x)
    assert not bp.check_constraints(C, v, aL, aR, aO, x)
    v2 = list(v)
    v2[k + 2] = (v2[k + 2] + 1) % L  # one output card changed: a_R of its gate no longer matches
    assert bp.check_constraints(C, v2, aL, aR, aO, x)


def test_shuffle_argument_checks_without_device():
    """bpp_perm_prove_shuffle_batch checks its witness and arguments before
    any device call and before it writes an output byte: a null context ->
    BPP_ERR_ARG (1), a perm that is not a bijection -> BPP_ERR_ARG, a card or
    blinding >= l -> BPP_ERR_NONCANONICAL (4), k out of range -> BPP_ERR_ARG."""
    from bpperm import _lib
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    fn = lib.bpp_perm_prove_shuffle_batch
    fn.restype = ctypes.c_int
    ARG, NONCANON = 1, 4
    k, count = 4, 2
    good_cards = b"".join(sr.scalar_bytes(c) for c in [3, 0, L - 1, 3, 9, 8, 7, 6])
    good_perm = [2, 0, 3, 1, 0, 1, 2, 3]
    good_gam = b"".join(sr.scalar_bytes(sr.rand_scalar(b"g%d" % j)) for j in range(count * 2 * k))
    fill = b"\xa5" * 4096

    def call(kk, cards, perm, gammas, ctx=None, gens=None):
        pf = ctypes.create_string_buffer(fill, len(fill))
        V = ctypes.create_string_buffer(fill, len(fill))
        pm = (ctypes.c_uint32 * len(perm))(*perm)
        rc = fn(ctx, gens, ctypes.c_uint32(kk), ctypes.c_size_t(count), ctypes.c_char_p(cards), pm,
                ctypes.c_char_p(gammas) if gammas is not None else None, None, None, ctypes.c_size_t(0), pf, V)
        assert pf.raw == fill and V.raw == fill, "outputs written on a refused call"
        return rc

    # a valid witness, no context
    assert call(k, good_cards, good_perm, None) == ARG
    assert call(k, good_cards, good_perm, good_gam) == ARG
    for kk in (0, 1, (1 << 20) + 1):
        assert call(kk, good_cards, good_perm, None) == ARG
    # not a bijection: a repeated index, an index out of range (second proof)
    assert call(k, good_cards, [2, 0, 3, 1, 0, 1, 1, 3], None) == ARG
    assert call(k, good_cards, [2, 0, 3, 1, 0, 1, 2, 4], None) == ARG
    assert call(k, good_cards, [2, 0, 3, 1, 0, 1, 2, 0xFFFFFFFF], None) == ARG
    # non-canonical: a card = l, a card = 2^256 - 1, a blinding = l
    for badv in (L, (1 << 256) - 1):
        bad = bytearray(good_cards)
        bad[32 * 5: 32 * 6] = badv.to_bytes(32, "little")
        assert call(k, bytes(bad), good_perm, None) == NONCANON
    badg = bytearray(good_gam)
    badg[32 * 11: 32 * 12] = L.to_bytes(32, "little")
    assert call(k, good_cards, good_perm, bytes(badg)) == NONCANON
    # null witness arrays
    pf = ctypes.create_string_buffer(64)
    assert fn(None, None, ctypes.c_uint32(k), ctypes.c_size_t(1), None, None, None, None, None, ctypes.c_size_t(0),
              pf, pf) == ARG


def test_python_wrapper_names_the_entry():
    import bpperm
    from bpperm import _lib
    assert "bpp_perm_prove_shuffle_batch" in _lib.SIGNATURES
    assert callable(bpperm.PermProver.prove_shuffle_batch)
