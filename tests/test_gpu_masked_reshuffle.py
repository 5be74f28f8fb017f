"""bpp_masked_reshuffle_* on the GPU: output cards and proofs byte-exact against
the reference helper (tests/masked_reshuffle_ref.py) and the committed fixtures,
batches across a wave boundary, the edge inputs, every region bound, every
refusal by name, per-proof verdicts (a card whose halves were re-masked under
two different scalars among them), a three-player chain from the open deck that
the key's discrete log unmasks, and the batch's secrets wiped with the plain
re-shuffle still exact in the same process, every refusal's text, and a batch
one proof longer than a launch sequence takes."""
import ctypes
import json
import random
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import masked_reshuffle_ref as mr  # noqa: E402
from oracle import ristretto as r255  # noqa: E402

pytestmark = pytest.mark.gpu
L = mr.L
GOLDEN = json.loads((HERE / "golden" / "masked_reshuffle.json").read_text())["cases"]
ARG, LEN, DECOMPRESS, NONCANONICAL, VERIFY = 1, 2, 3, 4, 6
UNDECODABLE = b"\xff" * 32
K_TEXT = "reshuffle: k > 342 (the inner circuit's 2k - 2 gates pass the plain bound of 682)"
KEY_TEXT = "masked reshuffle: the key does not decode"


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


def split(joined: bytes):
    """The k 64-byte cards of a shuffle's joined output."""
    return [joined[64 * i:64 * i + 64] for i in range(len(joined) // 64)]


def bump(pf: bytes, at: int) -> bytes:
    return pf[:at] + mr.sb(int.from_bytes(pf[at:at + 32], "little") + 1) + pf[at + 32:]


_REF = {}


def reference(k):
    """Three reference shuffles at k cards under one key (the third with
    supplied blinds, 0 and l - 1 among them), computed once."""
    if k not in _REF:
        key, rows = mr.rand_point(b"gm-key-%d" % k), []
        for i in range(3):
            tag = b"gm-%d-%d" % (k, i)
            cards, perm, seed = mr.rand_cards(k, tag), mr.rand_perm(k, tag), mr.seed32(tag)
            blinds = None
            if i == 2:
                blinds = [mr.rand_scalar(tag + b"-r%d" % j) for j in range(k)]
                blinds[0], blinds[-1] = 0, L - 1
            out, pf = mr.prove(key, cards, perm, seed, blinds)
            rows.append((cards, perm, seed, blinds, out, pf))
        _REF[k] = (key, rows)
    return _REF[k]


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 5, 9])
def test_bit_exact_vs_reference(gens, k, count):
    """k = 2: the n_p floor of 4; k = 3 and 5: on both sides of a padding step;
    k = 9: 16 gates, no padding gate.  count = 1 draws its r_i, count = 3 is
    given them.  cards_out and proofs equal the reference's bytes; the three
    verifiers accept."""
    import bpperm
    key, rows = reference(k)
    ms = bpperm.MaskedReshuffler(gens, k, key)
    assert ms.proof_len == mr.proof_len(k) == bpperm.Reshuffler(gens, k).proof_len + 32
    if count == 1:
        cards, perm, seed, _, out, pf = rows[0]
        got_out, got_pf = ms.shuffle_batch([cards], [perm], seeds32=seed)
        assert got_out == [b"".join(out)] and got_pf == [pf]
        assert ms.verify(cards, out, pf)
        return
    blinds = [[mr.sb(b) for b in (r[3] if r[3] else mr.draws(r[2], k)[0])] for r in rows]
    got_out, got_pf = ms.shuffle_batch([r[0] for r in rows], [r[1] for r in rows], blinds=blinds,
                                       seeds32=b"".join(r[2] for r in rows))
    for i, r in enumerate(rows):
        assert got_out[i] == b"".join(r[4]), i
        assert got_pf[i] == r[5], i
        assert ms.verify(r[0], r[4], r[5])
    assert ms.verify_batch([r[0] for r in rows], [r[4] for r in rows], got_pf)
    assert ms.verify_batch_each([r[0] for r in rows], [r[4] for r in rows], got_pf) == [True] * 3


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: "k%d" % c["k"])
def test_golden(gens, case):
    """The committed proofs (k = 52 among them) verify, and the prover
    reproduces them from their seeds."""
    import bpperm
    k, key = case["k"], bytes.fromhex(case["key"])
    ci = [bytes.fromhex(h) for h in case["cards_in"]]
    co = [bytes.fromhex(h) for h in case["cards_out"]]
    pf = bytes.fromhex(case["proof"])
    assert len(pf) == mr.proof_len(k)
    ms = bpperm.MaskedReshuffler(gens, k, key, label=case["label"].encode())
    assert ms.verify(ci, co, pf)
    blinds = [[bytes.fromhex(h) for h in case["blinds"]]] if case["blinds"] else None
    out, proofs = ms.shuffle_batch([ci], [case["perm"]], blinds=blinds, seeds32=bytes.fromhex(case["seed"]))
    assert out == [b"".join(co)] and proofs == [pf]
    assert not bpperm.MaskedReshuffler(gens, k, key, label=b"another label").verify(ci, co, pf)


@pytest.mark.parametrize("count", [65, 130])
def test_batches_across_a_wave_boundary(gens, count):
    """k = 4: 260 and 520 card lanes, 520 and 1040 table rows, 65 and 130 Merlin
    lanes.  All verify on the GPU in one batch; proofs 0, 64 and the last also
    in the reference."""
    import bpperm
    k, key = 4, mr.rand_point(b"wave-key")
    cards = [mr.rand_cards(k, b"wave-%d" % p) for p in range(count)]
    perms = [mr.rand_perm(k, b"wave-%d" % p) for p in range(count)]
    seeds = b"".join(mr.seed32(b"wave-%d" % p) for p in range(count))
    ms = bpperm.MaskedReshuffler(gens, k, key)
    out, proofs = ms.shuffle_batch(cards, perms, seeds32=seeds)
    assert ms.verify_batch(cards, out, proofs)
    assert ms.verify_batch_each(cards, out, proofs) == [True] * count
    for p in (0, 64, count - 1):
        assert mr.verify(key, cards[p], split(out[p]), proofs[p]), p
        assert ms.verify(cards[p], split(out[p]), proofs[p])


@pytest.mark.parametrize("name", mr.EDGES)
def test_edge_inputs(gens, name):
    """The open deck, a card (identity, identity), two equal cards, supplied
    blinds with a zero, pi the identity and the reversal, K the identity: bytes
    equal the reference's."""
    import bpperm
    k = 5
    key, cards, perm, blinds = mr.edge_case(k, name)
    seed = mr.seed32(b"edge-%d" % k)
    want_out, want_pf = mr.prove(key, cards, perm, seed, blinds)
    ms = bpperm.MaskedReshuffler(gens, k, key)
    out, proofs = ms.shuffle_batch([cards], [perm], blinds=[[mr.sb(b) for b in blinds]] if blinds else None,
                                   seeds32=seed)
    assert out == [b"".join(want_out)] and proofs == [want_pf]
    assert ms.verify(cards, want_out, want_pf)


@pytest.fixture(scope="module")
def one(gens):
    """One valid shuffle at k = 3, its MaskedReshuffler and the regions of its proof."""
    import bpperm
    key, rows = reference(3)
    cards, perm, seed, _, out, pf = rows[0]
    return bpperm.MaskedReshuffler(gens, 3, key), cards, out, pf, {name: off for name, off, _ in mr.regions(3)}


def code_of(ms, cards, out, pf):
    import bpperm
    try:
        return 0 if ms.verify(cards, out, pf) else VERIFY
    except bpperm.BppError as e:
        return e.code


@pytest.mark.parametrize("region", ["A", "E", "Ti", "TU", "TW", "z", "om", "zR", "Vk", "inner"])
def test_each_region_tampered_is_a_verification_error(one, region):
    ms, cards, out, pf, o = one
    at = o[region]
    if region in ("z", "om", "zR"):
        bad = bump(pf, at)
    elif region == "inner":
        bad = bump(pf, at + 8 * 32)  # tau_x
    else:
        bad = pf[:at] + mr.rand_point(b"gpu-other-" + region.encode()) + pf[at + 32:]
    assert not mr.verify(ms.key, cards, out, bad)
    assert code_of(ms, cards, out, bad) == VERIFY
    assert not ms.verify_batch([cards], [out], [bad])
    assert ms.verify_batch_each([cards, cards], [out, out], [pf, bad]) == [True, False]


def test_refusals_by_name(gens, one):
    import bpperm
    ms, cards, out, pf, o = one
    key, perm, seed = ms.key, reference(3)[1][0][1], reference(3)[1][0][2]

    def prove_code(m, cards, perm, blinds=None):
        try:
            m.shuffle_batch([cards], [perm], blinds=blinds, seeds32=mr.seed32(b"x"))
            return 0
        except bpperm.BppError as e:
            return e.code

    # the prover: no bijection, a blind >= l, an undecodable key, an undecodable half of an input card
    assert prove_code(ms, cards, [0, 0, 1]) == ARG
    assert prove_code(ms, cards, [0, 1, 3]) == ARG
    assert prove_code(ms, cards, perm, [[mr.sb(1), L.to_bytes(32, "little"), mr.sb(2)]]) == NONCANONICAL
    assert prove_code(ms, cards, [0, 0, 1], [[mr.sb(1), L.to_bytes(32, "little"), mr.sb(2)]]) == ARG  # (in this order)
    assert prove_code(bpperm.MaskedReshuffler(gens, 3, UNDECODABLE), cards, perm) == DECOMPRESS
    assert prove_code(ms, [UNDECODABLE + cards[0][32:]] + cards[1:], perm) == DECOMPRESS
    assert prove_code(ms, cards[:2] + [cards[2][:32] + UNDECODABLE], perm) == DECOMPRESS
    # the verifier: an undecodable key, card half and proof point; z = l; a short proof
    assert code_of(bpperm.MaskedReshuffler(gens, 3, UNDECODABLE), cards, out, pf) == DECOMPRESS
    assert code_of(ms, cards, [out[0][:32] + UNDECODABLE] + out[1:], pf) == DECOMPRESS
    assert code_of(ms, cards, out, pf[:o["E"] + 32] + UNDECODABLE + pf[o["E"] + 64:]) == DECOMPRESS  # E_1
    assert code_of(ms, cards, out, pf[:o["TU"]] + UNDECODABLE + pf[o["TU"] + 32:]) == DECOMPRESS
    assert code_of(ms, cards, out, pf[:o["z"]] + L.to_bytes(32, "little") + pf[o["z"] + 32:]) == NONCANONICAL
    assert code_of(ms, cards, out, pf[:-32]) == VERIFY
    with pytest.raises(bpperm.BppError) as e:  # the batch verdict names the refusal
        ms.verify_batch([cards, cards], [out, [UNDECODABLE + out[0][32:]] + out[1:]], [pf, pf])
    assert e.value.code == DECOMPRESS
    # _each: a proof with an undecodable point fails alone, an undecodable key refuses the call
    bad_tw = pf[:o["TW"]] + UNDECODABLE + pf[o["TW"] + 32:]
    assert ms.verify_batch_each([cards] * 4, [out, [out[0][:32] + UNDECODABLE] + out[1:], out, out],
                                [pf, pf, pf, bad_tw]) == [True, False, True, False]
    with pytest.raises(bpperm.BppError) as e:
        bpperm.MaskedReshuffler(gens, 3, UNDECODABLE).verify_batch_each([cards], [out], [pf])
    assert e.value.code == DECOMPRESS
    # swapped cards, swapped halves, another key
    assert code_of(ms, [cards[1], cards[0], cards[2]], out, pf) == VERIFY
    assert code_of(ms, cards, [out[1], out[0], out[2]], pf) == VERIFY
    assert code_of(ms, cards, [out[0][32:] + out[0][:32]] + out[1:], pf) == VERIFY
    assert code_of(bpperm.MaskedReshuffler(gens, 3, mr.rand_point(b"another key")), cards, out, pf) == VERIFY
    # k = 1 and k = 343, on both sides; no proofs
    lib, buf = ms.ctx.lib, bytes(343 * 64)
    ident = (ctypes.c_uint32 * 343)(*range(343))
    sink = ctypes.create_string_buffer(343 * 64)
    assert lib.bpp_masked_reshuffle_proof_len(1) == 0 and lib.bpp_masked_reshuffle_proof_len(343) == 0
    assert lib.bpp_masked_reshuffle_proof_len(342) > 0
    for k, code in ((1, ARG), (343, LEN)):
        assert lib.bpp_masked_reshuffle_verify(ms.ctx.h, gens.h, k, key, b"bp-perm", 7, buf, buf, buf, 32) == code
        assert lib.bpp_masked_reshuffle_prove_batch(ms.ctx.h, gens.h, k, 1, key, buf, ident, None, seed, b"bp-perm", 7,
                                                    sink, sink) == code
    assert sink.raw == bytes(343 * 64)  # (no output byte)
    assert ms.verify_batch([], [], []) and ms.verify_batch_each([], [], []) == []
    assert ms.shuffle_batch([], []) == ([], [])


def test_verify_batch_each_names_the_failing_proofs(gens):
    """8 proofs at k = 4.  Proof 1: z_1 + 1.  Proof 3: U'_0 re-masked with r, W'_0
    with r + 1, forced through the reference prover.  Proof 4: the inner proof's
    t_hat + 1.  Proof 6: an undecodable T_W.  Exactly those four fail, and the
    error text counts them."""
    import bpperm
    k, count = 4, 8
    key = mr.rand_point(b"each-key")
    cards = [mr.rand_cards(k, b"each-%d" % p) for p in range(count)]
    perms = [mr.rand_perm(k, b"each-%d" % p) for p in range(count)]
    seeds = [mr.seed32(b"each-%d" % p) for p in range(count)]
    ms = bpperm.MaskedReshuffler(gens, k, key)
    out, proofs = ms.shuffle_batch(cards, perms, seeds32=b"".join(seeds))
    assert ms.verify_batch_each(cards, out, proofs) == [True] * count
    o = {name: off for name, off, _ in mr.regions(k)}
    bad, bad_out = list(proofs), list(out)
    bad[1] = bump(bad[1], o["z"] + 32)
    co = split(out[3])
    moved = [co[0][:32] + r255.encode(r255.ed_add(r255.decode(co[0][32:]), r255.decode(key)))] + co[1:]
    _, bad[3] = mr.prove(key, cards[3], perms[3], seeds[3], cards_out=moved)
    bad_out[3] = b"".join(moved)
    bad[4] = bump(bad[4], o["inner"] + 10 * 32)
    bad[6] = bad[6][:o["TW"]] + UNDECODABLE + bad[6][o["TW"] + 32:]
    ok = ctypes.create_string_buffer(b"\x01" * count, count)
    rc = ms.ctx.lib.bpp_masked_reshuffle_verify_batch_each(ms.ctx.h, gens.h, k, count, key, b"bp-perm", 7,
                                                           b"".join(b"".join(c) for c in cards), b"".join(bad_out),
                                                           b"".join(bad), ok)
    text = (ms.ctx.lib.bpp_ctx_last_error(ms.ctx.h) or b"").decode()
    assert rc == VERIFY
    assert list(ok.raw) == [1, 0, 1, 0, 0, 1, 0, 1]
    assert text.endswith("4 of 8 proofs failed, the first at index 1"), text
    assert ms.verify_batch_each(cards, bad_out, bad) == [True, False, True, False, False, True, False, True]
    assert mr.verify_parts(key, cards[1], split(out[1]), bad[1]) == (False, False, False, True)
    assert mr.verify_parts(key, cards[3], moved, bad[3]) == (True, True, False, True)
    assert mr.verify_parts(key, cards[4], split(out[4]), bad[4]) == (True, True, True, False)
    # without the undecodable point the batch verdict is a plain failure
    assert not ms.verify_batch(cards[:6], bad_out[:6], bad[:6])


def test_three_players_shuffle_the_open_deck(gens):
    """Three players with key shares sk_j shuffle the open deck (identity, M_j)
    at k = 5 in turn under K = (sk_1 + sk_2 + sk_3) B: every step verifies, a
    step checked under another key fails, and the sum of the shares unmasks
    the final cards to the composed permutation of the deck."""
    import bpperm
    k = 5
    sks = [mr.rand_scalar(b"gchain-sk%d" % j) for j in range(3)]
    key = mr.key_of(sum(sks))
    M = [mr.rand_point(b"gchain-M%d" % j) for j in range(k)]
    ms = bpperm.MaskedReshuffler(gens, k, key, label=b"chain")
    wrong = bpperm.MaskedReshuffler(gens, k, mr.key_of(sks[0]), label=b"chain")
    cards, src = mr.open_deck(M), list(range(k))
    for s in range(3):
        perm = mr.rand_perm(k, b"gchain-%d" % s)
        out, proofs = ms.shuffle_batch([cards], [perm])  # (the OS CSPRNG's seed)
        nxt = split(out[0])
        assert ms.verify(cards, nxt, proofs[0])
        assert not wrong.verify(cards, nxt, proofs[0])
        assert not ms.verify(nxt, cards, proofs[0])
        src = [src[perm[i]] for i in range(k)]
        cards = nxt
    assert sorted(src) == list(range(k))
    assert mr.unmask(cards, sum(sks)) == [M[j] for j in src]


def test_secrets_are_wiped_and_the_plain_reshuffle_is_unmoved(gens, ctx):
    """The two provers share their workspaces: after a masked batch nothing
    secret is left, and the plain Reshuffler still reproduces its committed
    proofs in the same process (and the masked one after it)."""
    import bpperm
    k = 5
    key = mr.rand_point(b"wipe-key")
    ms = bpperm.MaskedReshuffler(gens, k, key)
    cards = [mr.rand_cards(k, b"wipe-%d" % p) for p in range(3)]
    perms = [mr.rand_perm(k, b"wipe-%d" % p) for p in range(3)]
    blinds = [[mr.sb(mr.rand_scalar(b"wipe-r%d-%d" % (p, i))) for i in range(k)] for p in range(3)]
    seeds = b"".join(mr.seed32(b"wipe-%d" % p) for p in range(3))
    first = ms.shuffle_batch(cards, perms, blinds=blinds, seeds32=seeds)
    assert ctx.secret_residue() == 0
    for case in json.loads((HERE / "golden" / "reshuffle.json").read_text())["cases"]:
        ci = [bytes.fromhex(h) for h in case["cards_in"]]
        rs = bpperm.Reshuffler(gens, case["k"], label=case["label"].encode())
        b = [[bytes.fromhex(h) for h in case["blinds"]]] if case["blinds"] else None
        out, proofs = rs.shuffle_batch([ci], [case["perm"]], blinds=b, seeds32=bytes.fromhex(case["seed"]))
        assert out == [bytes.fromhex("".join(case["cards_out"]))] and proofs == [bytes.fromhex(case["proof"])]
        assert rs.verify(ci, [bytes.fromhex(h) for h in case["cards_out"]], proofs[0])
    assert ctx.secret_residue() == 0
    assert ms.shuffle_batch(cards, perms, blinds=blinds, seeds32=seeds) == first
    assert ms.verify_batch(cards, first[0], first[1])
    assert ctx.secret_residue() == 0


def test_refusal_texts(gens, one):
    """k = 3, at most 3 proofs a call: what bpp_ctx_last_error ends with after
    each refusal, the proof's index (never 0 alone), the card's or point's and
    the card's half among them; the key's from the prover and the three
    verifiers."""
    import bpperm
    ms, cards, out, pf, o = one
    perm, seed = reference(3)[1][0][1], reference(3)[1][0][2]
    lib, bad = ms.ctx.lib, UNDECODABLE
    nokey = bpperm.MaskedReshuffler(gens, 3, UNDECODABLE)

    def text_of(code, f, *a, **kw):
        with pytest.raises(bpperm.BppError) as e:
            f(*a, **kw)
        assert e.value.code == code
        return (lib.bpp_ctx_last_error(ms.ctx.h) or b"").decode()

    def at(region, i=0):
        return pf[:o[region] + 32 * i] + bad + pf[o[region] + 32 * i + 32:]

    def verifier(code, q, ci=cards, co=out, proof=pf):  # three proofs, proof q as given
        cis, cos, pfs = [cards] * 3, [out] * 3, [pf] * 3
        cis[q], cos[q], pfs[q] = ci, co, proof
        return text_of(code, ms.verify_batch, cis, cos, pfs)

    bad_u, bad_w = bad + cards[1][32:], cards[2][:32] + bad
    # the key: the prover and the three verifiers
    assert text_of(DECOMPRESS, nokey.shuffle_batch, [cards], [perm], seeds32=seed).endswith(KEY_TEXT)
    assert text_of(DECOMPRESS, nokey.verify, cards, out, pf).endswith(KEY_TEXT)
    assert text_of(DECOMPRESS, nokey.verify_batch, [cards] * 2, [out] * 2, [pf] * 2).endswith(KEY_TEXT)
    assert text_of(DECOMPRESS, nokey.verify_batch_each, [cards] * 2, [out] * 2, [pf] * 2).endswith(KEY_TEXT)
    # the prover
    t = text_of(DECOMPRESS, ms.shuffle_batch, [cards, [cards[0], bad_u, cards[2]]], [perm, perm], seeds32=seed * 2)
    assert t.endswith("masked reshuffle 1: U of input card 1 does not decode"), t
    t = text_of(DECOMPRESS, ms.shuffle_batch, [cards, cards, cards[:2] + [bad_w]], [perm] * 3, seeds32=seed * 3)
    assert t.endswith("masked reshuffle 2: W of input card 2 does not decode"), t
    t = text_of(ARG, ms.shuffle_batch, [cards] * 3, [perm, perm, [0, 0, 1]], seeds32=seed * 3)
    assert t.endswith("masked reshuffle 2: perm is not a bijection on [0, k)"), t
    t = text_of(NONCANONICAL, ms.shuffle_batch, [cards] * 2, [perm] * 2, seeds32=seed * 2,
                blinds=[[mr.sb(1)] * 3, [mr.sb(1), L.to_bytes(32, "little"), mr.sb(2)]])
    assert t.endswith("masked reshuffle 1: non-canonical blind"), t
    # the verifier, one case per class of point
    t = verifier(DECOMPRESS, 1, ci=[cards[0], bad_u, cards[2]])
    assert t.endswith("masked reshuffle 1: U of input card 1 does not decode"), t
    t = verifier(DECOMPRESS, 2, ci=cards[:2] + [bad_w])
    assert t.endswith("masked reshuffle 2: W of input card 2 does not decode"), t
    t = verifier(DECOMPRESS, 2, co=[bad + out[0][32:]] + out[1:])
    assert t.endswith("masked reshuffle 2: U of output card 0 does not decode"), t
    t = verifier(DECOMPRESS, 1, co=[out[0], out[1][:32] + bad, out[2]])
    assert t.endswith("masked reshuffle 1: W of output card 1 does not decode"), t
    t = verifier(DECOMPRESS, 0, proof=at("A", 1))
    assert t.endswith("masked reshuffle 0: A 1 does not decode"), t
    t = verifier(DECOMPRESS, 2, proof=at("E", 0))
    assert t.endswith("masked reshuffle 2: E 0 does not decode"), t
    t = verifier(DECOMPRESS, 1, proof=at("Ti", 2))
    assert t.endswith("masked reshuffle 1: T 2 does not decode"), t
    t = verifier(DECOMPRESS, 2, proof=at("TU"))
    assert t.endswith("masked reshuffle 2: T_U does not decode"), t
    t = verifier(DECOMPRESS, 1, proof=at("TW"))
    assert t.endswith("masked reshuffle 1: T_W does not decode"), t
    t = verifier(NONCANONICAL, 2, proof=pf[:o["om"]] + L.to_bytes(32, "little") + pf[o["om"] + 32:])
    assert t.endswith("masked reshuffle 2: a response scalar is not canonical"), t
    # k = 343, on both sides: the blind re-shuffle's text
    buf, sink = bytes(343 * 64), ctypes.create_string_buffer(343 * 64)
    ident = (ctypes.c_uint32 * 343)(*range(343))
    assert lib.bpp_masked_reshuffle_prove_batch(ms.ctx.h, gens.h, 343, 1, ms.key, buf, ident, None, seed, b"bp-perm", 7,
                                                sink, sink) == LEN
    assert (lib.bpp_ctx_last_error(ms.ctx.h) or b"").decode().endswith(K_TEXT)
    assert lib.bpp_masked_reshuffle_verify(ms.ctx.h, gens.h, 343, ms.key, b"bp-perm", 7, buf, buf, buf, 32) == LEN
    assert (lib.bpp_ctx_last_error(ms.ctx.h) or b"").decode().endswith(K_TEXT)


def test_a_batch_across_a_chunk_boundary(ctx):
    """k = 342: a launch sequence takes 2^22 / (7k + 2) = 1750 proofs, so 1751
    shuffles of one open deck run as two.  The batch verifies; with z_0 + 1 in
    proofs 0, 1749 and 1750 exactly those three fail; an undecodable A_0 in
    proof 1750 alone refuses the batch and names that proof."""
    import bpperm
    k, chunk = 342, 1750
    count = chunk + 1
    assert chunk == (1 << 22) // (7 * k + 2)
    rnd = random.Random(343)
    g = bpperm.Gens(ctx, 1024)
    try:
        pts = g.pedersen_commit([mr.sb(10 + i) for i in range(k + 1)], [mr.sb(rnd.randrange(L)) for _ in range(k + 1)])
        ms = bpperm.MaskedReshuffler(g, k, pts[k])
        cin = b"".join(bytes(32) + m for m in pts[:k]) * count  # the open deck
        cout, proofs = ms.shuffle_batch(cin, [rnd.sample(range(k), k) for _ in range(count)],
                                        seeds32=rnd.randbytes(32 * count), raw=True)
        assert ms.verify_batch(cin, cout, proofs)
        pl, z0 = ms.proof_len, 32 * (3 * k + 2)
        bad = bytearray(proofs)
        for p in (0, chunk - 1, chunk):
            at = p * pl + z0
            bad[at:at + 32] = mr.sb(int.from_bytes(bad[at:at + 32], "little") + 1)
        ok = ctypes.create_string_buffer(count)
        rc = ctx.lib.bpp_masked_reshuffle_verify_batch_each(ctx.h, g.h, k, count, ms.key, b"bp-perm", 7, cin, cout,
                                                            bytes(bad), ok)
        text = (ctx.lib.bpp_ctx_last_error(ctx.h) or b"").decode()
        assert rc == VERIFY
        assert [p for p in range(count) if not ok.raw[p]] == [0, chunk - 1, chunk]
        assert text.endswith("3 of %d proofs failed, the first at index 0" % count), text
        bad = bytearray(proofs)
        bad[chunk * pl:chunk * pl + 32] = b"\xff" * 32
        with pytest.raises(bpperm.BppError) as e:
            ms.verify_batch(cin, cout, bytes(bad))
        assert e.value.code == DECOMPRESS
        assert str(e.value).endswith("masked reshuffle %d: A 0 does not decode" % chunk), str(e.value)
    finally:
        g.close()
