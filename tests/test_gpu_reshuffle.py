"""bpp_reshuffle_* on the GPU: output cards and proofs byte-exact against the
reference helper (tests/reshuffle_ref.py) and the committed fixtures, batches
across a wave boundary, the edge inputs, every refusal by name, per-proof
verdicts, a three-player chain over one committed deck, the batch's secrets wiped, every
refusal's text, and a batch one proof longer than a launch sequence takes."""
import ctypes
import json
import random
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import reshuffle_ref as rr  # noqa: E402
from oracle import ristretto as r255  # noqa: E402
from oracle.merlin import pedersen_gens_default  # noqa: E402

pytestmark = pytest.mark.gpu
L = rr.L
GOLDEN = json.loads((HERE / "golden" / "reshuffle.json").read_text())["cases"]
ARG, LEN, VERIFY, DECOMPRESS, NONCANONICAL = 1, 2, 6, 3, 4
K_TEXT = "reshuffle: k > 342 (the inner circuit's 2k - 2 gates pass the plain bound of 682)"


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


def other_point(tag: bytes) -> bytes:
    return rr.rand_cards(1, b"gpu-other-" + tag)[0]


_REF = {}


def reference(k):
    """Three reference shuffles at k cards (the third with supplied blinds, 0
    and l - 1 among them), computed once."""
    if k not in _REF:
        rows = []
        for i in range(3):
            tag = b"gr-%d-%d" % (k, i)
            cards, perm, seed = rr.rand_cards(k, tag), rr.rand_perm(k, tag), rr.seed32(tag)
            blinds = None
            if i == 2:
                blinds = [rr.rand_scalar(tag + b"-r%d" % j) for j in range(k)]
                blinds[0], blinds[-1] = 0, L - 1
            out, pf = rr.prove(cards, perm, seed, blinds)
            rows.append((cards, perm, seed, blinds, out, pf))
        _REF[k] = rows
    return _REF[k]


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 5, 9])
def test_bit_exact_vs_reference(gens, k, count):
    """k = 2: the n_p floor of 4; k = 3 and 5: non-powers of two on both sides
    of a padding step; k = 9: 16 gates, no padding gate.  cards_out and proofs
    equal the reference's bytes; the three verifiers accept."""
    import bpperm
    rows = reference(k)
    rs = bpperm.Reshuffler(gens, k)
    assert rs.proof_len == rr.proof_len(k)
    if count == 1:
        cards, perm, seed, _, out, pf = rows[0]
        got_out, got_pf = rs.shuffle_batch([cards], [perm], seeds32=seed)
        assert got_out == [b"".join(out)] and got_pf == [pf]
        assert rs.verify(cards, out, pf)
        return
    # all three with supplied blinds: the third's own, the others' their draws
    blinds = [[rr.sb(b) for b in (r[3] if r[3] else rr.draws(r[2], k)[0])] for r in rows]
    got_out, got_pf = rs.shuffle_batch([r[0] for r in rows], [r[1] for r in rows], blinds=blinds,
                                       seeds32=b"".join(r[2] for r in rows))
    for i, r in enumerate(rows):
        assert got_out[i] == b"".join(r[4]), i
        assert got_pf[i] == r[5], i
        assert rs.verify(r[0], r[4], r[5])
    assert rs.verify_batch([r[0] for r in rows], [r[4] for r in rows], got_pf)
    assert rs.verify_batch_each([r[0] for r in rows], [r[4] for r in rows], got_pf) == [True] * 3


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: "k%d" % c["k"])
def test_golden(gens, case):
    """The committed proofs (k = 52 among them) verify, and the prover
    reproduces them from their seeds."""
    import bpperm
    k = case["k"]
    ci = [bytes.fromhex(h) for h in case["cards_in"]]
    co = [bytes.fromhex(h) for h in case["cards_out"]]
    pf = bytes.fromhex(case["proof"])
    rs = bpperm.Reshuffler(gens, k, label=case["label"].encode())
    assert rs.verify(ci, co, pf)
    blinds = [[bytes.fromhex(h) for h in case["blinds"]]] if case["blinds"] else None
    out, proofs = rs.shuffle_batch([ci], [case["perm"]], blinds=blinds, seeds32=bytes.fromhex(case["seed"]))
    assert out == [b"".join(co)] and proofs == [pf]
    assert not bpperm.Reshuffler(gens, k, label=b"another label").verify(ci, co, pf)


@pytest.mark.parametrize("count", [65, 130])
def test_batches_across_a_wave_boundary(gens, count):
    """k = 4: 260 and 520 card lanes, 65 and 130 Merlin lanes.  All verify on
    the GPU; proofs 0, 64 and the last also in the reference."""
    import bpperm
    k = 4
    cards = [rr.rand_cards(k, b"wave-%d" % p) for p in range(count)]
    perms = [rr.rand_perm(k, b"wave-%d" % p) for p in range(count)]
    seeds = b"".join(rr.seed32(b"wave-%d" % p) for p in range(count))
    rs = bpperm.Reshuffler(gens, k)
    out, proofs = rs.shuffle_batch(cards, perms, seeds32=seeds)
    assert rs.verify_batch(cards, out, proofs)
    assert rs.verify_batch_each(cards, out, proofs) == [True] * count
    for p in (0, 64, count - 1):
        co = [out[p][32 * i:32 * i + 32] for i in range(k)]
        assert rr.verify(cards[p], co, proofs[p]), p
        assert rs.verify(cards[p], co, proofs[p])


@pytest.mark.parametrize("name", rr.EDGES)
def test_edge_inputs(gens, name):
    """The identity among the input cards, two equal cards, supplied blinds
    with a zero, pi the identity and the reversal: bytes equal the reference's."""
    import bpperm
    k = 5
    cards, perm, blinds = rr.edge_case(k, name)
    seed = rr.seed32(b"edge-%d" % k)
    want_out, want_pf = rr.prove(cards, perm, seed, blinds)
    rs = bpperm.Reshuffler(gens, k)
    out, proofs = rs.shuffle_batch([cards], [perm], blinds=[[rr.sb(b) for b in blinds]] if blinds else None,
                                   seeds32=seed)
    assert out == [b"".join(want_out)] and proofs == [want_pf]
    assert rs.verify(cards, want_out, want_pf)


@pytest.fixture(scope="module")
def one(gens):
    """One valid shuffle at k = 3, its Reshuffler and the regions of its proof."""
    import bpperm
    cards, perm, seed, _, out, pf = reference(3)[0]
    return bpperm.Reshuffler(gens, 3), cards, out, pf, {name: off for name, off, _ in rr.regions(3)}


def code_of(rs, cards, out, pf):
    import bpperm
    try:
        return 0 if rs.verify(cards, out, pf) else VERIFY
    except bpperm.BppError as e:
        return e.code


@pytest.mark.parametrize("region", ["A", "E", "Ti", "T", "z", "om", "zR", "Vk", "inner"])
def test_each_region_tampered_is_a_verification_error(one, region):
    rs, cards, out, pf, o = one
    at = o[region]
    if region in ("z", "om", "zR"):
        new = rr.sb(int.from_bytes(pf[at:at + 32], "little") + 1)
    elif region == "inner":
        at += 8 * 32  # tau_x
        new = rr.sb(int.from_bytes(pf[at:at + 32], "little") + 1)
    else:
        new = other_point(region.encode())
    bad = pf[:at] + new + pf[at + 32:]
    assert not rr.verify(cards, out, bad)
    assert code_of(rs, cards, out, bad) == VERIFY
    assert not rs.verify_batch([cards], [out], [bad])
    assert rs.verify_batch_each([cards, cards], [out, out], [pf, bad]) == [True, False]


def test_refusals_by_name(one):
    import bpperm
    rs, cards, out, pf, o = one
    undecodable = b"\xff" * 32
    assert code_of(rs, cards, [undecodable] + out[1:], pf) == DECOMPRESS
    assert code_of(rs, cards, out, pf[:o["E"] + 32] + undecodable + pf[o["E"] + 64:]) == DECOMPRESS  # E_1
    assert code_of(rs, cards, out, pf[:o["z"]] + L.to_bytes(32, "little") + pf[o["z"] + 32:]) == NONCANONICAL
    with pytest.raises(bpperm.BppError) as e:  # an undecodable input card: the prover too, and no output
        rs.shuffle_batch([[undecodable] + cards[1:]], [[0, 1, 2]], seeds32=rr.seed32(b"x"))
    assert e.value.code == DECOMPRESS
    # _each: the proofs with an undecodable point fail alone (two of them here, a card and T_S)
    bad_ts = pf[:o["T"]] + undecodable + pf[o["T"] + 32:]
    assert rs.verify_batch_each([cards] * 4, [out, [undecodable] + out[1:], out, out], [pf, pf, pf, bad_ts]) == \
        [True, False, True, False]
    with pytest.raises(bpperm.BppError) as e:  # the batch verdict names the refusal
        rs.verify_batch([cards, cards], [out, [undecodable] + out[1:]], [pf, pf])
    assert e.value.code == DECOMPRESS
    # an output that is no re-blinding: C'_0 + B
    g, _ = pedersen_gens_default()
    moved = [r255.encode(r255.ed_add(r255.decode(out[0]), g))] + out[1:]
    assert code_of(rs, cards, moved, pf) == VERIFY
    _, forced = rr.prove(cards, reference(3)[0][1], reference(3)[0][2], cards_out=moved)
    assert code_of(rs, cards, moved, forced) == VERIFY
    # swapped cards, and a proof one field short
    assert code_of(rs, [cards[1], cards[0], cards[2]], out, pf) == VERIFY
    assert code_of(rs, cards, [out[1], out[0], out[2]], pf) == VERIFY
    assert code_of(rs, cards, out, pf[:-32]) == VERIFY
    assert rs.verify_batch([], [], []) and rs.verify_batch_each([], [], []) == []


def test_verify_batch_each_names_the_failing_proofs(gens):
    """8 proofs at k = 4, proof 2 with a bad sigma part (z_1 + 1) and proof 5
    with a bad inner proof (its t_hat + 1): exactly those two zeros."""
    import bpperm
    k, count = 4, 8
    cards = [rr.rand_cards(k, b"each-%d" % p) for p in range(count)]
    perms = [rr.rand_perm(k, b"each-%d" % p) for p in range(count)]
    rs = bpperm.Reshuffler(gens, k)
    out, proofs = rs.shuffle_batch(cards, perms, seeds32=b"".join(rr.seed32(b"each-%d" % p) for p in range(count)))
    assert rs.verify_batch_each(cards, out, proofs) == [True] * count
    o = {name: off for name, off, _ in rr.regions(k)}

    def bump(pf, at):
        return pf[:at] + rr.sb(int.from_bytes(pf[at:at + 32], "little") + 1) + pf[at + 32:]

    bad = list(proofs)
    bad[2] = bump(bad[2], o["z"] + 32)
    bad[5] = bump(bad[5], o["inner"] + 10 * 32)
    lib, ok = rs.ctx.lib, bytearray(b"\x01" * count)
    import ctypes
    okb = (ctypes.c_char * count).from_buffer(ok)
    rc = lib.bpp_reshuffle_verify_batch_each(rs.ctx.h, gens.h, k, count, b"bp-perm", 7, b"".join(b"".join(c) for c in cards),
                                             b"".join(out), b"".join(bad), okb)
    assert rc == VERIFY
    assert list(ok) == [1, 1, 0, 1, 1, 0, 1, 1]
    assert not rs.verify_batch(cards, out, bad)
    for p in (2, 5):
        co = [out[p][32 * i:32 * i + 32] for i in range(k)]
        sigma, inner = rr.verify_parts(cards[p], co, bad[p])
        assert (sigma, inner) == ((False, True) if p == 2 else (True, False))


def test_verify_batch_each_error_text(gens):
    """3 proofs at k = 2, the last one's z_R with its lowest bit flipped (still
    canonical): the text counts the failing proofs and names the first."""
    import bpperm
    import ctypes
    k, rows = 2, reference(2)
    at = {name: off for name, off, _ in rr.regions(k)}["zR"]
    proofs = [r[5] for r in rows]
    proofs[2] = proofs[2][:at] + bytes([proofs[2][at] ^ 1]) + proofs[2][at + 1:]
    assert int.from_bytes(proofs[2][at:at + 32], "little") < L
    rs = bpperm.Reshuffler(gens, k)
    ok = ctypes.create_string_buffer(3)
    rc = rs.ctx.lib.bpp_reshuffle_verify_batch_each(rs.ctx.h, gens.h, k, 3, b"bp-perm", 7,
                                                    b"".join(b"".join(r[0]) for r in rows),
                                                    b"".join(b"".join(r[4]) for r in rows), b"".join(proofs), ok)
    text = (rs.ctx.lib.bpp_ctx_last_error(rs.ctx.h) or b"").decode()
    assert rc == VERIFY and list(ok.raw) == [1, 1, 0]
    assert text.endswith("1 of 3 proofs failed, the first at index 2"), text


def test_three_players_reshuffle_one_committed_deck(gens):
    """Player 0 commits 5 cards; players 1..3 re-shuffle in turn without any
    opening, every step verifies, and player 0 opens the final cards as
    v_{pi1 pi2 pi3 (i)} B + (gamma + r1 + r2 + r3) Bb."""
    import bpperm
    k = 5
    v = [10 + i for i in range(k)]
    gam = [rr.rand_scalar(b"chain-g%d" % i) for i in range(k)]
    deck = gens.pedersen_commit([rr.sb(x) for x in v], [rr.sb(x) for x in gam])
    rs = bpperm.Reshuffler(gens, k, label=b"chain")
    cards, src, blind = list(deck), list(range(k)), list(gam)
    for s in (1, 2, 3):
        perm = rr.rand_perm(k, b"chain-%d" % s)
        r = [rr.rand_scalar(b"chain-r%d-%d" % (s, i)) for i in range(k)]
        out, proofs = rs.shuffle_batch([cards], [perm], blinds=[[rr.sb(x) for x in r]])  # (the OS CSPRNG's seed)
        nxt = [out[0][32 * i:32 * i + 32] for i in range(k)]
        assert rs.verify(cards, nxt, proofs[0])
        assert not rs.verify(nxt, cards, proofs[0])
        src = [src[perm[i]] for i in range(k)]
        blind = [(blind[perm[i]] + r[i]) % L for i in range(k)]
        cards = nxt
    assert sorted(src) == list(range(k))
    opened = gens.pedersen_commit([rr.sb(v[j]) for j in src], [rr.sb(b) for b in blind])
    assert opened == cards


def test_secrets_are_wiped(gens, ctx):
    import bpperm
    k = 5
    rs = bpperm.Reshuffler(gens, k)
    cards = [rr.rand_cards(k, b"wipe-%d" % p) for p in range(3)]
    rs.shuffle_batch(cards, [rr.rand_perm(k, b"wipe-%d" % p) for p in range(3)],
                     blinds=[[rr.sb(rr.rand_scalar(b"wipe-r%d-%d" % (p, i))) for i in range(k)] for p in range(3)])
    assert ctx.secret_residue() == 0


def test_refusal_texts(gens, one):
    """k = 3, at most 3 proofs a call: what bpp_ctx_last_error ends with after
    each refusal that names a proof, the proof's index (never 0 alone) and the
    point's among them."""
    import bpperm
    rs, cards, out, pf, o = one
    perm, seed = reference(3)[0][1], reference(3)[0][2]
    lib, bad = rs.ctx.lib, b"\xff" * 32

    def text_of(code, f, *a, **kw):
        with pytest.raises(bpperm.BppError) as e:
            f(*a, **kw)
        assert e.value.code == code
        return (lib.bpp_ctx_last_error(rs.ctx.h) or b"").decode()

    def at(region, i):
        return pf[:o[region] + 32 * i] + bad + pf[o[region] + 32 * i + 32:]

    def verifier(code, q, ci=cards, co=out, proof=pf):  # three proofs, proof q as given
        cis, cos, pfs = [cards] * 3, [out] * 3, [pf] * 3
        cis[q], cos[q], pfs[q] = ci, co, proof
        return text_of(code, rs.verify_batch, cis, cos, pfs)

    # the prover
    t = text_of(DECOMPRESS, rs.shuffle_batch, [cards, cards[:2] + [bad]], [perm, perm], seeds32=seed * 2)
    assert t.endswith("reshuffle 1: input card 2 does not decode"), t
    t = text_of(ARG, rs.shuffle_batch, [cards] * 3, [perm, perm, [0, 0, 1]], seeds32=seed * 3)
    assert t.endswith("reshuffle 2: perm is not a bijection on [0, k)"), t
    t = text_of(NONCANONICAL, rs.shuffle_batch, [cards] * 2, [perm] * 2, seeds32=seed * 2,
                blinds=[[rr.sb(1)] * 3, [rr.sb(1), L.to_bytes(32, "little"), rr.sb(2)]])
    assert t.endswith("reshuffle 1: non-canonical blind"), t
    # the verifier, one case per class of point
    t = verifier(DECOMPRESS, 1, ci=[cards[0], bad, cards[2]])
    assert t.endswith("reshuffle 1: input card 1 does not decode"), t
    t = verifier(DECOMPRESS, 2, co=out[:2] + [bad])
    assert t.endswith("reshuffle 2: output card 2 does not decode"), t
    t = verifier(DECOMPRESS, 0, proof=at("A", 1))
    assert t.endswith("reshuffle 0: A 1 does not decode"), t
    t = verifier(DECOMPRESS, 2, proof=at("E", 0))
    assert t.endswith("reshuffle 2: E 0 does not decode"), t
    t = verifier(DECOMPRESS, 1, proof=at("Ti", 2))
    assert t.endswith("reshuffle 1: T 2 does not decode"), t
    t = verifier(DECOMPRESS, 2, proof=at("T", 0))
    assert t.endswith("reshuffle 2: T_S 0 does not decode"), t
    t = verifier(NONCANONICAL, 2, proof=pf[:o["om"]] + L.to_bytes(32, "little") + pf[o["om"] + 32:])
    assert t.endswith("reshuffle 2: a response scalar is not canonical"), t
    # k = 343, on both sides
    buf, sink = bytes(343 * 32), ctypes.create_string_buffer(343 * 32)
    ident = (ctypes.c_uint32 * 343)(*range(343))
    assert lib.bpp_reshuffle_prove_batch(rs.ctx.h, gens.h, 343, 1, buf, ident, None, seed, b"bp-perm", 7, sink,
                                         sink) == LEN
    assert (lib.bpp_ctx_last_error(rs.ctx.h) or b"").decode().endswith(K_TEXT)
    assert lib.bpp_reshuffle_verify(rs.ctx.h, gens.h, 343, b"bp-perm", 7, buf, buf, buf, 32) == LEN
    assert (lib.bpp_ctx_last_error(rs.ctx.h) or b"").decode().endswith(K_TEXT)


def test_a_batch_across_a_chunk_boundary(ctx):
    """k = 342: a launch sequence takes 2^22 / (5k + 1) = 2451 proofs, so 2452
    shuffles of one committed deck run as two.  The batch verifies; with z_0 + 1
    in proofs 0, 2450 and 2451 exactly those three fail; an undecodable A_0 in
    proof 2451 alone refuses the batch and names that proof."""
    import bpperm
    k, chunk = 342, 2451
    count = chunk + 1
    assert chunk == (1 << 22) // (5 * k + 1)
    rnd = random.Random(342)
    g = bpperm.Gens(ctx, 1024)
    try:
        rs = bpperm.Reshuffler(g, k)
        deck = b"".join(g.pedersen_commit([rr.sb(10 + i) for i in range(k)],
                                          [rr.sb(rnd.randrange(L)) for _ in range(k)]))
        cin = deck * count
        cout, proofs = rs.shuffle_batch(cin, [rnd.sample(range(k), k) for _ in range(count)],
                                        seeds32=rnd.randbytes(32 * count), raw=True)
        assert rs.verify_batch(cin, cout, proofs)
        pl, z0 = rs.proof_len, 32 * (3 * k + 1)
        bad = bytearray(proofs)
        for p in (0, chunk - 1, chunk):
            at = p * pl + z0
            bad[at:at + 32] = rr.sb(int.from_bytes(bad[at:at + 32], "little") + 1)
        ok = ctypes.create_string_buffer(count)
        rc = ctx.lib.bpp_reshuffle_verify_batch_each(ctx.h, g.h, k, count, b"bp-perm", 7, cin, cout, bytes(bad), ok)
        text = (ctx.lib.bpp_ctx_last_error(ctx.h) or b"").decode()
        assert rc == VERIFY
        assert [p for p in range(count) if not ok.raw[p]] == [0, chunk - 1, chunk]
        assert text.endswith("3 of %d proofs failed, the first at index 0" % count), text
        bad = bytearray(proofs)
        bad[chunk * pl:chunk * pl + 32] = b"\xff" * 32
        with pytest.raises(bpperm.BppError) as e:
            rs.verify_batch(cin, cout, bytes(bad))
        assert e.value.code == DECOMPRESS
        assert str(e.value).endswith("reshuffle %d: A 0 does not decode" % chunk), str(e.value)
    finally:
        g.close()
