"""bpp_deck_* on the GPU: public-deck shuffle proofs byte-exact against the
reference helper (tests/deck_ref.py) and the committed golden file, accepted and
rejected by the three verifiers, kept apart from two-half proofs of the same
shape, on both witness paths, under the prover's switches, with the batch's
secrets wiped and the old provers' bytes unchanged."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import deck_child  # noqa: E402
import deck_ref as dr  # noqa: E402
import shuffle_ref as sr  # noqa: E402
from oracle import bulletproofs as bp  # noqa: E402

pytestmark = pytest.mark.gpu
L = bp.L
GOLDEN = json.loads((HERE / "golden" / "deck.json").read_text())["cases"]


@pytest.fixture(scope="module")
def gens(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens2048(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 2048)
    yield g
    g.close()


def sb(xs):
    return [sr.scalar_bytes(x) for x in xs]


@pytest.mark.parametrize("deck_kind", ["default", "edge"])
@pytest.mark.parametrize("with_gammas", [False, True], ids=["drawn", "supplied"])
@pytest.mark.parametrize("k", [2, 3, 5, 6, 9])
def test_deck_bit_exact_vs_helper(gens, k, with_gammas, deck_kind):
    """n_p = 4 with one, two and four gates (k = 2, 3, 5), the first n_p = 8
    (k = 6) and n = n_p exactly (k = 9).  Three proofs per call; V and proof
    bytes equal the helper's, and the three verifiers accept."""
    import bpperm
    deck = None if deck_kind == "default" else sr.edge_decks(k)[0]
    perms = [sr.rand_perm(k, b"gd-%d-%d" % (k, i)) for i in range(3)]
    seeds = [sr.seed32(b"gd-%d-%d" % (k, i)) for i in range(3)]
    gam = None
    if with_gammas:
        gam = [[sr.rand_scalar(b"gdg-%d-%d-%d" % (k, i, j)) for j in range(k)] for i in range(3)]
        gam[1][0], gam[1][1] = 0, L - 1
    pr = bpperm.DeckProver(gens, k, sb(deck) if deck else None)
    assert pr.proof_len == dr.deck_proof_len(k)
    proofs, Vs = pr.prove_batch(perms, b"".join(seeds), [sb(g) for g in gam] if gam else None)
    for i in range(3):
        want = dr.prove_deck(deck, perms[i], seeds[i], gam[i] if gam else None)
        assert Vs[i] == b"".join(want.V), i
        assert proofs[i] == want.to_bytes(), i
        assert pr.verify(proofs[i], Vs[i])
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * 3


@pytest.mark.parametrize("case", GOLDEN, ids=lambda c: "k%d" % c["k"])
def test_deck_golden(gens, case):
    import bpperm
    k = case["k"]
    deck = [bytes.fromhex(h) for h in case["deck"]] if case["deck"] else None
    gam = [[bytes.fromhex(h) for h in row] for row in case["gammas"]] if case["gammas"] else None
    pr = bpperm.DeckProver(gens, k, deck, label=case["label"].encode())
    proofs, Vs = pr.prove_batch(case["perms"], b"".join(bytes.fromhex(s) for s in case["seeds"]), gam)
    assert [p.hex() for p in proofs] == case["proofs"]
    assert [v.hex() for v in Vs] == ["".join(v) for v in case["V"]]
    assert all(pr.verify(p, v) for p, v in zip(proofs, Vs))
    assert pr.verify_batch(proofs, Vs)
    assert pr.verify_batch_each(proofs, Vs) == [True] * len(proofs)


@pytest.fixture(scope="module")
def batch8(gens):
    import bpperm
    k = 6
    deck = sr.edge_decks(k)[1]
    pr = bpperm.DeckProver(gens, k, sb(deck))
    perms = [sr.rand_perm(k, b"b8-%d" % i) for i in range(8)]
    proofs, Vs = pr.prove_batch(perms, b"".join(sr.seed32(b"b8-%d" % i) for i in range(8)))
    return k, deck, pr, proofs, Vs


def _tamper(proofs, Vs, i, what):
    p, v = bytearray(proofs[i]), bytearray(Vs[i])
    if what == "V":
        v[32 * 2 + 5] ^= 1
    elif what == "t_hat":
        p[32 * 10 + 3] ^= 1
    elif what == "L":
        p[32 * 11 + 7] ^= 1
    else:  # mu = l: not a canonical scalar
        p[32 * 9: 32 * 10] = L.to_bytes(32, "little")
    return proofs[:i] + [bytes(p)] + proofs[i + 1:], Vs[:i] + [bytes(v)] + Vs[i + 1:]


@pytest.mark.parametrize("what,i", [("V", 0), ("t_hat", 3), ("L", 5), ("mu", 7)])
def test_deck_batch_names_the_tampered_proof(batch8, what, i):
    k, deck, pr, proofs, Vs = batch8
    assert pr.verify_batch(proofs, Vs)
    bp_, bv = _tamper(proofs, Vs, i, what)
    assert not pr.verify_batch(bp_, bv)
    each = pr.verify_batch_each(bp_, bv)
    assert each == [j != i for j in range(8)]
    assert each == [pr.verify(p, v) for p, v in zip(bp_, bv)]


def test_deck_wrong_deck_and_label_reject_all(gens, batch8):
    import bpperm
    k, deck, pr, proofs, Vs = batch8
    other = list(deck)
    other[k - 1] = (other[k - 1] + 1) % L
    for bad in (bpperm.DeckProver(gens, k, sb(other)), bpperm.DeckProver(gens, k, sb(deck), label=b"another")):
        assert not bad.verify_batch(proofs, Vs)
        assert bad.verify_batch_each(proofs, Vs) == [False] * 8
        assert not bad.verify(proofs[0], Vs[0])
    with pytest.raises(bpperm.BppError):  # a deck card = l
        bpperm.DeckProver(gens, k, sb(deck[:-1]) + [L.to_bytes(32, "little")]).verify_batch(proofs, Vs)


def test_deck_and_two_half_proofs_of_one_shape(ctx, gens):
    """k' = 3 two-half and k = 6 deck proofs share m, n_p and byte length: each
    verifier rejects the other's proofs, and a batch of 8 costs the same MSM
    work either way (the deck path adds no hidden MSM)."""
    import bpperm
    two, deckp = bpperm.PermProver(gens, 3), bpperm.DeckProver(gens, 6)
    assert two.proof_len == deckp.proof_len and two.m == deckp.m
    tp, tv = two.prove_batch(list(range(8)))
    dp, dv = deckp.prove_batch([sr.rand_perm(6, b"col-%d" % i) for i in range(8)],
                               b"".join(sr.seed32(b"col-%d" % i) for i in range(8)))
    ctx.work_reset()
    assert two.verify_batch(tp, tv)
    w_two = ctx.work()
    ctx.work_reset()
    assert deckp.verify_batch(dp, dv)
    w_deck = ctx.work()
    assert w_deck == w_two and w_two["msm_terms"] > 0
    assert not deckp.verify_batch(tp, tv) and not two.verify_batch(dp, dv)
    assert deckp.verify_batch_each(tp, tv) == [False] * 8 and two.verify_batch_each(dp, dv) == [False] * 8
    assert not deckp.verify(tp[0], tv[0]) and not two.verify(dp[0], dv[0])


def test_deck_witness_paths(gens2048, monkeypatch):
    """k = 1536: the last k of k_witness_deck's LDS budget, byte for byte
    against the host witness of the same batch; k = 1537: the host witness."""
    import bpperm
    k = 1536
    deck = [sr.rand_scalar(b"wp-%d" % i) for i in range(k + 1)]
    perms = [sr.rand_perm(k, b"wp-%d" % p) for p in range(2)]
    seeds = b"".join(sr.seed32(b"wp-%d" % p) for p in range(2))
    pr = bpperm.DeckProver(gens2048, k, sb(deck[:k]))
    proofs, Vs = pr.prove_batch(perms, seeds)
    assert pr.verify_batch(proofs, Vs)
    monkeypatch.setenv("BPP_DECK_HOST_WITNESS", "1")
    host, hostV = pr.prove_batch(perms, seeds)
    monkeypatch.delenv("BPP_DECK_HOST_WITNESS")
    assert host == proofs and hostV == Vs
    k = 1537
    pr = bpperm.DeckProver(gens2048, k, sb(deck))
    proofs, Vs = pr.prove_batch([sr.rand_perm(k, b"wq-%d" % p) for p in range(2)], seeds)
    assert pr.verify_batch(proofs, Vs)


@pytest.mark.parametrize("env", [{"BPP_PROVE_STREAMS": "3"}, {"BPP_PROVE_DEV_V": "0"}, {"BPP_PROVE_DEV_V": "1"}],
                         ids=["streams3", "dev_v0", "dev_v1"])
def test_deck_bytes_under_switches(ctx, env):
    """The same proofs under BPP_PROVE_STREAMS=3 and both settings of
    BPP_PROVE_DEV_V, each in a child process."""
    want_p, want_v = deck_child.prove(ctx)
    e = {k: v for k, v in os.environ.items() if k not in ("BPP_PROVE_STREAMS", "BPP_PROVE_DEV_V")}
    e.update(env)
    r = subprocess.run([sys.executable, str(HERE / "deck_child.py")], capture_output=True, text=True, env=e,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = dict(line.split(" ", 1) for line in r.stdout.splitlines() if line.startswith(("PROOFS ", "V ")))
    assert out["PROOFS"] == want_p.hex() and out["V"] == want_v.hex()


@pytest.mark.parametrize("streams", [1, 3])
def test_deck_leaves_no_secret_bytes(ctx, gens, monkeypatch, streams):
    import bpperm
    k, n = 52, 7
    pr = bpperm.DeckProver(gens, k)
    perms = [sr.rand_perm(k, b"dres-%d" % i) for i in range(n)]
    seeds = b"".join(sr.seed32(b"dres-%d" % i) for i in range(n))
    gam = [[sr.scalar_bytes(sr.rand_scalar(b"drg-%d-%d" % (p, j))) for j in range(k)] for p in range(n)]
    monkeypatch.setenv("BPP_PROVE_STREAMS", "1")
    want, wantV = pr.prove_batch(perms, seeds, gam)
    monkeypatch.setenv("BPP_PROVE_STREAMS", str(streams))
    bpperm.PermProver(gens, k).prove_batch([3, 4, 5])  # a test-hook batch leaves its secrets in place
    assert ctx.secret_residue() > 0
    got, gotV = pr.prove_batch(perms, seeds, gam)
    assert ctx.secret_residue() == 0
    assert got == want and gotV == wantV
    assert pr.verify_batch(got, gotV)


def test_old_provers_unchanged_after_a_deck_batch(gens):
    """A seeded batch (the golden config-1 proof among it) and a shuffle batch
    give the same bytes before and after a deck batch on the same context."""
    import bpperm
    k = 52
    gold = json.loads((HERE / "golden" / "protocol.json").read_text())["config1"]
    pr = bpperm.PermProver(gens, k, label=gold["label"].encode())
    cards = [sb(sr.rand_scalar(b"oc-%d-%d" % (p, i)) for i in range(k)) for p in range(2)]
    perms = [sr.rand_perm(k, b"oc-%d" % p) for p in range(2)]
    sseeds = b"".join(sr.seed32(b"oc-%d" % p) for p in range(2))
    before = pr.prove_batch([gold["seed"], 12, 13])
    sbefore = pr.prove_shuffle_batch(cards, perms, sseeds)
    assert before[0][0].hex() == gold["proof"] and before[1][0].hex() == "".join(gold["V"])
    dk = bpperm.DeckProver(gens, k)
    dp, dv = dk.prove_batch([sr.rand_perm(k, b"od-%d" % i) for i in range(3)])
    assert dk.verify_batch(dp, dv)
    assert pr.prove_batch([gold["seed"], 12, 13]) == before
    assert pr.prove_shuffle_batch(cards, perms, sseeds) == sbefore
    assert pr.verify_batch(before[0] + sbefore[0], before[1] + sbefore[1])
