"""Mixed batches on the GPU (bpp_verify_groups, bpp_verify_groups_each;
bpperm.verify_groups): proofs of five statements of three widths in one call
with one MSM.

The reference for every verdict is the unchanged single-proof entry point,
prover.verify(proof, V[, pub]); never the code under test.  The shapes are the
smallest at which each piece can go wrong:

  A  PermProver(k = 2)                      n_p = 4   m = 5
  B  DeckProver(k = 6)                      n_p = 8   m = 7
  C  CircuitProver(two_half_shuffle(3))     n_p = 8   m = 7   B's byte lengths
  D  CircuitProver(shuffle_of_public(5))    n_p = 8   m = 6   public inputs
  E  CircuitProver(in_range(16))            n_p = 16  m = 2

three proofs each unless stated.  A valid batch fails if one generator scalar
of the merged block is misplaced, so the accepting runs -- the widest group first
and last, a generator set exactly as long as the widest circuit (no index list)
and a longer one (index list) -- test the layout; the rejecting runs test that
every failure class of every group is named, and only it."""
import ctypes as C
import hashlib

import pytest

pytestmark = pytest.mark.gpu

L = 2**252 + 27742317777372353535851937790883648493
ORDER = "ABCDE"


def sb(x):
    return (x % L).to_bytes(32, "little")


def rs(tag):
    return int.from_bytes(hashlib.sha512(tag).digest(), "little") % L


def seed32(tag):
    return hashlib.sha256(tag).digest()


def perm_of(n, tag):
    return sorted(range(n), key=lambda i: hashlib.sha256(tag + b"%d" % i).digest())


class Group:
    """One statement's prover, its valid proofs and their single-proof verdicts."""

    def __init__(self, prover, proofs, Vs, pub=None):
        self.pr, self.proofs, self.Vs, self.pub = prover, list(proofs), list(Vs), pub

    def entry(self, proofs=None, Vs=None, pub=None, n=None):
        p, v = self.proofs if proofs is None else proofs, self.Vs if Vs is None else Vs
        u = self.pub if pub is None else pub
        if n is not None:
            p, v, u = p[:n], v[:n], (u[:n] if u is not None else None)
        return (self.pr, p, v) if u is None else (self.pr, p, v, u)

    def singles(self, proofs=None, Vs=None, pub=None):
        p, v = self.proofs if proofs is None else proofs, self.Vs if Vs is None else Vs
        u = self.pub if pub is None else pub
        if u is None:
            return [self.pr.verify(p[i], v[i]) for i in range(len(p))]
        return [self.pr.verify(p[i], v[i], pub=u[i]) for i in range(len(p))]


def make_groups(bpperm, gens, n=3, tag=b"vg"):
    from bpperm import gadgets as gd
    out = {}
    a = bpperm.PermProver(gens, 2)
    out["A"] = Group(a, *a.prove_batch([rs(tag + b"A%d" % i) % 2**60 for i in range(n)]))
    b = bpperm.DeckProver(gens, 6)
    out["B"] = Group(b, *b.prove_batch([perm_of(6, tag + b"B%d" % i) for i in range(n)],
                                       b"".join(seed32(tag + b"B%d" % i) for i in range(n))))
    c = bpperm.CircuitProver(gens, gd.two_half_shuffle(3))
    vs = []
    for i in range(n):
        half = [rs(tag + b"C%d-%d" % (i, j)) for j in range(3)]
        vs.append([sb(x) for x in half + [half[j] for j in perm_of(3, tag + b"C%d" % i)]])
    out["C"] = Group(c, *c.prove_batch(vs, None, b"".join(seed32(tag + b"C%d" % i) for i in range(n))))
    d = bpperm.CircuitProver(gens, gd.shuffle_of_public(5))
    pubs, vs = [], []
    for i in range(n):
        deck = [rs(tag + b"D%d-%d" % (i, j)) for j in range(5)]
        pubs.append(b"".join(sb(x) for x in deck))
        vs.append([sb(deck[j]) for j in perm_of(5, tag + b"D%d" % i)])
    out["D"] = Group(d, *d.prove_batch(vs, None, b"".join(seed32(tag + b"D%d" % i) for i in range(n)), pub=pubs),
                     pub=pubs)
    desc = gd.in_range(16)
    e = bpperm.CircuitProver(gens, desc)
    xs = [[rs(tag + b"E%d" % i) % 2**16] for i in range(n)]
    out["E"] = Group(e, *e.prove_batch([[sb(x[0])] for x in xs], [[sb(h) for h in desc.aux_of(x)] for x in xs],
                                       b"".join(seed32(tag + b"E%d" % i) for i in range(n))))
    return out


@pytest.fixture(scope="module")
def gens16(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 16)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens128(ctx):
    import bpperm
    g = bpperm.Gens(ctx, 128)
    yield g
    g.close()


@pytest.fixture(scope="module")
def grp(gens128):
    """Groups A-E, made once and left unchanged; every proof verifies alone."""
    import bpperm
    g = make_groups(bpperm, gens128)
    shape = {k: (g[k].pr.proof_len, g[k].pr.m) for k in ORDER}
    assert shape["B"] == shape["C"] and shape["A"] != shape["B"]  # the collision, and a group that differs
    np_of = {"A": 4, "B": 8, "C": 8, "D": 8, "E": 16}
    for k in "CDE":
        assert g[k].pr.circuit.n_p == np_of[k]
    for k in ORDER:
        assert g[k].singles() == [True] * 3, k
    return g


def terms(grp, counts):
    """2 n_max + 2 merged generators + every group's proof points."""
    lg = {"A": 2, "B": 3, "C": 3, "D": 3, "E": 4}
    return 2 * 16 + 2 + sum(counts[k] * (grp[k].pr.m + 8 + 2 * lg[k]) for k in counts)


# ---------------------------------------------------------------------------
# 1. accept

@pytest.mark.parametrize("order", [ORDER, ORDER[::-1]], ids=["widest_last", "widest_first"])
@pytest.mark.parametrize("gn", [16, 128], ids=["no_index_list", "index_list"])
def test_accept(grp, gens16, gens128, order, gn):
    import bpperm
    gens = gens16 if gn == 16 else gens128
    call = [grp[k].entry() for k in order]
    assert bpperm.verify_groups(gens, call) is True
    assert bpperm.verify_groups(gens, call, each=True) == [[True] * 3] * 5


# ---------------------------------------------------------------------------
# 2. reject and name

def _xor(b, off, x):
    b = bytearray(b)
    b[off] ^= x
    return bytes(b)


def spoil(g, how):
    """-> (proofs, Vs, pub) of group g with proof 1 spoiled (`swap`: the public
    inputs of proofs 0 and 2 exchanged)."""
    p, v, u = list(g.proofs), list(g.Vs), (list(g.pub) if g.pub is not None else None)
    if how == "t_hat":  # stays canonical: the proof's MSM fails
        p[1] = _xor(p[1], 10 * 32 + 6, 1)
    elif how == "point":  # L_0 = an encoding that does not decode (s >= p)
        p[1] = p[1][:11 * 32] + b"\xff" * 32 + p[1][12 * 32:]
    elif how == "scalar":  # tau_x >= l: the replay rejects
        p[1] = _xor(p[1], 8 * 32 + 31, 0xF0)
    elif how == "swap":
        u[0], u[2] = u[2], u[0]
    return p, v, u


CASES = [(k, how) for k in ORDER for how in ("t_hat", "point", "scalar")] + [("D", "swap")]


@pytest.mark.parametrize("which,how", CASES, ids=["%s-%s" % c for c in CASES])
def test_reject_and_name(grp, gens128, which, how):
    import bpperm
    p, v, u = spoil(grp[which], how)
    want = grp[which].singles(p, v, u)
    assert not all(want)
    call = [grp[k].entry(p, v, u) if k == which else grp[k].entry() for k in ORDER]
    assert bpperm.verify_groups(gens128, call) is False
    got = bpperm.verify_groups(gens128, call, each=True)
    for k, verdicts in zip(ORDER, got):
        assert verdicts == (want if k == which else [True] * 3), k


def test_error_text_names_count_and_first(grp, ctx, gens128):
    """3 two-half proofs (k = 2) and 2 deck proofs (k = 3), the first deck proof
    with t_hat's lowest bit flipped (still canonical): proof 3 of the call."""
    import bpperm
    a = grp["A"]
    d = bpperm.DeckProver(gens128, 3)
    proofs, Vs = d.prove_batch([perm_of(3, b"txt%d" % i) for i in range(2)],
                               b"".join(seed32(b"txt%d" % i) for i in range(2)))
    proofs[0] = _xor(proofs[0], 10 * 32, 1)
    assert [d.verify(proofs[i], Vs[i]) for i in range(2)] == [False, True]
    call = [a.entry(), (d, proofs, Vs)]
    last = lambda: (ctx.lib.bpp_ctx_last_error(ctx.h) or b"").decode()
    assert bpperm.verify_groups(gens128, call, each=True) == [[True] * 3, [False, True]]
    assert last().endswith("1 of 5 proofs failed, the first at index 3"), last()
    assert bpperm.verify_groups(gens128, call) is False  # (rc 6: any other code raises)
    assert last().endswith("the batch check failed"), last()


# ---------------------------------------------------------------------------
# 3. kept apart

def test_same_lengths_kept_apart(grp, gens128):
    """B's valid proofs handed in as a C group and the reverse: the byte lengths
    agree, the statements do not."""
    import bpperm
    b, c = grp["B"], grp["C"]
    assert Group(c.pr, b.proofs, b.Vs).singles() == [False] * 3
    assert Group(b.pr, c.proofs, c.Vs).singles() == [False] * 3
    call = [grp["A"].entry(), (c.pr, b.proofs, b.Vs), (b.pr, c.proofs, c.Vs), grp["D"].entry(), grp["E"].entry()]
    assert bpperm.verify_groups(gens128, call) is False
    assert bpperm.verify_groups(gens128, call, each=True) == [[True] * 3, [False] * 3, [False] * 3, [True] * 3,
                                                              [True] * 3]


# ---------------------------------------------------------------------------
# 4. weights are per call

def test_weights_per_call(grp, gens128):
    """The same statement as two groups: the bad proof sits at position 1 of
    the call in one and at position 2 in the other."""
    import bpperm
    a = grp["A"]
    bad = _xor(a.proofs[1], 10 * 32 + 6, 1)
    assert a.pr.verify(bad, a.Vs[1]) is False
    call = [(a.pr, [a.proofs[0], bad], [a.Vs[0], a.Vs[1]]), (a.pr, [bad, a.proofs[2]], [a.Vs[1], a.Vs[2]])]
    assert bpperm.verify_groups(gens128, call) is False
    assert bpperm.verify_groups(gens128, call, each=True) == [[True, False], [False, True]]
    good = [(a.pr, a.proofs[:2], a.Vs[:2]), (a.pr, a.proofs[1:], a.Vs[1:])]
    assert bpperm.verify_groups(gens128, good) is True


# ---------------------------------------------------------------------------
# 5. edges

def test_single_group_and_empty(grp, gens128):
    import bpperm
    for k in ORDER:
        g = grp[k]
        batch = g.pr.verify_batch(g.proofs, g.Vs, **({"pub": g.pub} if g.pub is not None else {}))
        assert bpperm.verify_groups(gens128, [g.entry()]) is batch is True
    p, v, u = spoil(grp["E"], "t_hat")
    assert grp["E"].pr.verify_batch(p, v) is False
    assert bpperm.verify_groups(gens128, [(grp["E"].pr, p, v)]) is False
    # nothing to verify
    assert bpperm.verify_groups(gens128, []) is True
    assert bpperm.verify_groups(gens128, [], each=True) == []
    assert bpperm.verify_groups(gens128, [grp["A"].entry(n=0), grp["D"].entry(n=0)], each=True) == [[], []]
    # an empty group between two others
    call = [grp["A"].entry(), grp["E"].entry(n=0), grp["D"].entry()]
    assert bpperm.verify_groups(gens128, call) is True
    call[2] = grp["D"].entry(*spoil(grp["D"], "swap"))
    assert bpperm.verify_groups(gens128, call, each=True) == [[True] * 3, [], grp["D"].singles(*spoil(grp["D"], "swap"))]


def test_counts_1_65_3(grp, gens128):
    """More than one replay workgroup in one group, a single proof in another."""
    import bpperm
    b = grp["B"].pr
    proofs, Vs = b.prove_batch([perm_of(6, b"b65-%d" % i) for i in range(65)],
                               b"".join(seed32(b"b65-%d" % i) for i in range(65)))
    call = [grp["A"].entry(n=1), (b, proofs, Vs), grp["E"].entry()]
    assert bpperm.verify_groups(gens128, call) is True
    proofs[64] = _xor(proofs[64], 10 * 32 + 6, 1)
    proofs[3] = _xor(proofs[3], 8 * 32 + 31, 0xF0)
    want = [b.verify(proofs[i], Vs[i]) for i in range(65)]
    assert [i for i, ok in enumerate(want) if not ok] == [3, 64]
    call[1] = (b, proofs, Vs)
    assert bpperm.verify_groups(gens128, call) is False
    assert bpperm.verify_groups(gens128, call, each=True) == [[True], want, [True] * 3]


def test_refusals(grp, ctx, gens128):
    import bpperm
    from bpperm import BppError
    # generators shorter than the widest circuit: verify_batch's error, no verdict
    g8 = bpperm.Gens(ctx, 8)
    e = grp["E"]
    with pytest.raises(BppError) as single:
        bpperm.CircuitProver(g8, e.pr.circuit).verify_batch(e.proofs, e.Vs)
    for each in (False, True):
        with pytest.raises(BppError) as mixed:
            bpperm.verify_groups(g8, [grp["A"].entry(), e.entry(), grp["B"].entry()], each=each)
        assert mixed.value.code == single.value.code == 2
    assert bpperm.verify_groups(g8, [grp["A"].entry(), grp["B"].entry()]) is True  # (8 covers these)
    g8.close()
    # what the per-kind entry points refuse, and what only a mixed call can get wrong
    d = grp["D"]
    with pytest.raises(BppError) as err:
        bpperm.verify_groups(gens128, [grp["A"].entry(), (d.pr, d.proofs, d.Vs)])  # pub missing
    assert err.value.code == 1
    arr = (bpperm._VerifyGroupC * 1)()  # pub given for a circuit with n_pub = 0
    arr[0].kind, arr[0].circuit, arr[0].count = 2, e.pr.circuit.h, 3
    arr[0].proofs, arr[0].V, arr[0].pub = b"".join(e.proofs), b"".join(e.Vs), b"".join(d.pub)
    arr[0].label, arr[0].label_len = e.pr.label, len(e.pr.label)
    assert ctx.lib.bpp_verify_groups(ctx.h, gens128.h, arr, 1) == 1
    arr[0].pub = None
    assert ctx.lib.bpp_verify_groups(ctx.h, gens128.h, arr, 1) == 0
    with pytest.raises(BppError) as err:
        bpperm.verify_groups(gens128, [(d.pr, d.proofs, d.Vs, [d.pub[0], d.pub[1][:-32] + b"\xff" * 32, d.pub[2]])])
    assert err.value.code == 4
    with pytest.raises(BppError) as err:
        bpperm.verify_groups(gens128, [grp["A"].entry()] * 17)
    assert err.value.code == 2
    deck = bpperm.DeckProver(gens128, 6, [sb(i) for i in range(1, 6)] + [b"\xff" * 32])
    with pytest.raises(BppError) as err:
        bpperm.verify_groups(gens128, [grp["A"].entry(), (deck, grp["B"].proofs, grp["B"].Vs)], each=True)
    assert err.value.code == 4
    arr = (bpperm._VerifyGroupC * 1)()
    arr[0].kind = 3
    assert ctx.lib.bpp_verify_groups(ctx.h, gens128.h, arr, 1) == 1
    assert b"group 0" in ctx.lib.bpp_ctx_last_error(ctx.h)
    arr[0].kind, arr[0].k = 0, 1
    assert ctx.lib.bpp_verify_groups(ctx.h, gens128.h, arr, 1) == 1  # k out of range, count 0 all the same
    arr[0].kind, arr[0].circuit = 2, None
    assert ctx.lib.bpp_verify_groups(ctx.h, gens128.h, arr, 1) == 1  # a null circuit
    # none of it moved anything: the next call verifies
    assert bpperm.verify_groups(gens128, [grp[k].entry() for k in ORDER]) is True


# ---------------------------------------------------------------------------
# 6. work

def test_work_counters(grp, ctx, gens128):
    """One MSM of 2 n_max + 2 + sum count (m + 8 + 2 lg) terms, and as many
    engine launches as one single-kind verify_batch issues."""
    import bpperm

    def delta(f):
        w0 = ctx.work()
        assert f() is True
        w1 = ctx.work()
        return {n: w1.get(n, 0) - w0.get(n, 0) for n in w1}

    one = delta(lambda: grp["B"].pr.verify_batch(grp["B"].proofs, grp["B"].Vs))
    assert one["msm_terms"] == 2 * 8 + 2 + 3 * (7 + 8 + 6) and one["msm_launches"] >= 1
    mixed = delta(lambda: bpperm.verify_groups(gens128, [grp[k].entry() for k in ORDER]))
    assert mixed["msm_terms"] == terms(grp, {k: 3 for k in ORDER})
    assert mixed["msm_launches"] == one["msm_launches"]
    each = delta(lambda: all(all(v) for v in bpperm.verify_groups(gens128, [grp[k].entry() for k in ORDER], each=True)))
    # a passing _each call costs what the plain one costs
    assert (each["msm_terms"], each["msm_launches"]) == (mixed["msm_terms"], mixed["msm_launches"])


# ---------------------------------------------------------------------------
# 7. old paths untouched

def test_old_paths_after_groups(grp, gens128):
    """verify_groups -- passing, failing and naming -- then the per-kind entry
    points on the same context: their verdicts, good and bad."""
    import bpperm
    p, v, u = spoil(grp["D"], "swap")
    pa, va, _ = spoil(grp["A"], "point")
    call = [grp["A"].entry(pa, va), grp["B"].entry(), grp["D"].entry(p, v, u)]
    assert bpperm.verify_groups(gens128, [grp[k].entry() for k in ORDER]) is True
    assert bpperm.verify_groups(gens128, call) is False
    got = bpperm.verify_groups(gens128, call, each=True)
    assert got == [grp["A"].singles(pa, va), [True] * 3, grp["D"].singles(p, v, u)]
    a, b, d = grp["A"], grp["B"], grp["D"]
    assert a.pr.verify_batch(a.proofs, a.Vs) is True and a.pr.verify_batch(pa, va) is False
    assert a.pr.verify_batch_each(pa, va) == got[0]
    assert b.pr.verify_batch(b.proofs, b.Vs) is True
    assert b.pr.verify_batch_each(b.proofs, b.Vs) == [True] * 3
    assert d.pr.verify_batch(d.proofs, d.Vs, pub=d.pub) is True and d.pr.verify_batch(p, v, pub=u) is False
    assert d.pr.verify_batch_each(p, v, pub=u) == got[2]
    # a device job begun on the context before the call is still that context's job after it
    job = bpperm.VerifyJob(2, a.proofs, a.Vs, ctx=a.pr.ctx)
    assert bpperm.verify_groups(gens128, [grp[k].entry() for k in ORDER[::-1]]) is True
    assert bpperm.verify_groups(gens128, call, each=True) == got
    part = a.pr.verify_partial(job, bpperm.verify_seed(), 0, 0, job.windows()[1])
    assert part is not None and bpperm.partials_is_identity([part])
    job.close()
