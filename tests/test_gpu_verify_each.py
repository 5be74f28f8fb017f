"""Batch verification that names the failing proofs
(bpp_perm_verify_batch_each / PermProver.verify_batch_each): a batch that
passes is verify_batch's one merged MSM; one that does not runs every proof's
own MSM over the scalars and points the batch left on the device
(k_verify_each_terms, the multi-MSM engine, k_verify_each_verdict).

The reference for every verdict vector is the unchanged single-proof path,
[pr.verify(proofs[i], Vs[i]) for i], beside the set of indices the test
tampered.  Covered: circuits with padded gates; every failure class (MSM,
replay-rejected scalar and point, undecodable point, swapped V) with bad
proofs on both sides of a wave border and in the last place; the edges of
count; a generator set longer than the circuit; several passes
(BPP_VERIFY_EACH_PROOFS) with the work counters of each path; a passing
batch's counters equal verify_batch's; the call supersedes a device job."""
import pytest

pytestmark = pytest.mark.gpu

K = 52
PLEN = 8 * 32 + 3 * 32 + 14 * 32 + 2 * 32  # bpp_perm_proof_len(52)
NG, NPT = 2 * 128 + 2, (2 * K + 1) + 8 + 2 * 7  # generator / proof-point terms of one 52-card proof
BAD = {0, 11, 50, 60, 63, 64, 69}


def _xor(items, i, off, x):
    b = bytearray(items[i])
    b[off] ^= x
    items[i] = bytes(b)


@pytest.fixture(scope="module")
def batch(ctx):
    """70 52-card proofs, the tampered copy of test 2 and the verdicts of the
    single-proof path over it (computed once)."""
    import bpperm
    g = bpperm.Gens(ctx, 128)
    pr = bpperm.PermProver(g, K)
    proofs, Vs = pr.prove_batch(list(range(81_000, 81_070)))
    assert len(proofs[0]) == PLEN
    bp, bv = list(proofs), list(Vs)
    _xor(bp, 0, 8 * 32 + 70, 1)  # t_hat, stays canonical: the MSM fails
    _xor(bp, 11, 8 * 32 + 31, 0xF0)  # tau_x not canonical: the replay rejects
    b = bytearray(bp[50])
    b[32:64] = bytes(32)  # A_O = the identity encoding: the replay rejects
    bp[50] = bytes(b)
    _xor(bp, 60, 11 * 32 + 31, 0x80)  # L_0's top bit: does not decode
    bv[63], bv[64] = bv[64], bv[63]  # V blocks swapped across the wave border
    _xor(bp, 69, PLEN - 32, 1)  # b, the last proof
    singles = [pr.verify(bp[i], bv[i]) for i in range(70)]
    yield g, pr, proofs, Vs, bp, bv, singles
    g.close()


def test_small_circuits_all_good(ctx):
    """lg = 2..5, 2k not a power of two (padded gates); rc 0."""
    import bpperm
    g = bpperm.Gens(ctx, 64)
    for k in (2, 3, 7, 16):
        pr = bpperm.PermProver(g, k)
        proofs, Vs = pr.prove_batch(list(range(140 + k, 152 + k)))
        assert pr.verify_batch_each(proofs, Vs) == [True] * 12, k
    g.close()


def test_every_failure_class(batch):
    _, pr, proofs, Vs, bp, bv, singles = batch
    got = pr.verify_batch_each(bp, bv)
    assert [i for i, ok in enumerate(got) if not ok] == sorted(BAD)
    assert got == singles
    # the return code behind the list
    import ctypes as C
    ok = C.create_string_buffer(70)
    rc = pr.ctx.lib.bpp_perm_verify_batch_each(pr.ctx.h, pr.gens.h, K, 70, pr.label, len(pr.label), b"".join(bp),
                                               b"".join(bv), ok)
    assert rc == 6 and [x != 0 for x in ok.raw] == singles and set(ok.raw) == {0, 1}
    rc = pr.ctx.lib.bpp_perm_verify_batch_each(pr.ctx.h, pr.gens.h, K, 70, pr.label, len(pr.label), b"".join(proofs),
                                               b"".join(Vs), ok)
    assert rc == 0 and ok.raw == b"\x01" * 70
    # the untampered batch still verifies on the same context afterwards
    assert pr.verify_batch(proofs, Vs)


def _each_raw(pr, k, proofs, Vs):
    """-> (rc, verdict bytes, the context's error text) of one bpp_perm_verify_batch_each call"""
    import ctypes as C
    n = len(proofs)
    ok = C.create_string_buffer(n)
    rc = pr.ctx.lib.bpp_perm_verify_batch_each(pr.ctx.h, pr.gens.h, k, n, pr.label, len(pr.label), b"".join(proofs),
                                               b"".join(Vs), ok)
    return rc, list(ok.raw), (pr.ctx.lib.bpp_ctx_last_error(pr.ctx.h) or b"").decode()


@pytest.fixture(scope="module")
def small(ctx):
    """5 proofs at k = 2 (8 points, tau_x, mu, t_hat, L_0 ...), left unchanged."""
    import bpperm
    g = bpperm.Gens(ctx, 64)
    pr = bpperm.PermProver(g, 2)
    proofs, Vs = pr.prove_batch(list(range(82_000, 82_005)))
    yield pr, proofs, Vs
    g.close()


def test_error_text_names_count_and_first(small):
    """Proof 2 of 5 with t_hat's lowest bit flipped (still canonical)."""
    pr, proofs, Vs = small
    bad = list(proofs)
    _xor(bad, 2, 10 * 32, 1)
    assert [pr.verify(bad[i], Vs[i]) for i in range(5)] == [True, True, False, True, True]
    rc, ok, text = _each_raw(pr, 2, bad, Vs)
    assert rc == 6 and ok == [1, 1, 0, 1, 1]
    assert text.endswith("1 of 5 proofs failed, the first at index 2"), text


def test_undecodable_point_fails_its_proof_alone(small):
    """L_0 of proof 1 of 4 with its top bit set: no field element, so no point."""
    pr, proofs, Vs = small
    bad = list(proofs[:4])
    _xor(bad, 1, 11 * 32 + 31, 0x80)
    assert [pr.verify(bad[i], Vs[i]) for i in range(4)] == [True, False, True, True]
    rc, ok, text = _each_raw(pr, 2, bad, Vs[:4])
    assert rc == 6 and ok == [1, 0, 1, 1]
    assert text.endswith("1 of 4 proofs failed, the first at index 1"), text


def test_edges(batch, ctx):
    import bpperm
    g, pr, proofs, Vs, bp, bv, singles = batch
    assert pr.verify_batch_each([], []) == []
    assert pr.verify_batch_each(proofs[:1], Vs[:1]) == [True]
    assert pr.verify_batch_each(bp[:1], bv[:1]) == [False]
    five = list(proofs[:5])
    for i in range(5):
        _xor(five, i, 8 * 32 + 33, 2)  # mu
    assert [pr.verify(five[i], Vs[i]) for i in range(5)] == [False] * 5
    assert pr.verify_batch_each(five, Vs[:5]) == [False] * 5
    other = bpperm.PermProver(g, K, label=b"another label")
    assert other.verify_batch_each(proofs[:6], Vs[:6]) == [False] * 6
    assert not other.verify(proofs[0], Vs[0])
    # the contiguous-buffer form
    assert pr.verify_batch_each(b"".join(bp), b"".join(bv)) == singles
    with pytest.raises(ValueError):
        pr.verify_batch_each(b"".join(bp)[:-1], b"".join(bv))
    with pytest.raises(ValueError):
        pr.verify_batch_each(b"".join(bp), b"".join(bv)[32:])
    # a generator set longer than the padded circuit: mapped generator slots
    p4 = bpperm.PermProver(g, 4)
    pf, v = p4.prove_batch(list(range(300, 306)))
    plen4 = len(pf[0])
    _xor(pf, 1, 8 * 32 + 70, 1)  # t_hat
    _xor(pf, 4, plen4 - 32, 1)  # b
    ref = [p4.verify(pf[i], v[i]) for i in range(6)]
    assert ref == [True, False, True, True, False, True]
    assert p4.verify_batch_each(pf, v) == ref


def test_passes(batch, ctx, monkeypatch):
    """3 passes of 32, 32 and 6 proofs give the same verdicts; the slow path
    adds count x (NG + npt) terms and one engine launch per pass to what a
    passing call of the same shape issues."""
    _, pr, proofs, Vs, bp, bv, singles = batch

    def delta(p, v):
        w0 = ctx.work()
        got = pr.verify_batch_each(p, v)
        w1 = ctx.work()
        return got, {n: w1[n] - w0[n] for n in w1}

    good, wg = delta(proofs, Vs)
    assert good == [True] * 70
    monkeypatch.setenv("BPP_VERIFY_EACH_PROOFS", "32")
    got, w3 = delta(bp, bv)
    assert got == singles
    assert w3["msm_terms"] - wg["msm_terms"] == 70 * (NG + NPT)
    assert w3["msm_launches"] - wg["msm_launches"] == 3
    monkeypatch.delenv("BPP_VERIFY_EACH_PROOFS")
    got, w1 = delta(bp, bv)
    assert got == singles
    assert w1["msm_terms"] - wg["msm_terms"] == 70 * (NG + NPT)
    assert w1["msm_launches"] - wg["msm_launches"] == 1


def test_fast_path_is_the_batch_verifiers(batch, ctx):
    _, pr, proofs, Vs, *_ = batch
    w0 = ctx.work()
    assert pr.verify_batch(proofs, Vs)
    w1 = ctx.work()
    assert pr.verify_batch_each(proofs, Vs) == [True] * 70
    w2 = ctx.work()
    assert {n: w2[n] - w1[n] for n in w1} == {n: w1[n] - w0[n] for n in w1}
    assert w1["msm_launches"] - w0["msm_launches"] == 1


def test_supersedes_a_device_job(batch, ctx):
    import bpperm
    from bpperm._lib import BppError
    _, pr, proofs, Vs, *_ = batch
    job = bpperm.VerifyJob(K, proofs[:8], Vs[:8], ctx=ctx)
    assert pr.verify_batch_each(proofs[8:16], Vs[8:16]) == [True] * 8
    with pytest.raises(BppError) as e:
        pr.verify_partial(job, bytes(range(32)), 0, 0, job.windows()[1])
    assert e.value.code == 1
    job.close()
