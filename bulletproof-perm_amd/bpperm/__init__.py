"""bpperm — MI355X-native Bulletproof permutation hot path (Python host side).

Thin host mirror of the reference's operator surface over the C ABI in
include/bpperm.h (libbpperm.so, HIP for gfx950):

  vartime_multiscalar_mul(scalars, points)   dalek VartimeMultiscalarMul
                                             (bp-perm/src/circuit_lib.rs:187…568)
  Context.decompress / PointTable.compress   CompressedRistretto::decompress,
                                             RistrettoPoint::compress
  Context.from_uniform                       RistrettoPoint::from_uniform_bytes

Scalars are 32-byte little-endian canonical values mod l; points are 32-byte
compressed ristretto255, exactly dalek's `as_bytes()` forms.  There is no
CPU fallback: without the built library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence

from . import _lib
from ._lib import BppError, check

MSM_INFLIGHT = 4  # BPP_MSM_INFLIGHT (include/bpperm.h)

__all__ = ["Context", "PointTable", "BppError", "vartime_multiscalar_mul", "default_context", "VerifyJob",
           "partials_is_identity", "Circuit", "CircuitProver", "verify_groups", "Reshuffler",
           "MaskedReshuffler"]


def _buf(b: bytes):
    return C.c_char_p(b) if b else None


def _join(items: Iterable[bytes], width: int, what: str) -> bytes:
    if isinstance(items, (bytes, bytearray, memoryview)):
        data = bytes(items)
    else:
        data = b"".join(bytes(x) for x in items)
    if len(data) % width:
        raise ValueError(f"{what}: length {len(data)} not a multiple of {width}")
    return data


class PointTable:
    """A point table resident in HBM (affine Niels, 10-limb field, 128-B rows)."""

    def __init__(self, ctx: "Context", handle: int):
        self._ctx = ctx
        self._h = C.c_void_p(handle)

    def __len__(self) -> int:
        return int(self._ctx.lib.bpp_points_len(self._h))

    @property
    def handle(self):
        return self._h

    def compress(self) -> list[bytes]:
        n = len(self)
        out = C.create_string_buffer(32 * n) if n else None
        check(self._ctx.lib.bpp_points_compress(self._ctx.h, self._h, out), "bpp_points_compress", self._ctx.h)
        raw = out.raw if n else b""
        return [raw[32 * i: 32 * i + 32] for i in range(n)]

    def close(self):
        if self._h:
            self._ctx.lib.bpp_points_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream (bpp_ctx)."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.bpp_ctx_create(device, C.byref(h))
        if rc != 0:
            raise BppError(rc, f"bpp_ctx_create(device={device})")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.bpp_ctx_destroy(self.h)
            self.h = C.c_void_p(0)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self) -> int:
        return int(self.lib.bpp_ctx_stream(self.h) or 0)

    def secret_residue(self) -> int:
        """Nonzero bytes left in what the last production prover batch zeroed
        (bpp_debug_secret_residue; a test hook)."""
        nz = C.c_uint64()
        check(self.lib.bpp_debug_secret_residue(self.h, C.byref(nz)), "bpp_debug_secret_residue", self.h)
        return nz.value

    def circuit_hints(self, circuit, v, pub=None) -> "list[list[bytes]]":
        """The hint kernel alone (bpp_debug_circuit_hints; a test hook): v[p] =
        the m_in inputs of proof p, pub[p] = its n_pub public inputs (32-byte
        scalars, or each proof's joined) -> each proof's n_aux derived values."""
        count = len(v)
        row = lambda rows, what: b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, what) for x in rows)
        vb, ub = row(v, "v"), row(pub, "pub") if pub is not None else b""
        if len(vb) != 32 * circuit.m_in * count or len(ub) != 32 * circuit.n_pub * count:
            raise ValueError("circuit_hints: expected m_in scalars in v and n_pub in pub per proof")
        n = circuit.n_aux
        out = C.create_string_buffer(max(32 * n * count, 1))
        check(self.lib.bpp_debug_circuit_hints(self.h, circuit.h, count, _buf(vb), _buf(ub), out),
              "bpp_debug_circuit_hints", self.h)
        return [[out.raw[32 * (p * n + i):32 * (p * n + i) + 32] for i in range(n)] for p in range(count)]

    def circuit_witness(self, circuit, v, x, pub=None):
        """The witness kernels alone (bpp_debug_circuit_witness; a test hook):
        v[p], pub[p] as circuit_hints takes them, x[p] = proof p's challenge (32
        bytes, the caller's) -> (aL, aR, aO, fail): per proof the n_p 32-byte
        scalars of each vector, and 1 + its first failing assert (0: none)."""
        count = len(v)
        row = lambda rows, what: b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, what) for x in rows)
        vb, ub, xb = row(v, "v"), row(pub, "pub") if pub is not None else b"", b"".join(x)
        if len(vb) != 32 * circuit.m_in * count or len(ub) != 32 * circuit.n_pub * count or len(xb) != 32 * count:
            raise ValueError("circuit_witness: expected m_in scalars in v, n_pub in pub and one x per proof")
        n = circuit.n_p
        outs = [C.create_string_buffer(max(32 * n * count, 1)) for _ in range(3)]
        fail = (C.c_uint32 * max(count, 1))()
        check(self.lib.bpp_debug_circuit_witness(self.h, circuit.h, count, _buf(vb), _buf(ub), _buf(xb), *outs, fail),
              "bpp_debug_circuit_witness", self.h)
        split = lambda o: [[o.raw[32 * (p * n + i):32 * (p * n + i) + 32] for i in range(n)] for p in range(count)]
        return split(outs[0]), split(outs[1]), split(outs[2]), [fail[p] for p in range(count)]

    # ---------------------------------------------------------- profiling
    def profile(self, enable: bool = True):
        check(self.lib.bpp_ctx_profile(self.h, 1 if enable else 0), "bpp_ctx_profile", self.h)

    def profile_get(self, stage: str):
        ms = C.c_double()
        n = C.c_uint64()
        check(self.lib.bpp_ctx_profile_get(self.h, stage.encode(), C.byref(ms), C.byref(n)),
              "bpp_ctx_profile_get", self.h)
        return ms.value, n.value

    def profile_reset(self):
        self.lib.bpp_ctx_profile_reset(self.h)

    WORK_COUNTERS = ("msm_terms", "madds", "padds", "msm_launches", "dt_terms", "dt_madds", "dt_launches",
                     "ipa_dt_terms", "ipa_dt_madds", "ipa_dt_launches")

    def work(self) -> dict:
        """Algorithmic work issued on this context since the last work_reset
        (bpp_ctx_work_get): MSM terms, mixed additions, point additions."""
        out = {}
        for name in self.WORK_COUNTERS:
            v = C.c_uint64()
            check(self.lib.bpp_ctx_work_get(self.h, name.encode(), C.byref(v)), "bpp_ctx_work_get", self.h)
            out[name] = v.value
        return out

    def work_reset(self):
        self.lib.bpp_ctx_work_reset(self.h)

    # ---------------------------------------------------------- device memory
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(self.lib.bpp_dev_alloc(self.h, nbytes, C.byref(p)), "bpp_dev_alloc", self.h)
        return p.value

    def dev_free(self, ptr: int):
        check(self.lib.bpp_dev_free(self.h, C.c_void_p(ptr)), "bpp_dev_free", self.h)

    def htod(self, dptr: int, data: bytes):
        check(self.lib.bpp_memcpy_htod(self.h, C.c_void_p(dptr), _buf(data), len(data)), "bpp_memcpy_htod", self.h)

    def dtoh(self, dptr: int, nbytes: int) -> bytes:
        out = C.create_string_buffer(nbytes)
        check(self.lib.bpp_memcpy_dtoh(self.h, out, C.c_void_p(dptr), nbytes), "bpp_memcpy_dtoh", self.h)
        return out.raw

    def synchronize(self):
        check(self.lib.bpp_synchronize(self.h), "bpp_synchronize", self.h)

    # ---------------------------------------------------------- points
    def decompress(self, encodings) -> PointTable:
        data = _join(encodings, 32, "encodings")
        h = C.c_void_p()
        bad = C.c_size_t()
        check(self.lib.bpp_points_decompress(self.h, _buf(data), len(data) // 32, C.byref(h), C.byref(bad)),
              "bpp_points_decompress", self.h)
        return PointTable(self, h.value)

    def from_uniform(self, bytes64) -> PointTable:
        data = _join(bytes64, 64, "uniform bytes")
        h = C.c_void_p()
        check(self.lib.bpp_points_from_uniform(self.h, _buf(data), len(data) // 64, C.byref(h)),
              "bpp_points_from_uniform", self.h)
        return PointTable(self, h.value)

    # ---------------------------------------------------------- MSM
    def msm(self, scalars, points) -> bytes:
        """vartime_multiscalar_mul over host scalars and compressed points."""
        s = _join(scalars, 32, "scalars")
        p = _join(points, 32, "points")
        if len(s) // 32 != len(p) // 32:
            raise BppError(2, "bpp_msm", "scalar/point count mismatch")
        out = C.create_string_buffer(32)
        check(self.lib.bpp_msm(self.h, _buf(s), _buf(p), len(s) // 32, out), "bpp_msm", self.h)
        return out.raw

    def msm_table(self, scalars, table: PointTable, n: int | None = None) -> bytes:
        s = _join(scalars, 32, "scalars")
        n = len(s) // 32 if n is None else n
        out = C.create_string_buffer(32)
        check(self.lib.bpp_msm_table(self.h, _buf(s), table.handle, n, out), "bpp_msm_table", self.h)
        return out.raw

    def msm_table_dev(self, d_scalars: int, table: PointTable, n: int) -> bytes:
        out = C.create_string_buffer(32)
        check(self.lib.bpp_msm_table_dev(self.h, C.c_void_p(d_scalars), table.handle, n, out),
              "bpp_msm_table_dev", self.h)
        return out.raw

    def msm_table_dev_partial(self, d_scalars: int, table: PointTable, n: int, w_begin: int, w_end: int) -> bytes:
        out = C.create_string_buffer(128)
        check(self.lib.bpp_msm_table_dev_partial(self.h, C.c_void_p(d_scalars), table.handle, n, w_begin, w_end, out),
              "bpp_msm_table_dev_partial", self.h)
        return out.raw

    # Asynchronous single MSMs (at most two in flight): submit returns a
    # ticket at once; collect waits for it and returns the compressed result
    # (or the raw 128-byte partial of windows [w_begin, w_end)).
    def msm_submit(self, d_scalars: int, table: PointTable, n: int, w_begin: int = 0, w_end: int = 0) -> int:
        t = C.c_uint64()
        check(self.lib.bpp_msm_submit(self.h, C.c_void_p(d_scalars), table.handle, n, w_begin, w_end, C.byref(t)),
              "bpp_msm_submit", self.h)
        return t.value

    def msm_submit_host(self, h_scalars, table: PointTable, n: int, w_begin: int = 0, w_end: int = 0) -> int:
        """As msm_submit with host scalars: a pinned buffer address from
        host_alloc (int; direct DMA on the MSM's stream) or bytes (staged)."""
        t = C.c_uint64()
        ptr = C.c_void_p(h_scalars) if isinstance(h_scalars, int) else _buf(h_scalars)
        check(self.lib.bpp_msm_submit_host(self.h, ptr, table.handle, n, w_begin, w_end, C.byref(t)),
              "bpp_msm_submit_host", self.h)
        return t.value

    def host_alloc(self, nbytes: int) -> int:
        """Pinned host memory (bpp_host_alloc); free with host_free."""
        p = C.c_void_p()
        check(self.lib.bpp_host_alloc(self.h, nbytes, C.byref(p)), "bpp_host_alloc", self.h)
        return p.value

    def host_free(self, ptr: int):
        check(self.lib.bpp_host_free(self.h, C.c_void_p(ptr)), "bpp_host_free", self.h)

    def msm_collect(self, ticket: int, partial: bool = False) -> bytes:
        out = C.create_string_buffer(128 if partial else 32)
        args = (None, out) if partial else (out, None)
        check(self.lib.bpp_msm_collect(self.h, ticket, *args), "bpp_msm_collect", self.h)
        return out.raw

    def msm_batch(self, offsets: Sequence[int], scalars, point_idx: Sequence[int], table: PointTable) -> list[bytes]:
        count = len(offsets) - 1
        s = _join(scalars, 32, "scalars")
        off = (C.c_uint64 * len(offsets))(*offsets)
        idx = (C.c_uint32 * max(1, len(point_idx)))(*point_idx)
        out = C.create_string_buffer(32 * max(count, 1))
        check(self.lib.bpp_msm_batch(self.h, count, off, _buf(s), idx, table.handle, out), "bpp_msm_batch", self.h)
        raw = out.raw  # .raw copies the whole buffer on every access
        return [raw[32 * i: 32 * i + 32] for i in range(count)]


def host_tuning(malloc: bool = True, hw_queues: bool = False):
    """Opt-in process-wide host tuning (bpp_host_tuning): BPP_TUNE_MALLOC
    fixes glibc's mmap threshold and disables heap trimming (the prover's
    per-batch host vectors stay in the arenas); BPP_TUNE_HW_QUEUES asks HIP
    for 8 hardware queues (GPU_MAX_HW_QUEUES=8 unless set; effective only
    before anything in the process initialises HIP)."""
    check(_lib.load().bpp_host_tuning((1 if malloc else 0) | (2 if hw_queues else 0)), "bpp_host_tuning")


def host_pool_threads() -> int:
    """Threads of the library's host pool (bpp_host_threads)."""
    return int(_lib.load().bpp_host_threads())


def msm_windows(n: int) -> tuple[int, int]:
    lib = _lib.load()
    c = C.c_uint32()
    w = C.c_uint32()
    lib.bpp_msm_windows(n, C.byref(c), C.byref(w))
    return c.value, w.value


def double_compress(raw_points: Sequence[bytes]) -> list[bytes]:
    """compress(2 P) for raw 128-byte extended points (host batch encoding)."""
    lib = _lib.load()
    data = b"".join(raw_points)
    out = C.create_string_buffer(32 * len(raw_points))
    check(lib.bpp_points_double_compress(_buf(data), len(raw_points), out), "bpp_points_double_compress")
    return [out.raw[32 * i:32 * i + 32] for i in range(len(raw_points))]


def partials_finish(partials: Sequence[bytes]) -> bytes:
    lib = _lib.load()
    data = b"".join(partials)
    out = C.create_string_buffer(32)
    check(lib.bpp_partials_finish(_buf(data), len(partials), out), "bpp_partials_finish")
    return out.raw


_default: Context | None = None


def default_context() -> Context:
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def vartime_multiscalar_mul(scalars, points) -> bytes:
    """`RistrettoPoint::vartime_multiscalar_mul(scalars, points).compress()`."""
    return default_context().msm(scalars, points)


# ------------------------------------------------------------------ protocol
class Transcript:
    """merlin 3.0.0 `Transcript` on the host side of libbpperm (byte-exact;
    transcript_protocol.rs TranscriptProtocol helpers included)."""

    def __init__(self, label: bytes = b"", _handle=None):
        self.lib = _lib.load()
        self.h = C.c_void_p(_handle) if _handle else C.c_void_p(self.lib.bpp_transcript_new(_buf(label), len(label)))

    def clone(self) -> "Transcript":
        return Transcript(_handle=self.lib.bpp_transcript_clone(self.h))

    def close(self):
        if self.h:
            self.lib.bpp_transcript_destroy(self.h)
            self.h = C.c_void_p(0)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def append_message(self, label: bytes, msg: bytes):
        check(self.lib.bpp_transcript_append_message(self.h, _buf(label), len(label), _buf(msg), len(msg)),
              "append_message")

    def append_u64(self, label: bytes, x: int):
        check(self.lib.bpp_transcript_append_u64(self.h, _buf(label), len(label), x), "append_u64")

    def challenge_bytes(self, label: bytes, n: int) -> bytes:
        out = C.create_string_buffer(n)
        check(self.lib.bpp_transcript_challenge_bytes(self.h, _buf(label), len(label), out, n), "challenge_bytes")
        return out.raw

    def challenge_scalar(self, label: bytes) -> bytes:
        out = C.create_string_buffer(32)
        check(self.lib.bpp_transcript_challenge_scalar(self.h, _buf(label), len(label), out), "challenge_scalar")
        return out.raw

    # TranscriptProtocol (transcript_protocol.rs)
    def arithmetic_domain_sep(self, n: int):
        self.append_message(b"dom-sep", b"acp v1")
        self.append_u64(b"n", n)

    def append_scalar(self, label: bytes, s: bytes):
        self.append_message(label, s)

    def append_point(self, label: bytes, p: bytes):
        self.append_message(label, p)


# bpp_transcript_hooks (include/bpperm.h): the caller's transcript behind C hooks
_APPEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_ubyte), C.c_size_t)
_CHALLENGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_ubyte), C.c_size_t, C.POINTER(C.c_ubyte), C.c_size_t)


class _Hooks(C.Structure):
    _fields_ = [("user", C.c_void_p), ("append_message", _APPEND_FN), ("challenge_bytes", _CHALLENGE_FN)]


def transcript_hooks(tr):
    """bpp_transcript_hooks over any object with merlin's two primitives,
    `append_message(label, msg)` and `challenge_bytes(label, n) -> bytes`
    (the caller keeps its own transcript, bpp_ipa_prove_cb).  An exception in
    a hook is kept on the returned object (`.error`) and reported to the
    library as a failed hook (BPP_ERR_CALLBACK)."""

    class _H:
        error = None

    h = _H()

    def _append(_u, lab, ll, msg, ml):
        try:
            tr.append_message(C.string_at(lab, ll), C.string_at(msg, ml) if ml else b"")
            return 0
        except Exception as e:  # noqa: BLE001 (reported through BPP_ERR_CALLBACK)
            h.error = e
            return 1

    def _challenge(_u, lab, ll, out, n):
        try:
            b = tr.challenge_bytes(C.string_at(lab, ll), n)
            if len(b) != n:
                raise ValueError("challenge_bytes returned %d bytes, wanted %d" % (len(b), n))
            C.memmove(out, b, n)
            return 0
        except Exception as e:  # noqa: BLE001
            h.error = e
            return 1

    h.fa, h.fc = _APPEND_FN(_append), _CHALLENGE_FN(_challenge)  # (kept alive with h)
    h.s = _Hooks(None, h.fa, h.fc)
    return h


def _tr_args(tr, lib, plain: str):
    """(function, transcript argument, hooks holder) for a library Transcript
    (bpp_transcript*) or a caller-owned one (hooks)."""
    if isinstance(tr, Transcript):
        return getattr(lib, plain), tr.h, None
    h = transcript_hooks(tr)
    return getattr(lib, plain + "_cb"), C.byref(h.s), h


class Gens:
    """BulletproofGens(n, 1) + PedersenGens resident on the GPU (bpp_gens)."""

    def __init__(self, ctx: Context, n: int | None = None, points=None):
        self.ctx = ctx
        h = C.c_void_p()
        if points is None:
            check(ctx.lib.bpp_gens_create(ctx.h, n, C.byref(h)), "bpp_gens_create", ctx.h)
        else:
            G, H, B, Bb = points
            g = _join(G, 32, "G")
            hh = _join(H, 32, "H")
            check(ctx.lib.bpp_gens_from_points(ctx.h, _buf(g), _buf(hh), len(g) // 32, _buf(B), _buf(Bb),
                                               C.byref(h)), "bpp_gens_from_points", ctx.h)
        self.h = h

    def __len__(self):
        return int(self.ctx.lib.bpp_gens_len(self.h))

    def export(self):
        n = len(self)
        out = C.create_string_buffer(32 * (2 * n + 2))
        check(self.ctx.lib.bpp_gens_export(self.ctx.h, self.h, out), "bpp_gens_export", self.ctx.h)
        raw = out.raw
        pts = [raw[32 * i: 32 * i + 32] for i in range(2 * n + 2)]
        return pts[:n], pts[n: 2 * n], pts[2 * n], pts[2 * n + 1]

    def close(self):
        if self.h:
            self.ctx.lib.bpp_gens_destroy(self.h)
            self.h = C.c_void_p(0)

    def pedersen_commit(self, v, gamma) -> list[bytes]:
        """PedersenGens::commit over a batch (weights.rs:58-61)."""
        vb = _join(v, 32, "v")
        gb = _join(gamma, 32, "gamma")
        m = len(vb) // 32
        if len(gb) // 32 != m:
            raise BppError(2, "bpp_pedersen_commit_batch", "length mismatch")
        out = C.create_string_buffer(32 * max(m, 1))
        check(self.ctx.lib.bpp_pedersen_commit_batch(self.ctx.h, self.h, _buf(vb), _buf(gb), m, out),
              "bpp_pedersen_commit_batch", self.ctx.h)
        raw = out.raw
        return [raw[32 * i: 32 * i + 32] for i in range(m)]

    def vec_commit(self, blind: bytes, a, b=None) -> bytes:
        ab = _join(a, 32, "a")
        bb = _join(b, 32, "b") if b is not None else None
        out = C.create_string_buffer(32)
        check(self.ctx.lib.bpp_vec_commit(self.ctx.h, self.h, _buf(blind), _buf(ab), _buf(bb) if bb else None,
                                          len(ab) // 32, out), "bpp_vec_commit", self.ctx.h)
        return out.raw

    def ipa_prove(self, tr, Q: bytes, G_factors, H_factors, a, b):
        """InnerProductProof::create -> (L list, R list, a, b).  `tr`: a
        bpperm.Transcript, or the caller's own transcript object (merlin's
        append_message / challenge_bytes; bpp_ipa_prove_cb)."""
        ab, bb = _join(a, 32, "a"), _join(b, 32, "b")
        n = len(ab) // 32
        gf = _join(G_factors, 32, "G_factors") if G_factors is not None else None
        hf = _join(H_factors, 32, "H_factors") if H_factors is not None else None
        lg = max(n.bit_length() - 1, 0)
        Lo = C.create_string_buffer(32 * max(lg, 1))
        Ro = C.create_string_buffer(32 * max(lg, 1))
        ao, bo = C.create_string_buffer(32), C.create_string_buffer(32)
        fn, targ, hooks = _tr_args(tr, self.ctx.lib, "bpp_ipa_prove")
        rc = fn(self.ctx.h, self.h, targ, _buf(Q), _buf(gf) if gf else None, _buf(hf) if hf else None, _buf(ab),
                _buf(bb), n, Lo, Ro, ao, bo)
        if hooks is not None and hooks.error is not None:
            raise hooks.error
        check(rc, "bpp_ipa_prove", self.ctx.h)
        lraw, rraw = Lo.raw, Ro.raw
        return ([lraw[32 * i: 32 * i + 32] for i in range(lg)], [rraw[32 * i: 32 * i + 32] for i in range(lg)],
                ao.raw, bo.raw)

    def ipa_verify(self, tr, n: int, G_factors, H_factors, P: bytes, Q: bytes, L, R, a: bytes,
                   b: bytes) -> bool:
        gf = _join(G_factors, 32, "G_factors") if G_factors is not None else None
        hf = _join(H_factors, 32, "H_factors") if H_factors is not None else None
        fn, targ, hooks = _tr_args(tr, self.ctx.lib, "bpp_ipa_verify")
        rc = fn(self.ctx.h, self.h, targ, n, _buf(gf) if gf else None, _buf(hf) if hf else None, _buf(P), _buf(Q),
                _buf(b"".join(L)), _buf(b"".join(R)), _buf(a), _buf(b))
        if hooks is not None and hooks.error is not None:
            raise hooks.error
        if rc == 6:
            return False
        check(rc, "bpp_ipa_verify", self.ctx.h)
        return True


class PermProver:
    """Permutation proof over resident generators — the sound-mode restatement
    of ACProof::ArithmeticCircuitProof (circuit_lib.rs:139-585)."""

    def __init__(self, gens: Gens, k: int, label: bytes = b"bp-perm", ctx: "Context | None" = None):
        """ctx: the context (stream, workspaces) proofs run on; default the
        generators' own.  One generator set may serve several contexts, e.g.
        one per host thread with batches in flight."""
        self.gens = gens
        self.ctx = ctx or gens.ctx
        self.k = k
        self.label = label
        self.proof_len = int(self.ctx.lib.bpp_perm_proof_len(k))
        self.m = 2 * k + 1

    def prove(self, seed: int):
        """-> (proof bytes, [V_j], permutation)"""
        pf = C.create_string_buffer(self.proof_len)
        V = C.create_string_buffer(32 * self.m)
        perm = (C.c_uint32 * self.k)()
        check(self.ctx.lib.bpp_perm_prove(self.ctx.h, self.gens.h, self.k, seed, _buf(self.label), len(self.label),
                                          pf, V, perm), "bpp_perm_prove", self.ctx.h)
        vraw = V.raw
        return pf.raw, [vraw[32 * j: 32 * j + 32] for j in range(self.m)], list(perm)

    def prove_batch(self, seeds: Sequence[int], raw: bool = False):
        """-> ([proof bytes], [V bytes of one proof]), or with raw=True the
        two contiguous buffers (proofs, V) as the C ABI writes them (what
        verify_batch takes without a join)."""
        cnt = len(seeds)
        pf = C.create_string_buffer(self.proof_len * cnt)
        V = C.create_string_buffer(32 * self.m * cnt)
        sd = (C.c_uint64 * cnt)(*seeds)
        check(self.ctx.lib.bpp_perm_prove_batch(self.ctx.h, self.gens.h, self.k, cnt, sd, _buf(self.label),
                                                len(self.label), pf, V), "bpp_perm_prove_batch", self.ctx.h)
        praw, vraw = pf.raw, V.raw
        if raw:
            return praw, vraw
        return ([praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(cnt)],
                [vraw[i * 32 * self.m:(i + 1) * 32 * self.m] for i in range(cnt)])

    def prove_batch_entropy(self, count: int, seeds32: bytes | None = None, raw: bool = False):
        """Production proving: 32 bytes of entropy per proof (seeds32) or,
        when None, from the OS CSPRNG (bpp_perm_prove_batch_entropy); the
        batch's secrets are wiped before it returns.  raw=True: the two
        contiguous buffers (proofs, V), as prove_batch(..., raw=True)."""
        if seeds32 is not None and len(seeds32) != 32 * count:
            raise ValueError("seeds32 must hold 32 bytes per proof")
        pf = C.create_string_buffer(self.proof_len * count)
        V = C.create_string_buffer(32 * self.m * count)
        check(self.ctx.lib.bpp_perm_prove_batch_entropy(self.ctx.h, self.gens.h, self.k, count, _buf(seeds32 or b""),
                                                        _buf(self.label), len(self.label), pf, V),
              "bpp_perm_prove_batch_entropy", self.ctx.h)
        praw, vraw = pf.raw, V.raw
        if raw:
            return praw, vraw
        return ([praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(count)],
                [vraw[i * 32 * self.m:(i + 1) * 32 * self.m] for i in range(count)])

    def prove_shuffle_batch(self, cards, perms, seeds32: bytes | None = None, gammas=None, raw: bool = False):
        """Proves caller-supplied shuffles (bpp_perm_prove_shuffle_batch):
        cards[p] = the k canonical 32-byte scalars of proof p's deck (or their
        32 k bytes joined), perms[p] = k indices, output slot i holding
        cards[p][perms[p][i]]; gammas[p] = the 2k blindings of V_0..V_2k-1
        (None: drawn); seeds32 = 32 bytes per proof (None: the OS CSPRNG).
        Returns what prove_batch returns; the batch's secrets are wiped."""
        count = len(cards)
        if len(perms) != count or (gammas is not None and len(gammas) != count):
            raise ValueError("cards, perms and gammas must have one entry per proof")
        if seeds32 is not None and len(seeds32) != 32 * count:
            raise ValueError("seeds32 must hold 32 bytes per proof")

        def rows(items, n, what):
            out = b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, what) for x in items)
            if len(out) != 32 * n * count:
                raise ValueError(f"{what}: expected {n} scalars of 32 bytes per proof")
            return out

        cb = rows(cards, self.k, "cards")
        gb = rows(gammas, 2 * self.k, "gammas") if gammas is not None else None
        flat = [int(i) for p in perms for i in p]
        if len(flat) != self.k * count:
            raise ValueError("perms: expected k indices per proof")
        pm = (C.c_uint32 * len(flat))(*flat)
        pf = C.create_string_buffer(self.proof_len * count)
        V = C.create_string_buffer(32 * self.m * count)
        check(self.ctx.lib.bpp_perm_prove_shuffle_batch(self.ctx.h, self.gens.h, self.k, count, _buf(cb), pm,
                                                        _buf(gb) if gb is not None else None,
                                                        _buf(seeds32) if seeds32 is not None else None,
                                                        _buf(self.label), len(self.label), pf, V),
              "bpp_perm_prove_shuffle_batch", self.ctx.h)
        praw, vraw = pf.raw, V.raw
        if raw:
            return praw, vraw
        return ([praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(count)],
                [vraw[i * 32 * self.m:(i + 1) * 32 * self.m] for i in range(count)])

    def verify(self, proof: bytes, V) -> bool:
        vb = _join(V, 32, "V")
        rc = self.ctx.lib.bpp_perm_verify(self.ctx.h, self.gens.h, self.k, _buf(self.label), len(self.label),
                                          _buf(proof), len(proof), _buf(vb))
        if rc == 6:
            return False
        check(rc, "bpp_perm_verify", self.ctx.h)
        return True

    def _batch_buffers(self, proofs, Vs):
        """verify_batch's two input forms -> (proof bytes, V bytes, count)."""
        if isinstance(proofs, (bytes, bytearray)):
            pb, vb = bytes(proofs), bytes(Vs)
            count = len(pb) // self.proof_len
            if len(pb) != count * self.proof_len or len(vb) != count * 32 * self.m:
                raise ValueError("contiguous proofs / V buffers of inconsistent length")
            return pb, vb, count
        return b"".join(proofs), b"".join(Vs), len(proofs)

    def verify_batch(self, proofs, Vs) -> bool:
        """proofs / Vs: sequences of per-proof bytes, or the two contiguous
        buffers (prove_batch(..., raw=True))."""
        pb, vb, count = self._batch_buffers(proofs, Vs)
        rc = self.ctx.lib.bpp_perm_verify_batch(self.ctx.h, self.gens.h, self.k, count, _buf(self.label),
                                                len(self.label), _buf(pb), _buf(vb))
        if rc == 6:
            return False
        check(rc, "bpp_perm_verify_batch", self.ctx.h)
        return True

    def verify_batch_each(self, proofs, Vs) -> "list[bool]":
        """verify_batch that names the failing proofs: one verdict per proof,
        what verify(proofs[i], Vs[i]) returns (bpp_perm_verify_batch_each; a
        batch that passes costs what verify_batch costs).  Inputs as
        verify_batch."""
        pb, vb, count = self._batch_buffers(proofs, Vs)
        ok = C.create_string_buffer(max(count, 1))
        rc = self.ctx.lib.bpp_perm_verify_batch_each(self.ctx.h, self.gens.h, self.k, count, _buf(self.label),
                                                     len(self.label), _buf(pb), _buf(vb), ok)
        if rc != 6:
            check(rc, "bpp_perm_verify_batch_each", self.ctx.h)
        return [b != 0 for b in ok.raw[:count]]

    def verify_batch_ptr(self, proofs_ptr: int, V_ptr: int, count: int) -> bool:
        """verify_batch over `count` proofs and their V already in host
        memory at two addresses -- e.g. pinned buffers from
        Context.host_alloc, which go up by DMA without the staging copy."""
        rc = self.ctx.lib.bpp_perm_verify_batch(self.ctx.h, self.gens.h, self.k, count, _buf(self.label),
                                                len(self.label), C.c_void_p(proofs_ptr), C.c_void_p(V_ptr))
        if rc == 6:
            return False
        check(rc, "bpp_perm_verify_batch", self.ctx.h)
        return True

    def verify_job(self, proofs: Sequence[bytes], Vs: Sequence[bytes], device: bool = True) -> "VerifyJob":
        """Replay phase of a batch verification that may be split over GPUs:
        on this prover's context (device=True, bpp_perm_verify_begin_dev) or
        on the host (bpp_perm_verify_begin)."""
        return VerifyJob(self.k, proofs, Vs, self.label, ctx=self.ctx if device else None)

    def verify_partial_sharded(self, job: "VerifyJob", first: int, d_blocks: int, stride: int, d_pblocks: int,
                               pstride: int, counts: Sequence[int], w_begin: int, w_end: int) -> bytes:
        """128-B raw partial of the whole batch's MSM over windows [w_begin,
        w_end), from every slice's scalar block (d_blocks + s * stride) and
        decompressed point block (d_pblocks + s * pstride) gathered in slice
        order; job = this rank's job over its own slice, batch proofs [first,
        first + job.count) (bpp_perm_verify_partial_sharded)."""
        part = C.create_string_buffer(128)
        cn = (C.c_size_t * max(len(counts), 1))(*counts)
        check(self.ctx.lib.bpp_perm_verify_partial_sharded(self.ctx.h, self.gens.h, job.h, first, d_blocks, stride,
                                                           d_pblocks, pstride, cn, len(counts), w_begin, w_end, part),
              "bpp_perm_verify_partial_sharded", self.ctx.h)
        return part.raw

    def verify_partial(self, job: "VerifyJob", seed: bytes, first: int, w_begin: int, w_end: int) -> bytes:
        """128-B raw partial of job's MSM over windows [w_begin, w_end) (see
        bpp_perm_verify_partial); seed = the batch's 32 verifier-random bytes
        (verify_seed(), the same on every rank), first = the batch index of
        the job's first proof.  None when a proof point does not decode
        (BPP_ERR_VERIFY)."""
        part = C.create_string_buffer(128)
        rc = self.ctx.lib.bpp_perm_verify_partial(self.ctx.h, self.gens.h, job.h, _seed(seed), first, w_begin, w_end,
                                                  part)
        if rc == 6:  # a proof point that does not decode: the batch cannot verify
            return None
        check(rc, "bpp_perm_verify_partial", self.ctx.h)
        return part.raw



class DeckProver:
    """Public-deck shuffle proof (bpp_deck_*): V_0..V_{k-1} commit to a
    permutation of the PUBLIC deck, V_k to the transcript challenge -- k + 1
    commitments and k - 1 gates where PermProver's two-half statement takes
    2k + 1 and 2k.  deck: None (the cards 1..k) or k canonical 32-byte scalars
    (or their 32 k bytes joined), shared by every proof."""

    def __init__(self, gens: Gens, k: int, deck=None, label: bytes = b"bp-perm", ctx: "Context | None" = None):
        self.gens = gens
        self.ctx = ctx or gens.ctx
        self.k = k
        self.label = label
        if deck is not None:
            deck = bytes(deck) if isinstance(deck, (bytes, bytearray)) else _join(deck, 32, "deck")
            if len(deck) != 32 * k:
                raise ValueError("deck: expected k scalars of 32 bytes")
        self.deck = deck
        self.proof_len = int(self.ctx.lib.bpp_deck_proof_len(k))
        self.m = k + 1

    def _deck(self):
        return _buf(self.deck) if self.deck is not None else None

    def prove_batch(self, perms, seeds32: bytes | None = None, gammas=None, raw: bool = False):
        """perms[p] = k indices, V_i of proof p committing to deck[perms[p][i]];
        gammas[p] = the k blindings of V_0..V_{k-1} (None: drawn); seeds32 = 32
        bytes per proof (None: the OS CSPRNG).  Returns what
        PermProver.prove_batch returns; the batch's secrets are wiped."""
        count = len(perms)
        if gammas is not None and len(gammas) != count:
            raise ValueError("perms and gammas must have one entry per proof")
        if seeds32 is not None and len(seeds32) != 32 * count:
            raise ValueError("seeds32 must hold 32 bytes per proof")
        gb = None
        if gammas is not None:
            gb = b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, "gammas") for x in gammas)
            if len(gb) != 32 * self.k * count:
                raise ValueError("gammas: expected k scalars of 32 bytes per proof")
        flat = [int(i) for p in perms for i in p]
        if len(flat) != self.k * count:
            raise ValueError("perms: expected k indices per proof")
        pm = (C.c_uint32 * max(len(flat), 1))(*flat)
        pf = C.create_string_buffer(max(self.proof_len * count, 1))
        V = C.create_string_buffer(max(32 * self.m * count, 1))
        check(self.ctx.lib.bpp_deck_prove_batch(self.ctx.h, self.gens.h, self.k, count, self._deck(), pm,
                                                _buf(gb) if gb is not None else None,
                                                _buf(seeds32) if seeds32 is not None else None,
                                                _buf(self.label), len(self.label), pf, V),
              "bpp_deck_prove_batch", self.ctx.h)
        praw, vraw = pf.raw[:self.proof_len * count], V.raw[:32 * self.m * count]
        if raw:
            return praw, vraw
        return ([praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(count)],
                [vraw[i * 32 * self.m:(i + 1) * 32 * self.m] for i in range(count)])

    def verify(self, proof: bytes, V) -> bool:
        vb = _join(V, 32, "V")
        rc = self.ctx.lib.bpp_deck_verify(self.ctx.h, self.gens.h, self.k, self._deck(), _buf(self.label),
                                          len(self.label), _buf(proof), len(proof), _buf(vb))
        if rc == 6:
            return False
        check(rc, "bpp_deck_verify", self.ctx.h)
        return True

    _batch_buffers = PermProver._batch_buffers

    def verify_batch(self, proofs, Vs) -> bool:
        """proofs / Vs: sequences of per-proof bytes, or the two contiguous
        buffers (prove_batch(..., raw=True))."""
        pb, vb, count = self._batch_buffers(proofs, Vs)
        rc = self.ctx.lib.bpp_deck_verify_batch(self.ctx.h, self.gens.h, self.k, count, self._deck(),
                                                _buf(self.label), len(self.label), _buf(pb), _buf(vb))
        if rc == 6:
            return False
        check(rc, "bpp_deck_verify_batch", self.ctx.h)
        return True

    def verify_batch_each(self, proofs, Vs) -> "list[bool]":
        """One verdict per proof, what verify(proofs[i], Vs[i]) returns
        (bpp_deck_verify_batch_each).  Inputs as verify_batch."""
        pb, vb, count = self._batch_buffers(proofs, Vs)
        ok = C.create_string_buffer(max(count, 1))
        rc = self.ctx.lib.bpp_deck_verify_batch_each(self.ctx.h, self.gens.h, self.k, count, self._deck(),
                                                     _buf(self.label), len(self.label), _buf(pb), _buf(vb), ok)
        if rc != 6:
            check(rc, "bpp_deck_verify_batch_each", self.ctx.h)
        return [b != 0 for b in ok.raw[:count]]


class _Reshuffle:
    """What the two kinds of re-shuffle proof share: every call, over the
    kind's export-name stem, the bytes of one card, the text that refuses cards
    of another size, and the leading key argument (none, or the key)."""
    _stem = ""       # bpp_<..>_prove_batch, .._verify, ..
    _card = 0        # bytes per card
    _card_what = ""  # "expected ..": what _cards refuses with
    _key = ()        # the exports' key argument: none, or (key,)

    def __init__(self, gens: Gens, k: int, label: bytes = b"bp-perm", ctx: "Context | None" = None):
        self.gens = gens
        self.ctx = ctx or gens.ctx
        self.k = k
        self.label = label
        self.proof_len = int(getattr(self.ctx.lib, self._stem + "_proof_len")(k))

    def _call(self, name: str, *args) -> "tuple[int, str]":
        """bpp_<stem>_<name>(ctx, gens, k, ..): its return code, and the export's name"""
        name = f"{self._stem}_{name}"
        return getattr(self.ctx.lib, name)(self.ctx.h, self.gens.h, self.k, *args), name

    def _verdict(self, rc: int, name: str) -> bool:
        if rc == 6:
            return False
        check(rc, name, self.ctx.h)
        return True

    def _cards(self, cards, count: int, what: str) -> bytes:
        cb = bytes(cards) if isinstance(cards, (bytes, bytearray)) else b"".join(_join(c, 32, what) for c in cards)
        if len(cb) != self._card * self.k * count:
            raise ValueError(f"{what}: {self._card_what}")
        return cb

    def shuffle_batch(self, cards_in, perms, blinds=None, seeds32: bytes | None = None, raw: bool = False):
        """cards_in[p] = the k input cards of shuffle p (joined, or their
        32-byte encodings in order); perms[p] = k indices, output slot i holding
        input perms[p][i]; blinds[p] = the k scalars r_i (None: drawn); seeds32
        = 32 bytes per proof (None: the OS CSPRNG).  Returns (cards_out,
        proofs): per shuffle the k output cards joined and the proof (raw=True:
        the two contiguous buffers).  The batch's secrets are wiped."""
        count = len(perms)
        if blinds is not None and len(blinds) != count:
            raise ValueError("perms and blinds must have one entry per proof")
        if seeds32 is not None and len(seeds32) != 32 * count:
            raise ValueError("seeds32 must hold 32 bytes per proof")
        cb = self._cards(cards_in, count, "cards_in")
        bb = None
        if blinds is not None:
            bb = b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, "blinds") for x in blinds)
            if len(bb) != 32 * self.k * count:
                raise ValueError("blinds: expected k scalars of 32 bytes per proof")
        flat = [int(i) for p in perms for i in p]
        if len(flat) != self.k * count:
            raise ValueError("perms: expected k indices per proof")
        pm = (C.c_uint32 * max(len(flat), 1))(*flat)
        deck = self._card * self.k
        out = C.create_string_buffer(max(deck * count, 1))
        pf = C.create_string_buffer(max(self.proof_len * count, 1))
        rc, name = self._call("prove_batch", count, *self._key, _buf(cb), pm, _buf(bb) if bb is not None else None,
                              _buf(seeds32) if seeds32 is not None else None, _buf(self.label), len(self.label), out, pf)
        check(rc, name, self.ctx.h)
        oraw, praw = out.raw[:deck * count], pf.raw[:self.proof_len * count]
        if raw:
            return oraw, praw
        return ([oraw[i * deck:(i + 1) * deck] for i in range(count)],
                [praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(count)])

    def verify(self, cards_in, cards_out, proof: bytes) -> bool:
        ci, co = self._cards(cards_in, 1, "cards_in"), self._cards(cards_out, 1, "cards_out")
        return self._verdict(*self._call("verify", *self._key, _buf(self.label), len(self.label), _buf(ci), _buf(co),
                                         _buf(proof), len(proof)))

    def _batch(self, cards_in, cards_out, proofs):
        pb = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(proofs)
        if self.proof_len == 0 or len(pb) % self.proof_len:
            raise ValueError("proofs: not a whole number of proofs")
        count = len(pb) // self.proof_len
        return self._cards(cards_in, count, "cards_in"), self._cards(cards_out, count, "cards_out"), pb, count

    def verify_batch(self, cards_in, cards_out, proofs) -> bool:
        """cards_in / cards_out / proofs: sequences with one entry per proof, or
        the contiguous buffers (shuffle_batch(..., raw=True))."""
        ci, co, pb, count = self._batch(cards_in, cards_out, proofs)
        return self._verdict(*self._call("verify_batch", count, *self._key, _buf(self.label), len(self.label), _buf(ci),
                                         _buf(co), _buf(pb)))

    def verify_batch_each(self, cards_in, cards_out, proofs) -> "list[bool]":
        """One verdict per proof, what verify() returns for it alone (the
        kind's .._verify_batch_each).  Inputs as verify_batch."""
        ci, co, pb, count = self._batch(cards_in, cards_out, proofs)
        ok = C.create_string_buffer(max(count, 1))
        rc, name = self._call("verify_batch_each", count, *self._key, _buf(self.label), len(self.label), _buf(ci),
                              _buf(co), _buf(pb), ok)
        if rc != 6:
            check(rc, name, self.ctx.h)
        return [b != 0 for b in ok.raw[:count]]


class Reshuffler(_Reshuffle):
    """Blind re-shuffle proof (bpp_reshuffle_*): the output cards are a
    permutation of the input cards, each re-blinded with a multiple of
    B_blinding, and the prover opens none of them -- the step of a card game in
    which a second player shuffles a deck that the first one committed.  A card
    is a 32-byte ristretto255 encoding; 2 <= k <= 342, and gens covers
    max(4, next_pow2(2k - 2))."""
    _stem, _card, _card_what = "bpp_reshuffle", 32, "expected k encodings of 32 bytes per proof"


class MaskedReshuffler(_Reshuffle):
    """Masked re-shuffle proof (bpp_masked_reshuffle_*): the blind re-shuffle
    over ElGamal pairs under a table's joint key, the shuffle a game can deal
    cards from.  A card is 64 bytes, U | W = (rho B, M + rho K); the output
    cards are a permutation of the input cards, each re-masked with (r B, r K)
    under one r.  The open deck is 32 zero bytes and the card's public point per
    card and needs no proof.  key: K, 32 bytes; 2 <= k <= 342, and gens covers
    max(4, next_pow2(2k - 2)).  A shuffle's input cards are 64 bytes each, or
    the 2k encodings U_0, W_0, U_1, ..; its output cards come joined, 64 k
    bytes."""
    _stem, _card, _card_what = "bpp_masked_reshuffle", 64, "expected k cards of 64 bytes (U | W) per proof"

    def __init__(self, gens: Gens, k: int, key: bytes, label: bytes = b"bp-perm", ctx: "Context | None" = None):
        if len(key) != 32:
            raise ValueError("key: expected one 32-byte encoding")
        super().__init__(gens, k, label, ctx)
        self.key = bytes(key)
        self._key = (_buf(self.key),)


class _CircuitDescC(C.Structure):
    _fields_ = [("m_in", C.c_uint32), ("n_gates", C.c_uint32), ("n_aux", C.c_uint32), ("n_asserts", C.c_uint32),
                ("side_aux", C.POINTER(C.c_uint32)), ("lc_off", C.POINTER(C.c_uint32)),
                ("lc_var", C.POINTER(C.c_uint32)), ("lc_coef", C.c_char_p)]


class _CircuitHintsC(C.Structure):
    _fields_ = [("op", C.POINTER(C.c_uint32)), ("lc_off", C.POINTER(C.c_uint32)), ("lc_var", C.POINTER(C.c_uint32)),
                ("lc_coef", C.c_char_p)]


class Circuit:
    """A compiled caller-defined circuit (bpp_circuit_create, or
    bpp_circuit_create_pub when desc.n_pub; no GPU): desc is a
    gadgets.CircuitDesc (or anything with its fields).  n_p, Q, m, n_pub,
    digest and proof_len are the compiled statement's; matrix() and eval()
    expose the compiled rows and the host witness.  large=True
    (bpp_circuit_create_ex, BPP_CIRCUIT_LARGE) accepts circuits beyond the
    one-workgroup LDS bounds (682 gates, Q = 1507); tiled=True
    (BPP_CIRCUIT_TILED, implies large) uses the large-circuit kernels even where
    the narrow ones fit.  Neither is part of the statement: digest, matrices and
    proof bytes are the same.  A desc with hints (desc.hints, a
    gadgets.CircuitHints: one hint per auxiliary value) is created through
    bpp_circuit_create_hinted, and CircuitProver.prove_batch then derives aux
    on the GPU; hints=False forces the plain entry point.  Hints are no part
    of the statement either.  When a hint names x or a wire (a late hint,
    gadgets.CircuitBuilder.derived) the entry point is
    bpp_circuit_create_wire_hinted: the witness kernel evaluates such a hint
    when it reaches the gate it feeds."""

    LARGE, TILED = 1, 2  # BPP_CIRCUIT_LARGE, BPP_CIRCUIT_TILED

    def __init__(self, desc, large: bool = False, tiled: bool = False, flags: "int | None" = None,
                 hints: bool = True, wire_hints: "bool | None" = None):
        """flags: the raw flag word in place of large / tiled (tests).
        wire_hints: bpp_circuit_create_wire_hinted (True) or
        bpp_circuit_create_hinted (False); None: the former when desc.hints
        says that a hint names x or a wire (CircuitHints.wire, which
        CircuitBuilder.build() sets), else the latter, which refuses such ids."""
        self.lib = _lib.load()
        self.desc = desc
        if flags is None:
            flags = (self.LARGE if large else 0) | (self.TILED if tiled else 0)
        self.flags = flags
        u32a = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)
        self._keep = (u32a(desc.side_aux), u32a(desc.lc_off), u32a(desc.lc_var), b"".join(desc.lc_coef))
        d = _CircuitDescC(desc.m_in, desc.n_gates, desc.n_aux, desc.n_asserts, self._keep[0], self._keep[1],
                          self._keep[2], self._keep[3])
        h = C.c_void_p()
        hd = getattr(desc, "hints", None) if hints else None
        if hd is not None:
            # (the C struct carries no count: one hint per auxiliary value is checked here)
            if len(hd.op) != desc.n_aux or len(hd.lc_off) != desc.n_aux + 1:
                raise ValueError("hints: one hint per auxiliary value (op [n_aux], lc_off [n_aux + 1])")
            if len(hd.lc_var) != len(hd.lc_coef) or (hd.lc_off and hd.lc_off[-1] > len(hd.lc_var)):
                raise ValueError("hints: lc_var / lc_coef shorter than lc_off says")
            self._keep_hints = (u32a(hd.op), u32a(hd.lc_off), u32a(hd.lc_var), b"".join(hd.lc_coef))
            hc = _CircuitHintsC(*self._keep_hints)
            # (hints that name x or a wire, as CircuitHints.wire says: the entry point that takes them)
            wire = bool(getattr(hd, "wire", False)) if wire_hints is None else wire_hints
            create = "bpp_circuit_create_wire_hinted" if wire else "bpp_circuit_create_hinted"
            check(getattr(self.lib, create)(C.byref(d), getattr(desc, "n_pub", 0), flags, C.byref(hc), C.byref(h)),
                  create)
        elif flags:
            check(self.lib.bpp_circuit_create_ex(C.byref(d), getattr(desc, "n_pub", 0), flags, C.byref(h)),
                  "bpp_circuit_create_ex")
        elif getattr(desc, "n_pub", 0):
            check(self.lib.bpp_circuit_create_pub(C.byref(d), desc.n_pub, C.byref(h)), "bpp_circuit_create_pub")
        else:
            check(self.lib.bpp_circuit_create(C.byref(d), C.byref(h)), "bpp_circuit_create")
        self.h = h
        self.n_pub = int(self.lib.bpp_circuit_n_pub(h))
        self.has_hints = bool(self.lib.bpp_circuit_has_hints(h))
        n_p, Q, m = C.c_uint32(), C.c_uint32(), C.c_uint32()
        dg = C.create_string_buffer(32)
        check(self.lib.bpp_circuit_info(h, C.byref(n_p), C.byref(Q), C.byref(m), dg), "bpp_circuit_info")
        self.n_p, self.Q, self.m, self.digest = n_p.value, Q.value, m.value, dg.raw
        self.m_in, self.n_aux = desc.m_in, desc.n_aux
        self.proof_len = int(self.lib.bpp_circuit_proof_len(h))

    def close(self):
        if self.h:
            self.lib.bpp_circuit_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def matrix(self, which: int):
        """Triplets (q, col, val bytes) of W_L, W_R, W_O, W_V (which = 0..3) or
        of c (which = 4: (q, 0, c[q])), or of W_U (which = 5: (q, i, val))."""
        n = C.c_size_t(0)
        rc = self.lib.bpp_circuit_matrix(self.h, which, None, None, None, C.byref(n))
        if rc not in (0, 2):
            check(rc, "bpp_circuit_matrix")
        cnt = n.value
        q, col = (C.c_uint32 * max(cnt, 1))(), (C.c_uint32 * max(cnt, 1))()
        val = C.create_string_buffer(max(32 * cnt, 1))
        check(self.lib.bpp_circuit_matrix(self.h, which, q, col, val, C.byref(n)), "bpp_circuit_matrix")
        return [(q[i], col[i], val.raw[32 * i:32 * i + 32]) for i in range(cnt)]

    def hint_eval(self, v, pub=None):
        """The hints' host reference (bpp_circuit_hint_eval; no GPU): the n_aux
        auxiliary values, 32-byte scalars, from v (m_in scalars) and pub (the
        n_pub public inputs)."""
        vb = _join(v, 32, "v")
        ub = _join(pub, 32, "pub") if pub is not None else b""
        if len(vb) != 32 * self.m_in or len(ub) != 32 * self.n_pub:
            raise ValueError("hint_eval: expected m_in scalars in v and n_pub in pub")
        out = C.create_string_buffer(max(32 * self.n_aux, 1))
        check(self.lib.bpp_circuit_hint_eval(self.h, _buf(vb), _buf(ub), out), "bpp_circuit_hint_eval")
        return [out.raw[32 * i:32 * i + 32] for i in range(self.n_aux)]

    def hint_eval_x(self, v, x: bytes, pub=None):
        """The hints' host reference with x (bpp_circuit_hint_eval_x; no GPU):
        all n_aux values, early hints as hint_eval gives them, late hints in
        gate order from the wires so far.  eval(v, that, x) is the witness."""
        vb = _join(v, 32, "v")
        ub = _join(pub, 32, "pub") if pub is not None else b""
        if len(vb) != 32 * self.m_in or len(ub) != 32 * self.n_pub or len(x) != 32:
            raise ValueError("hint_eval_x: expected m_in scalars in v, n_pub in pub and one in x")
        out = C.create_string_buffer(max(32 * self.n_aux, 1))
        check(self.lib.bpp_circuit_hint_eval_x(self.h, _buf(vb), _buf(ub), _buf(x), out), "bpp_circuit_hint_eval_x")
        return [out.raw[32 * i:32 * i + 32] for i in range(self.n_aux)]

    def eval(self, v, aux, x: bytes, pub=None):
        """The host witness: (a_L, a_R, a_O) as lists of n_p 32-byte scalars,
        and 1 + the first assert that does not hold (0: all hold).  pub: the
        n_pub public inputs (bpp_circuit_eval_pub)."""
        vb, ab = _join(v, 32, "v"), _join(aux, 32, "aux")
        outs = [C.create_string_buffer(32 * self.n_p) for _ in range(3)]
        bad = C.c_uint32()
        if pub is not None:
            ub = _join(pub, 32, "pub")
            check(self.lib.bpp_circuit_eval_pub(self.h, _buf(vb), _buf(ab), _buf(ub) if ub else None, _buf(x), *outs,
                                                C.byref(bad)), "bpp_circuit_eval_pub")
        else:
            check(self.lib.bpp_circuit_eval(self.h, _buf(vb), _buf(ab), _buf(x), *outs, C.byref(bad)),
                  "bpp_circuit_eval")
        return tuple([o.raw[32 * i:32 * i + 32] for i in range(self.n_p)] for o in outs) + (bad.value,)


class CircuitProver:
    """Proofs of a caller-defined circuit (bpp_circuit_*), mirroring DeckProver:
    circuit is a Circuit, or a description it is compiled from."""

    def __init__(self, gens: Gens, circuit, label: bytes = b"bp-perm", ctx: "Context | None" = None):
        self.gens = gens
        self.ctx = ctx or gens.ctx
        self.circuit = circuit if isinstance(circuit, Circuit) else Circuit(circuit)
        self.label = label
        self.proof_len = self.circuit.proof_len
        self.m = self.circuit.m

    def _pub_bytes(self, pub, count: int) -> bytes:
        """pub[p] = the n_pub public inputs of proof p (or each proof's joined)
        -> the joined bytes of the _pub entry points."""
        ub = b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, "pub") for x in pub)
        if len(ub) != 32 * self.circuit.n_pub * count:
            raise ValueError("pub: expected n_pub scalars of 32 bytes per proof")
        return ub

    def _pub(self, pub, count: int):
        ub = self._pub_bytes(pub, count)
        return _buf(ub) if ub else None

    def prove_batch(self, v, aux=None, seeds32: bytes | None = None, gammas=None, raw: bool = False,
                    out: "tuple | None" = None, pub=None):
        """v[p] = the m_in committed inputs of proof p, aux[p] = its n_aux
        auxiliary values, gammas[p] = the m_in blindings of V_0..V_{m_in-1}
        (None: drawn) -- 32-byte scalars (or each proof's joined); aux = None on
        a circuit with hints: derived on the GPU from v and pub; seeds32 = 32
        bytes per proof (None: the OS CSPRNG).  out = (proofs, V) ctypes buffers
        to write into instead of fresh ones.  pub[p] = the n_pub public inputs
        of proof p (bpp_circuit_prove_batch_pub; None: the entry point without
        them).  Returns what DeckProver.prove_batch returns; the batch's
        secrets are wiped."""
        c = self.circuit
        count = len(v)
        row = lambda rows, what: b"".join(x if isinstance(x, (bytes, bytearray)) else _join(x, 32, what) for x in rows)
        vb = row(v, "v")
        if len(vb) != 32 * c.m_in * count:
            raise ValueError("v: expected m_in scalars of 32 bytes per proof")
        ab = row(aux, "aux") if aux is not None else b""
        # (no aux on a circuit with hints: NULL, and the library derives the values on the GPU)
        if len(ab) != 32 * c.n_aux * count and not (aux is None and c.has_hints):
            raise ValueError("aux: expected n_aux scalars of 32 bytes per proof")
        gb = None
        if gammas is not None:
            gb = row(gammas, "gammas")
            if len(gb) != 32 * c.m_in * count:
                raise ValueError("gammas: expected m_in scalars of 32 bytes per proof")
        if seeds32 is not None and len(seeds32) != 32 * count:
            raise ValueError("seeds32 must hold 32 bytes per proof")
        if out is None:
            pf = C.create_string_buffer(max(self.proof_len * count, 1))
            V = C.create_string_buffer(max(32 * self.m * count, 1))
        else:
            pf, V = out
        tail = (_buf(gb) if gb is not None else None, _buf(seeds32) if seeds32 is not None else None,
                _buf(self.label), len(self.label), pf, V)
        if pub is not None:
            check(self.ctx.lib.bpp_circuit_prove_batch_pub(self.ctx.h, self.gens.h, c.h, count, _buf(vb), _buf(ab),
                                                           self._pub(pub, count), *tail),
                  "bpp_circuit_prove_batch_pub", self.ctx.h)
        else:
            check(self.ctx.lib.bpp_circuit_prove_batch(self.ctx.h, self.gens.h, c.h, count, _buf(vb), _buf(ab), *tail),
                  "bpp_circuit_prove_batch", self.ctx.h)
        praw, vraw = pf.raw[:self.proof_len * count], V.raw[:32 * self.m * count]
        if raw:
            return praw, vraw
        return ([praw[i * self.proof_len:(i + 1) * self.proof_len] for i in range(count)],
                [vraw[i * 32 * self.m:(i + 1) * 32 * self.m] for i in range(count)])

    def verify(self, proof: bytes, V, pub=None) -> bool:
        """pub: this proof's n_pub public inputs (bpp_circuit_verify_pub)."""
        vb = _join(V, 32, "V")
        args = (self.ctx.h, self.gens.h, self.circuit.h, _buf(self.label), len(self.label), _buf(proof), len(proof),
                _buf(vb))
        if pub is not None:
            rc = self.ctx.lib.bpp_circuit_verify_pub(*args, self._pub([pub], 1))
        else:
            rc = self.ctx.lib.bpp_circuit_verify(*args)
        if rc == 6:
            return False
        check(rc, "bpp_circuit_verify", self.ctx.h)
        return True

    _batch_buffers = PermProver._batch_buffers

    def verify_batch(self, proofs, Vs, pub=None) -> bool:
        pb, vb, count = self._batch_buffers(proofs, Vs)
        args = (self.ctx.h, self.gens.h, self.circuit.h, count, _buf(self.label), len(self.label), _buf(pb), _buf(vb))
        if pub is not None:
            rc = self.ctx.lib.bpp_circuit_verify_batch_pub(*args, self._pub(pub, count))
        else:
            rc = self.ctx.lib.bpp_circuit_verify_batch(*args)
        if rc == 6:
            return False
        check(rc, "bpp_circuit_verify_batch", self.ctx.h)
        return True

    def verify_batch_each(self, proofs, Vs, pub=None) -> "list[bool]":
        pb, vb, count = self._batch_buffers(proofs, Vs)
        ok = C.create_string_buffer(max(count, 1))
        args = (self.ctx.h, self.gens.h, self.circuit.h, count, _buf(self.label), len(self.label), _buf(pb), _buf(vb))
        if pub is not None:
            rc = self.ctx.lib.bpp_circuit_verify_batch_each_pub(*args, self._pub(pub, count), ok)
        else:
            rc = self.ctx.lib.bpp_circuit_verify_batch_each(self.ctx.h, self.gens.h, self.circuit.h, count,
                                                            _buf(self.label), len(self.label), _buf(pb), _buf(vb), ok)
        if rc != 6:
            check(rc, "bpp_circuit_verify_batch_each", self.ctx.h)
        return [b != 0 for b in ok.raw[:count]]


VERIFY_GROUPS_MAX = 16  # BPP_VERIFY_GROUPS_MAX (include/bpperm.h)


class _VerifyGroupC(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("k", C.c_uint32), ("deck", C.c_char_p), ("circuit", C.c_void_p),
                ("label", C.c_char_p), ("label_len", C.c_size_t), ("count", C.c_size_t), ("proofs", C.c_char_p),
                ("V", C.c_char_p), ("pub", C.c_char_p)]


def verify_groups(gens: Gens, groups, each: bool = False, ctx: "Context | None" = None):
    """Proofs of different statements verified in one call with one MSM
    (bpp_verify_groups, bpp_verify_groups_each).  groups: a sequence of
    (prover, proofs, Vs) or (prover, proofs, Vs, pub), prover a PermProver,
    DeckProver or CircuitProver -- it supplies the statement and the label --
    and proofs / Vs in the two forms its verify_batch takes; pub as
    CircuitProver.verify_batch takes it.  Returns True if every proof
    verifies; with each=True one list of per-proof verdicts per group, what
    prover.verify(proof, V[, pub]) returns for each."""
    ctx = ctx or gens.ctx
    arr = (_VerifyGroupC * max(len(groups), 1))()
    keep = []  # the buffers the structs point into, alive across the call
    counts = []
    for i, grp in enumerate(groups):
        prover, proofs, Vs = grp[0], grp[1], grp[2]
        pub = grp[3] if len(grp) > 3 else None
        pb, vb, count = prover._batch_buffers(proofs, Vs)
        g = arr[i]
        g.label, g.label_len, g.count = prover.label or None, len(prover.label), count
        g.proofs, g.V = pb or None, vb or None
        if isinstance(prover, CircuitProver):
            g.kind, g.circuit = 2, prover.circuit.h
            if pub is not None:
                ub = prover._pub_bytes(pub, count)
                g.pub = ub or None
                keep.append(ub)
        elif isinstance(prover, DeckProver):
            g.kind, g.k, g.deck = 1, prover.k, prover.deck
        elif isinstance(prover, PermProver):
            g.kind, g.k = 0, prover.k
        else:
            raise TypeError("verify_groups: prover must be a PermProver, DeckProver or CircuitProver")
        keep += [prover, pb, vb]
        counts.append(count)
    if not each:
        rc = ctx.lib.bpp_verify_groups(ctx.h, gens.h, arr, len(groups))
        if rc == 6:
            return False
        check(rc, "bpp_verify_groups", ctx.h)
        return True
    total = sum(counts)
    ok = C.create_string_buffer(max(total, 1))
    rc = ctx.lib.bpp_verify_groups_each(ctx.h, gens.h, arr, len(groups), ok)
    if rc != 6:
        check(rc, "bpp_verify_groups_each", ctx.h)
    flags, out, o = ok.raw, [], 0
    for n in counts:
        out.append([b != 0 for b in flags[o:o + n]])
        o += n
    return out


class VerifyJob:
    """Parsed proofs with their transcripts replayed: on the host
    (bpp_perm_verify_begin, ctx=None; no GPU) or on the GPU of `ctx`
    (bpp_perm_verify_begin_dev: the job's records stay in that context's
    workspaces, valid until its next device job).  `r` holds each proof's
    weight challenge; proof p's batch weight mixes it with the batch's
    verifier seed (bpp_perm_verify_scalars)."""

    def __init__(self, k: int, proofs: Sequence[bytes], Vs: Sequence[bytes], label: bytes = b"bp-perm",
                 ctx: "Context | None" = None, wait: bool = True):
        """wait=False (a device job): bpp_perm_verify_begin_dev_async --
        returns before the replay ends, `r` is None and a rejected proof
        surfaces as False from slice_scalars / verify_partial."""
        self.lib = _lib.load()
        self.k = k
        self.count = len(proofs)
        self.device = ctx is not None
        self.ctx = ctx
        h = C.c_void_p()
        nr = self.count
        r = C.create_string_buffer(32 * nr + 1)
        pb, vb = _buf(b"".join(proofs)), _buf(b"".join(Vs))
        if ctx is None:
            rc = self.lib.bpp_perm_verify_begin(k, self.count, _buf(label), len(label), pb, vb, r, C.byref(h))
            name = "bpp_perm_verify_begin"
        elif not wait:
            self._keep = (pb, vb)  # (pinned inputs are read after the return; these are staged, but keep them)
            rc = self.lib.bpp_perm_verify_begin_dev_async(ctx.h, k, self.count, _buf(label), len(label), pb, vb,
                                                          C.byref(h))
            name = "bpp_perm_verify_begin_dev_async"
            nr = 0
        else:
            rc = self.lib.bpp_perm_verify_begin_dev(ctx.h, k, self.count, _buf(label), len(label), pb, vb, r,
                                                    C.byref(h))
            name = "bpp_perm_verify_begin_dev"
        if rc == 6:
            self.h = None
            self.r = None
            return
        check(rc, name, ctx.h if ctx is not None else None)
        self.h = h
        self.r = r.raw[:32 * nr] if nr else (None if not wait else b"")

    def slice_bytes(self) -> int:
        return int(self.lib.bpp_perm_verify_slice_bytes(self.h))

    def slice_scalars(self, seed: bytes, d_out: int, first: int = 0) -> bool:
        """The replayed slice's MSM scalars into device memory d_out
        (slice_bytes() bytes; bpp_perm_verify_slice_scalars_at), weighted from
        the batch's verifier seed; first = the batch index of the job's first
        proof.  False
        if an asynchronous begin's replay rejected a proof."""
        rc = self.lib.bpp_perm_verify_slice_scalars_at(self.ctx.h, self.h, _seed(seed), first, d_out)
        if rc == 6:
            return False
        check(rc, "bpp_perm_verify_slice_scalars_at", self.ctx.h)
        return True

    def point_bytes(self) -> int:
        """Bytes of the job's decompressed proof points (128 per point)."""
        return int(self.lib.bpp_perm_verify_slice_point_bytes(self.h))

    def slice_points(self, d_out: int) -> bool:
        """The job's decompressed proof points into device memory d_out
        (point_bytes() bytes; bpp_perm_verify_slice_points); False if a
        point did not decode."""
        rc = self.lib.bpp_perm_verify_slice_points(self.ctx.h, self.h, d_out)
        if rc == 6:
            return False
        check(rc, "bpp_perm_verify_slice_points", self.ctx.h)
        return True

    @property
    def ok(self) -> bool:
        """False if a proof was malformed (the batch cannot verify)."""
        return self.h is not None

    def terms(self) -> int:
        n = C.c_size_t()
        check(self.lib.bpp_perm_verify_terms(self.h, C.byref(n)), "bpp_perm_verify_terms")
        return n.value

    def windows(self) -> tuple[int, int]:
        return msm_windows(self.terms())

    def scalars(self, seed: bytes, first: int):
        """(scalars, proof-point encodings) of the job's MSM (host), its
        proofs being batch proofs [first, first + count) weighted from the
        batch's verifier seed: the first 2 n_p + 2 scalars go to G[0..n_p),
        H[0..n_p), B, B_blinding."""
        T = self.terms()
        n_p = 1
        while n_p < 2 * self.k:
            n_p <<= 1
        npts = T - (2 * n_p + 2)
        sc = C.create_string_buffer(32 * T)
        pts = C.create_string_buffer(32 * max(npts, 1))
        check(self.lib.bpp_perm_verify_scalars(self.h, _seed(seed), first, sc, pts), "bpp_perm_verify_scalars")
        sraw, praw = sc.raw, pts.raw
        return ([sraw[32 * i: 32 * i + 32] for i in range(T)], [praw[32 * i: 32 * i + 32] for i in range(npts)])

    def close(self):
        if self.h is not None:
            self.lib.bpp_perm_verify_end(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def scalar_invert(x: bytes) -> bytes:
    """Scalar::invert of a canonical 32-byte scalar (bpp_scalar_invert)."""
    out = C.create_string_buffer(32)
    check(_lib.load().bpp_scalar_invert(_buf(bytes(x)), out), "bpp_scalar_invert")
    return out.raw


def scalar_powers(x: bytes, n: int) -> bytes:
    """x^0 .. x^(n-1) as n x 32 bytes (bpp_scalar_powers; util.rs exp_iter)."""
    out = C.create_string_buffer(32 * max(n, 1))
    check(_lib.load().bpp_scalar_powers(_buf(bytes(x)), n, out), "bpp_scalar_powers")
    return out.raw[:32 * n]


def verify_seed() -> bytes:
    """32 bytes of verifier randomness for one batch (bpp_verify_seed: the OS
    CSPRNG).  Every job / rank of the batch must use the same bytes."""
    out = C.create_string_buffer(32)
    check(_lib.load().bpp_verify_seed(out), "bpp_verify_seed")
    return out.raw


def _seed(seed: bytes):
    if not isinstance(seed, (bytes, bytearray)) or len(seed) != 32:
        raise ValueError("a batch-verification seed is 32 bytes")
    return _buf(bytes(seed))


def partials_is_identity(partials: Sequence[bytes]) -> bool:
    """True iff the raw partial points add up to the identity."""
    raw = _join(partials, 128, "partial")
    rc = _lib.load().bpp_partials_is_identity(_buf(raw), len(partials))
    if rc == 6:
        return False
    check(rc, "bpp_partials_is_identity")
    return True

