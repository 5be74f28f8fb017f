"""bpp_perm_verify_batch_each without a GPU: the argument checks that run
before any device work, and the symbol's presence in the library, the Python
binding and INTEGRATION.md."""
import ctypes
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NAME = "bpp_perm_verify_batch_each"
ARG = 1


def _cdll():
    from bpperm import _lib
    return ctypes.CDLL(str(_lib.LIB_PATH))


def _call(lib, ctx, gens, k, count, proofs, V, ok):
    return getattr(lib, NAME)(ctx, gens, ctypes.c_uint32(k), ctypes.c_size_t(count), None, ctypes.c_size_t(0), proofs,
                              V, ok)


def test_argument_checks_without_device():
    lib = _cdll()
    buf = ctypes.create_string_buffer(4096)
    ok = ctypes.create_string_buffer(b"\x01" * 4, 4)
    fake = ctypes.c_void_p(8)  # never dereferenced: the checks below come first
    # ok_out NULL with count > 0
    assert _call(lib, fake, fake, 52, 1, buf, buf, None) == ARG
    # a null context; ok_out was reachable, so it holds no pass
    assert _call(lib, None, None, 52, 4, buf, buf, ok) == ARG
    assert ok.raw == bytes(4)
    for k in (1, (1 << 20) + 1):
        ok = ctypes.create_string_buffer(b"\x01" * 4, 4)
        assert _call(lib, fake, fake, k, 4, buf, buf, ok) == ARG
        assert ok.raw == bytes(4)
    # null proofs / V with count > 0
    assert _call(lib, fake, fake, 52, 1, None, buf, ok) == ARG
    assert _call(lib, fake, fake, 52, 1, buf, None, ok) == ARG


def test_symbol_is_exported_bound_and_documented():
    from bpperm import _lib
    assert hasattr(_cdll(), NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 9
    sec = (ROOT / "INTEGRATION.md").read_text().split("## 5.")[1]
    assert f"`{NAME}`" in sec
    assert NAME in (ROOT / "include" / "bpperm.h").read_text()
