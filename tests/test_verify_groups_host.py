"""bpp_verify_groups / bpp_verify_groups_each without a GPU: the exports, their
ctypes signatures, and the refusals that need no context -- a null context, more
groups than BPP_VERIFY_GROUPS_MAX (checked first: it bounds what is read of the
caller's array), an unknown statement kind."""
import ctypes as C

import pytest

NAMES = ("bpp_verify_groups", "bpp_verify_groups_each")
ARG, LEN = 1, 2


@pytest.fixture(scope="module")
def lib():
    from bpperm import _lib
    return _lib.load()


def _groups(n, kind=0):
    import bpperm
    arr = (bpperm._VerifyGroupC * max(n, 1))()
    for g in arr:
        g.kind, g.k, g.count = kind, 4, 0
    return arr


def test_exported_with_signatures(lib):
    from bpperm import _lib
    import bpperm
    for name in NAMES:
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["bpp_verify_groups_each"][1]) == len(_lib.SIGNATURES["bpp_verify_groups"][1]) + 1
    assert callable(bpperm.verify_groups) and bpperm.VERIFY_GROUPS_MAX == 16
    # the struct the header declares: two u32, three pointers, two size_t, three pointers
    assert C.sizeof(bpperm._VerifyGroupC) == 8 + 8 * C.sizeof(C.c_void_p)


def test_null_context(lib):
    ok = C.create_string_buffer(4)
    assert lib.bpp_verify_groups(None, None, None, 0) == ARG
    assert lib.bpp_verify_groups_each(None, None, None, 0, ok) == ARG
    assert lib.bpp_verify_groups(None, None, _groups(3), 3) == ARG
    assert lib.bpp_verify_groups_each(None, None, _groups(3), 3, ok) == ARG


def test_too_many_groups(lib):
    ok = C.create_string_buffer(4)
    assert lib.bpp_verify_groups(None, None, _groups(17), 17) == LEN
    assert lib.bpp_verify_groups_each(None, None, _groups(17), 17, ok) == LEN
    assert lib.bpp_verify_groups(None, None, _groups(16), 16) == ARG  # (the null context, not the length)


def test_unknown_kind(lib):
    ok = C.create_string_buffer(4)
    assert lib.bpp_verify_groups(None, None, _groups(1, kind=3), 1) == ARG
    assert lib.bpp_verify_groups_each(None, None, _groups(2, kind=0xFFFFFFFF), 2, ok) == ARG
