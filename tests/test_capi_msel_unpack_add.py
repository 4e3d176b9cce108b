"""Host checks of mgr_msel_unpack_add (the halo's return path): the symbol is
exported and bound, every argument refusal comes before any launch, and an
empty call reads nothing."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


def _args():
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    masks = (ctypes.c_int * 2)(1, 2)
    srcs = (ctypes.c_void_p * 2)(p.value, None)
    return buf, p, masks, srcs


def test_symbol_exported_and_bound(lib):
    from mpi_grid_redistribute_amd import _lib
    assert hasattr(lib, "mgr_msel_unpack_add")
    assert "mgr_msel_unpack_add" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mgr_msel_unpack_add"][1]) == 11
    assert (_lib.MGR_ELEM_F32, _lib.MGR_ELEM_F64, _lib.MGR_ELEM_I32, _lib.MGR_ELEM_I64) == (
        0, 1, 2, 3)


def test_refusals(lib):
    buf, p, masks, srcs = _args()
    f = lib.mgr_msel_unpack_add
    assert f(p, 0, 1, 5, p, 0, masks, 4096, p, srcs, None) == -1          # no sets
    assert b"nsets" in lib.mgr_last_error()
    assert f(p, 0, 1, 5, p, 33, masks, 4096, p, srcs, None) == -1         # > 32 sets
    assert f(p, 0, 0, 5, p, 2, masks, 4096, p, srcs, None) == -1          # ncomp < 1
    assert b"ncomp" in lib.mgr_last_error()
    for elem in (-1, 4, 99):
        assert f(p, elem, 1, 5, p, 2, masks, 4096, p, srcs, None) == -1   # unknown elem
        assert b"elem" in lib.mgr_last_error()
    assert f(p, 0, 1, -1, p, 2, masks, 4096, p, srcs, None) == -1         # n < 0
    assert f(p, 0, 1, 5, p, 2, masks, 100, p, srcs, None) == -1           # tile not 64 k
    bad = (ctypes.c_int * 2)(1, 1 << 16)
    assert f(p, 0, 1, 5, p, 2, bad, 4096, p, srcs, None) == -1            # mask beyond 16 bits
    for a in range(4):   # a null acc / flags / workspace / srcs with n > 0
        args = [p, 0, 1, 5, p, 2, masks, 4096, p, srcs, None]
        args[(0, 4, 8, 9)[a]] = None
        assert f(*args) == -1, a
        assert b"null" in lib.mgr_last_error()


def test_empty_reads_nothing(lib):
    _, _, masks, _ = _args()
    for elem in range(4):
        assert lib.mgr_msel_unpack_add(None, elem, 3, 0, None, 2, masks, 4096, None, None,
                                       None) == 0
