"""Host checks of mgr_unpack_ranked_fields, the inverse of the ranked
fine-cell sort: the symbol is exported with the header's signature, the
profiler knows its id, and every argument error is refused on the host, before
any launch, with a message."""
import ctypes

import pytest

from tests.test_capi_unpack import MGR_EINVAL, _p, header_signature

NAME = "mgr_unpack_ranked_fields"


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


def test_exported_with_the_headers_signature(lib):
    from mpi_grid_redistribute_amd import _lib
    assert hasattr(lib, NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert (res, args) == header_signature(NAME)
    fn = getattr(lib, NAME)
    assert fn.restype is res and list(fn.argtypes) == args
    assert len(args) == 12


def test_profiler_knows_unpack_ranked(lib):
    from mpi_grid_redistribute_amd import _lib
    assert _lib.PROFILE_KERNELS[-1] == "unpack_ranked"            # appended: earlier ids stable
    assert _lib.PROFILE_KERNELS.index("unpack") == len(_lib.PROFILE_KERNELS) - 2
    for i, name in enumerate(_lib.PROFILE_KERNELS):
        assert lib.mgr_profile_kernel_id(name.encode()) == i, name


def test_sort_route_is_exported():
    import mpi_grid_redistribute_amd as m
    assert "SortRoute" in m.__all__ and m.SortRoute is m.redistributor.SortRoute


def test_unpack_ranked_einval(lib):
    keep, p = _p()
    err = lib.mgr_last_error
    V = ctypes.c_void_p

    def call(nf=2, sorted_=(p.value, p.value), rbs=(8, 3), n=5, ids=p, ranks=p, ts=p, nbins=4,
             tile=2048, ws=p, outs=(p.value, p.value)):
        k = max(len(sorted_), 1)
        sd = (V * k)(*sorted_)
        ot = (V * k)(*outs)
        rb = (ctypes.c_int64 * k)(*rbs)
        return lib.mgr_unpack_ranked_fields(nf, sd, rb, n, ids, ranks, ts, nbins, tile, ws, ot,
                                            None)

    assert call(nf=0) == MGR_EINVAL and b"nfields" in err()
    many = (p.value,) * 17
    assert call(nf=17, sorted_=many, rbs=(8,) * 17, outs=many) == MGR_EINVAL and b"nfields" in err()
    for kw in ({"ids": None}, {"ranks": None}, {"ts": None}, {"ws": None},
               {"sorted_": (p.value, None)}, {"sorted_": (None, p.value)},
               {"outs": (None, p.value)}, {"outs": (p.value, None)}):
        assert call(**kw) == MGR_EINVAL, kw
        assert b"null" in err(), kw
    for rbs in ((8, 0), (-4, 8)):
        assert call(rbs=rbs) == MGR_EINVAL and b"row_bytes" in err()
    for tile in (0, 64, 512, 1024, 2047, 3072, 8192, 1 << 20):
        assert call(tile=tile) == MGR_EINVAL and b"tile_rows" in err(), tile
    for nbins in (0, -1, 1025, 2048):
        assert call(nbins=nbins) == MGR_EINVAL and b"nbins" in err(), nbins
    assert call(n=-1) == MGR_EINVAL and b"n < 0" in err()
    # argument errors are errors for an empty call too
    assert call(n=0, tile=512) == MGR_EINVAL and call(n=0, nf=0) == MGR_EINVAL
    # n == 0: nothing is read, no pointer is touched, no launch (there is no GPU here)
    for tile in (2048, 4096):
        assert call(n=0, ids=None, ranks=None, ts=None, ws=None, sorted_=(None, None),
                    outs=(None, None), tile=tile) == 0
    del keep
