"""Host checks of the return path's C ABI (mgr_unpack, mgr_unpack_fields):
the symbols are exported, their ctypes signatures are the header's, and every
argument error is refused on the host, before any launch, with a message."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgr.h")
MGR_EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


def header_signature(name):
    """(restype, [argtypes]) of ``name`` as include/mgr.h declares it."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in mgr.h"

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return ctypes.c_void_p
        base = decl.split()[0] if decl.split()[0] != "const" else decl.split()[1]
        return {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[base]

    return ctype(m.group(1)), [ctype(a) for a in m.group(2).split(",")]


@pytest.mark.parametrize("name", ["mgr_unpack", "mgr_unpack_fields"])
def test_exported_with_the_headers_signature(lib, name):
    from mpi_grid_redistribute_amd import _lib
    assert hasattr(lib, name)
    res, args = _lib.SIGNATURES[name]
    assert (res, args) == header_signature(name)
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args


def test_profiler_and_hook_know_the_unpack(lib):
    from mpi_grid_redistribute_amd import _lib
    assert "unpack" in _lib.PROFILE_KERNELS
    assert lib.mgr_profile_kernel_id(b"unpack") == _lib.PROFILE_KERNELS.index("unpack")
    assert _lib.HOOK_DEFAULTS["unpack_kernel"] == 0
    for v in (1, 2, 0):
        _lib.test_hook("unpack_kernel", v)
    with pytest.raises(_lib.MgrError):
        _lib.test_hook("unpack_kernel", 3)


def _p():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_unpack_einval(lib):
    keep, p = _p()
    err = lib.mgr_last_error

    def call(packed=p, rb=8, n=5, dest=p, nbins=4, drop=-1, tile=512, ws=p, out=p, red=-1,
             red_src=None):
        return lib.mgr_unpack(packed, rb, n, dest, nbins, drop, tile, ws, out, red, red_src, None)

    for kw in ({"dest": None}, {"ws": None}, {"out": None}, {"packed": None}):
        assert call(**kw) == MGR_EINVAL, kw
        assert b"null" in err()
    assert call(rb=0) == MGR_EINVAL and b"row_bytes" in err()
    for tile in (0, 100, 63, 1 << 20):
        assert call(tile=tile) == MGR_EINVAL and b"tile_rows" in err()
    assert call(red=2, red_src=None) == MGR_EINVAL and b"redirect" in err()
    assert call(red=2, drop=2, red_src=p) == MGR_EINVAL and b"drop bin" in err()
    assert call(red=4, red_src=p) == MGR_EINVAL and b"redirect_bin" in err()
    assert call(nbins=0) == MGR_EINVAL and b"nbins" in err()
    assert call(n=-1) == MGR_EINVAL
    # n == 0: nothing is read, no pointer is touched
    assert call(packed=None, n=0, dest=None, ws=None, out=None) == 0
    del keep


def test_unpack_fields_einval(lib):
    keep, p = _p()
    err = lib.mgr_last_error
    V = ctypes.c_void_p

    def call(nf=2, packed=(p.value, p.value), rbs=(8, 4), n=5, dest=p, nbins=4, drop=-1, tile=512,
             ws=p, outs=(p.value, p.value), red=-1, reds=None, t0=0, t1=-1):
        k = max(len(packed), 1)
        pk = (V * k)(*packed)
        ot = (V * k)(*outs)
        rb = (ctypes.c_int64 * k)(*rbs)
        rs = (V * k)(*reds) if reds is not None else None
        return lib.mgr_unpack_fields(nf, pk, rb, n, dest, nbins, drop, tile, ws, ot, red, rs, t0,
                                     t1, None)

    assert call(nf=0) == MGR_EINVAL and b"nfields" in err()
    many = (p.value,) * 17
    assert call(nf=17, packed=many, rbs=(8,) * 17, outs=many) == MGR_EINVAL and b"nfields" in err()
    assert call(packed=(p.value, None)) == MGR_EINVAL and b"null" in err()
    assert call(outs=(None, p.value)) == MGR_EINVAL and b"null" in err()
    assert call(dest=None) == MGR_EINVAL and b"null" in err()
    assert call(ws=None) == MGR_EINVAL and b"null" in err()
    assert call(rbs=(8, 0)) == MGR_EINVAL and b"row_bytes" in err()
    assert call(tile=96) == MGR_EINVAL and b"tile_rows" in err()
    assert call(red=1) == MGR_EINVAL and b"redirect" in err()
    assert call(red=1, reds=(p.value, None)) == MGR_EINVAL and b"redirect" in err()
    assert call(red=1, drop=1, reds=(p.value, p.value)) == MGR_EINVAL and b"drop bin" in err()
    # tile ranges: 5 rows of 512-row tiles are one tile
    for t0, t1 in ((-1, 1), (1, 0), (0, 2), (2, 2)):
        assert call(t0=t0, t1=t1) == MGR_EINVAL, (t0, t1)
        assert b"tiles" in err()
    assert call(t0=0, t1=0) == 0 and call(t0=1, t1=1) == 0       # empty ranges: no launch
    assert call(n=0, dest=None, ws=None, packed=(None, None), outs=(None, None)) == 0
    assert call(n=0, t0=0, t1=1) == MGR_EINVAL and b"tiles" in err()
    del keep
