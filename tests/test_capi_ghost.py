"""Host checks of the ghost-cell entry points (mgr_shift_regions,
mgr_ghost_cells): the symbols are exported and bound, every argument refusal
comes before any launch, an empty call reads nothing; and the values of
``ghost_grid``, the one definition of the extended grid."""
import ctypes

import numpy as np
import pytest

F32, F64 = 1, 2
EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


def _p():
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


def _int(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_exported_and_bound(lib):
    from mpi_grid_redistribute_amd import _lib
    for name, nargs in (("mgr_shift_regions", 9), ("mgr_ghost_cells", 13)):
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs


def test_shift_regions_refusals(lib):
    buf, p = _p()
    f = lib.mgr_shift_regions
    ends, sh = _i64(2, 5), _f64(*([1.0] * 6))
    for dt in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, 99):     # anything but f32 / f64
        assert f(p, dt, 5, 3, 3, 2, ends, sh, None) == EUNSUPPORTED, dt
        assert b"float32" in lib.mgr_last_error()
    for dim in (0, -1, 9):
        assert f(p, F32, 5, 9, dim, 2, ends, sh, None) == EINVAL
        assert b"dim" in lib.mgr_last_error()
    assert f(p, F32, -1, 3, 3, 2, ends, sh, None) == EINVAL             # n < 0
    assert f(p, F64, 5, 2, 3, 2, ends, sh, None) == EINVAL              # row_stride < dim
    assert b"row_stride" in lib.mgr_last_error()
    for k in (0, -3, 65):
        assert f(p, F32, 5, 3, 3, k, ends, sh, None) == EINVAL
        assert b"nregions" in lib.mgr_last_error()
    for a in (0, 6, 7):   # a null pos / region_end / shift with n > 0
        args = [p, F32, 5, 3, 3, 2, ends, sh, None]
        args[a] = None
        assert f(*args) == EINVAL, a
        assert b"null" in lib.mgr_last_error()
    assert f(p, F32, 5, 3, 3, 2, _i64(3, 2), sh, None) == EINVAL        # decreasing
    assert b"decreases" in lib.mgr_last_error()
    assert f(p, F32, 5, 3, 3, 2, _i64(-1, 5), sh, None) == EINVAL       # starts below row 0
    assert f(p, F32, 5, 3, 3, 2, _i64(2, 4), sh, None) == EINVAL        # ends before n
    assert b"ends at" in lib.mgr_last_error()
    assert f(p, F32, 5, 3, 3, 2, _i64(2, 6), sh, None) == EINVAL        # ends beyond n


def test_ghost_cells_refusals(lib):
    buf, p = _p()
    f = lib.mgr_ghost_cells
    org, wid, fine, gh = _f64(0, 0, 0), _f64(.1, .1, .1), _int(4, 4, 4), _int(1, 1, 1)

    def call(**kw):
        a = dict(pos=p, dt=F32, n=5, no=3, stride=3, dim=3, org=org, wid=wid, fine=fine, gh=gh,
                 ids=p, out=None)
        a.update(kw)
        return f(a["pos"], a["dt"], a["n"], a["no"], a["stride"], a["dim"], a["org"], a["wid"],
                 a["fine"], a["gh"], a["ids"], a["out"], None)

    for dt in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, 99):
        assert call(dt=dt) == EUNSUPPORTED, dt
    for dim in (0, -1, 9):
        assert call(dim=dim, stride=9) == EINVAL
        assert b"dim" in lib.mgr_last_error()
    assert call(n=-1, no=0) == EINVAL
    for no in (-1, 6):
        assert call(no=no) == EINVAL
        assert b"n_owned" in lib.mgr_last_error()
    assert call(stride=2) == EINVAL
    for k in ("pos", "org", "wid", "fine", "gh", "ids"):
        assert call(**{k: None}) == EINVAL, k
        assert b"null" in lib.mgr_last_error()
    for w in (0.0, -0.5, float("inf"), float("nan")):
        assert call(wid=_f64(.1, w, .1)) == EINVAL, w
        assert b"width" in lib.mgr_last_error()
    assert call(fine=_int(4, 0, 4)) == EINVAL
    assert b"fine" in lib.mgr_last_error()
    assert call(gh=_int(1, 1, -1)) == EINVAL
    assert b"ghost" in lib.mgr_last_error()
    assert call(fine=_int(8, 8, 8), gh=_int(2, 2, 2)) == EINVAL         # 12^3 = 1728 cells
    assert b"1024" in lib.mgr_last_error()
    assert call(fine=_int(2 ** 30, 2 ** 30, 2 ** 30)) == EINVAL         # no overflow on the way
    assert call(dim=1, fine=_int(1024), gh=_int(1)) == EINVAL           # 1026 cells


def test_empty_reads_nothing(lib):
    for dt in (F32, F64):
        assert lib.mgr_shift_regions(None, dt, 0, 3, 3, 1, None, None, None) == 0
        assert lib.mgr_ghost_cells(None, dt, 0, 0, 3, 3, None, None, None, None, None, None,
                                   None) == 0


def _grid(cell, fine, ol, low=0.0):
    from mpi_grid_redistribute_amd import ghost_grid
    cl = np.asarray(cell, dtype=np.float64)
    lim = np.stack([np.full(len(cl), low), low + cl], axis=1)
    return ghost_grid(cl, lim, fine, ol)


def test_ghost_grid_values():
    # no halo: the fine grid itself
    ghost, ext, origin, width = _grid([1.0, 0.5, 0.25], [8, 4, 2], [0, 0, 0], low=0.5)
    assert ghost.tolist() == [0, 0, 0] and ext.tolist() == [8, 4, 2]
    assert origin.tolist() == [0.5, 0.5, 0.5] and origin.dtype == np.float64
    assert width.tolist() == [0.125, 0.125, 0.125] and width.dtype == np.float64
    # an exact multiple of the width: exactly that many layers, no spare one
    ghost, ext, _, width = _grid([1.0, 1.0, 1.0], [8, 8, 4], [0.25, 0.125, 0.5])
    assert ghost.tolist() == [2, 1, 2] and ext.tolist() == [12, 10, 8]
    # between multiples: rounded up; a zero length beside non-zero ones
    ghost, ext, _, _ = _grid([1.0, 1.0, 1.0], [8, 8, 8], [0.05, 0.0, 0.126])
    assert ghost.tolist() == [1, 0, 2] and ext.tolist() == [10, 8, 12]
    # ol > cell: more ghost layers than fine cells
    ghost, ext, _, _ = _grid([0.5, 0.5], [4, 2], [0.75, 0.6])
    assert ghost.tolist() == [6, 3] and ext.tolist() == [16, 8]
    # width is numpy's cell_length / fine, bit for bit
    _, _, _, width = _grid([1.0 / 3.0], [7], [0.01])
    assert width[0] == np.float64(1.0 / 3.0) / 7


def test_ghost_grid_refusals():
    with pytest.raises(ValueError, match="1024"):
        _grid([1.0, 1.0, 1.0], [8, 8, 8], [0.25, 0.25, 0.25])           # 12^3
    with pytest.raises(ValueError, match="1024"):
        _grid([1.0], [4], [1000.0])
    with pytest.raises(ValueError):
        _grid([1.0, 1.0], [4, 0], [0.1, 0.1])
    with pytest.raises(ValueError):
        _grid([1.0, 1.0], [4, 4], [0.1, -0.1])
    with pytest.raises(ValueError):
        _grid([1.0, 1.0], [4, 4], [0.1])
    assert _grid([1.0, 1.0, 1.0], [8, 8, 8], [0.125] * 3)[1].tolist() == [10, 10, 10]
