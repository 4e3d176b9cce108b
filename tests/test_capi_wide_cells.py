"""Host checks of the entry points of the cell lists beyond 1024 cells
(mgr_ghost_cells_wide, mgr_id_digit, mgr_cell_offsets): exported and bound,
every argument refusal comes before any launch, the accepted boundaries pass
argument checking, an empty call reads nothing; and ``ghost_grid(max_cells=)``."""
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


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


def _int(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_exported_and_bound(lib):
    from mpi_grid_redistribute_amd import _lib
    for name, nargs in (("mgr_ghost_cells_wide", 13), ("mgr_id_digit", 6),
                        ("mgr_cell_offsets", 6)):
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == nargs
    # profiler ids: appended behind the existing ones, which keep their values
    base = len(_lib.PROFILE_KERNELS)
    for i, name in enumerate(_lib.PROFILE_KERNELS + _lib.WIDE_PROFILE_KERNELS):
        assert lib.mgr_profile_kernel_id(name.encode()) == i, name
    assert _lib.WIDE_PROFILE_KERNELS == ("ghost_cells_wide", "id_digit", "cell_offsets")
    assert lib.mgr_profile_kernel_id(b"ghost_cells_wide") == base


def _wide(lib, p, **kw):
    a = dict(pos=p, dt=F32, n=5, no=3, stride=3, dim=3, org=_f64(0, 0, 0), wid=_f64(.1, .1, .1),
             fine=_int(4, 4, 4), gh=_int(1, 1, 1), ids=p, out=None)
    a.update(kw)
    return lib.mgr_ghost_cells_wide(a["pos"], a["dt"], a["n"], a["no"], a["stride"], a["dim"],
                                    a["org"], a["wid"], a["fine"], a["gh"], a["ids"], a["out"],
                                    None)


def test_ghost_cells_wide_refusals(lib):
    buf, p = _p()
    for dt in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, 99):
        assert _wide(lib, p, dt=dt) == EUNSUPPORTED, dt
        assert b"float32" in lib.mgr_last_error()
    for dim in (0, -1, 9):
        assert _wide(lib, p, dim=dim, stride=9) == EINVAL
        assert b"dim" in lib.mgr_last_error()
    assert _wide(lib, p, n=-1, no=0) == EINVAL
    for no in (-1, 6):
        assert _wide(lib, p, no=no) == EINVAL
        assert b"n_owned" in lib.mgr_last_error()
    assert _wide(lib, p, stride=2) == EINVAL
    assert b"row_stride" in lib.mgr_last_error()
    for k in ("pos", "org", "wid", "fine", "gh", "ids"):
        assert _wide(lib, p, **{k: None}) == EINVAL, k
        assert b"null" in lib.mgr_last_error()
    for w in (0.0, -0.5, float("inf"), float("nan")):
        assert _wide(lib, p, wid=_f64(.1, w, .1)) == EINVAL, w
        assert b"width" in lib.mgr_last_error()
    assert _wide(lib, p, org=_f64(0, float("inf"), 0)) == EINVAL
    assert b"origin" in lib.mgr_last_error()
    assert _wide(lib, p, fine=_int(4, 0, 4)) == EINVAL
    assert b"fine" in lib.mgr_last_error()
    assert _wide(lib, p, gh=_int(1, 1, -1)) == EINVAL
    assert b"ghost" in lib.mgr_last_error()
    # the bound is 2^20 cells, named in the message; the product does not overflow
    assert _wide(lib, p, fine=_int(128, 128, 64), gh=_int(0, 0, 1)) == EINVAL     # 2^20 + 2^15
    assert b"2^20" in lib.mgr_last_error() and b"1048576" in lib.mgr_last_error()
    assert _wide(lib, p, fine=_int(2 ** 30, 2 ** 30, 2 ** 30)) == EINVAL
    assert b"2^20" in lib.mgr_last_error()
    assert _wide(lib, p, dim=1, fine=_int(2 ** 20 - 1), gh=_int(1)) == EINVAL      # 2^20 + 1
    assert b"2^20" in lib.mgr_last_error()
    assert _wide(lib, p, dim=2, stride=2, fine=_int(2 ** 20 + 1, 1), gh=_int(0, 0)) == EINVAL
    # the 16-bit entry keeps its bound and its message
    assert lib.mgr_ghost_cells(p, F32, 5, 3, 3, 3, _f64(0, 0, 0), _f64(.1, .1, .1),
                               _int(8, 8, 8), _int(2, 2, 2), p, None, None) == EINVAL
    assert b"beyond 1024 cells" in lib.mgr_last_error()


def test_ghost_cells_wide_accepted_boundaries(lib):
    """prod(E) == 2^20 passes argument checking; so do 12^3 cells (refused by
    the 16-bit entry).  What follows argument checking is the launch: it
    succeeds on a GPU and fails in HIP (not MGR_EINVAL) without one."""
    import torch
    if torch.cuda.is_available():
        pos = torch.zeros((5, 3), dtype=torch.float32, device="cuda")
        ids = torch.zeros(8, dtype=torch.int32, device="cuda")
        p, q = ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(ids.data_ptr())
    else:
        buf, p = _p()
        q = p
    for fine, gh in ((_int(128, 128, 64), _int(0, 0, 0)),        # 2^20 exactly
                     (_int(126, 126, 62), _int(1, 1, 1)),        # 2^20 with ghost layers
                     (_int(8, 8, 8), _int(2, 2, 2))):            # 12^3
        rc = _wide(lib, p, ids=q, fine=fine, gh=gh)
        assert rc != EINVAL and rc != EUNSUPPORTED, lib.mgr_last_error()
        if torch.cuda.is_available():
            assert rc == 0
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def test_id_digit_refusals(lib):
    buf, p = _p()
    f = lib.mgr_id_digit
    for bits in (0, -1, 17, 32):
        assert f(p, 4, 0, bits, p, None) == EINVAL
        assert b"bits" in lib.mgr_last_error()
    for shift in (-1, 32, 100):
        assert f(p, 4, shift, 1, p, None) == EINVAL
        assert b"shift" in lib.mgr_last_error()
    for shift, bits in ((31, 2), (17, 16), (24, 9)):
        assert f(p, 4, shift, bits, p, None) == EINVAL
        assert b"> 32" in lib.mgr_last_error()
    assert f(p, -1, 0, 10, p, None) == EINVAL
    assert b"n < 0" in lib.mgr_last_error()
    assert f(None, 4, 0, 10, p, None) == EINVAL and b"null" in lib.mgr_last_error()
    assert f(p, 4, 0, 10, None, None) == EINVAL and b"null" in lib.mgr_last_error()


def test_cell_offsets_refusals(lib):
    buf, p = _p()
    f = lib.mgr_cell_offsets
    for nc in (0, -1, (1 << 20) + 1, 1 << 40):
        assert f(p, 4, nc, p, None, None) == EINVAL
        assert b"ncells" in lib.mgr_last_error() and b"2^20" in lib.mgr_last_error()
    assert f(p, -1, 8, p, None, None) == EINVAL
    assert b"n < 0" in lib.mgr_last_error()
    assert f(None, 4, 8, p, None, None) == EINVAL
    assert b"null sorted_ids" in lib.mgr_last_error()
    for n in (0, 4):
        assert f(p, n, 8, None, None, None) == EINVAL
        assert b"null offsets" in lib.mgr_last_error()


def test_empty_reads_nothing(lib):
    for dt in (F32, F64):
        assert lib.mgr_ghost_cells_wide(None, dt, 0, 0, 3, 3, None, None, None, None, None, None,
                                        None) == 0
    for shift, bits in ((0, 1), (0, 16), (16, 16), (31, 1), (10, 10)):
        assert lib.mgr_id_digit(None, 0, shift, bits, None, None) == 0


def _grid(cell, fine, ol, low=0.0, **kw):
    from mpi_grid_redistribute_amd import ghost_grid
    cl = np.asarray(cell, dtype=np.float64)
    lim = np.stack([np.full(len(cl), low), low + cl], axis=1)
    return ghost_grid(cl, lim, fine, ol, **kw)


def test_ghost_grid_max_cells():
    from mpi_grid_redistribute_amd import CELLS_MAX, GHOST_MAX_CELLS
    assert GHOST_MAX_CELLS == 1024 and CELLS_MAX == 1 << 20
    # 12^3: refused by default with today's message, accepted with max_cells
    with pytest.raises(ValueError, match=r"at most 1024 \(the ranked sort's bound\)"):
        _grid([1.0] * 3, [8, 8, 8], [0.25] * 3)
    ghost, ext, origin, width = _grid([1.0] * 3, [8, 8, 8], [0.25] * 3, max_cells=CELLS_MAX)
    assert ghost.tolist() == [2, 2, 2] and ext.tolist() == [12, 12, 12]
    assert width.tolist() == [0.125] * 3 and origin.tolist() == [0.0] * 3
    # the bound follows max_cells: cells and ghost layers
    assert _grid([1.0] * 3, [8, 8, 8], [0.25] * 3, max_cells=1728)[1].tolist() == [12] * 3
    with pytest.raises(ValueError, match="1727"):
        _grid([1.0] * 3, [8, 8, 8], [0.25] * 3, max_cells=1727)
    with pytest.raises(ValueError, match="1024"):
        _grid([1.0], [4], [1000.0])                                      # 4000 layers
    assert _grid([1.0], [4], [1000.0], max_cells=CELLS_MAX)[0].tolist() == [4000]
    assert _grid([1.0] * 3, [128, 128, 64], [0, 0, 0], max_cells=CELLS_MAX)[1].tolist() == \
        [128, 128, 64]                                                   # 2^20 exactly
    with pytest.raises(ValueError, match=str(CELLS_MAX)):
        _grid([1.0] * 3, [128, 128, 65], [0, 0, 0], max_cells=CELLS_MAX)
    # max_cells out of range
    for bad in (0, -1, CELLS_MAX + 1):
        with pytest.raises(ValueError, match="max_cells"):
            _grid([1.0] * 3, [4, 4, 4], [0.1] * 3, max_cells=bad)
    # where both accept, the values are the default call's
    for cell, fine, ol, low in (([1.0, 0.5, 0.25], [8, 4, 2], [0, 0, 0], 0.5),
                                ([1.0] * 3, [8, 8, 4], [0.25, 0.125, 0.5], 0.0),
                                ([0.5, 0.5], [4, 2], [0.75, 0.6], 0.0), ([1.0 / 3.0], [7], [0.01], 0.0)):
        a, b = _grid(cell, fine, ol, low), _grid(cell, fine, ol, low, max_cells=CELLS_MAX)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_digit_split():
    from mpi_grid_redistribute_amd import sort
    for ncells in (1025, 2048, 2049, 4096, 13824, 66 ** 3, (1 << 20) - 1, 1 << 20):
        for split in ("balanced", "low10"):
            b0, b1, nb0, nb1 = sort._digit_split(ncells, split)
            assert 1 <= b0 <= 10 and 1 <= b1 <= 10 and nb0 == 1 << b0
            assert (1 << (b0 + b1)) >= ncells
            assert nb1 == -(-ncells // nb0) and 1 <= nb1 <= 1 << b1
    assert sort._digit_split(13824, "balanced")[:2] == (7, 7)
    assert sort._digit_split(13824, "low10")[:2] == (10, 4)
    assert sort.WIDE_SPLIT in ("balanced", "low10")
    with pytest.raises(ValueError):
        sort._digit_split((1 << 20) + 1)
