"""mgr_shift_regions and mgr_ghost_cells against numpy models written here.

Shift: ``pos[row, d] + T(shift)`` computed by numpy in the positions' dtype,
so the whole buffer -- shifted coordinates, zero-shift coordinates with a -0.0
and a NaN payload, the columns beyond ``dim`` -- compares as raw bytes.
Ghost cells: ``floor((float64(x) - origin) / width) + ghost`` by numpy in
float64, clamped as include/mgr.h says; ids and the ``outside`` count are
compared exactly, on positions lying on every cell face and one ulp either
side of it, NaN, +-inf and far outside."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import _lib  # noqa: E402

CODE = {np.float32: _lib.MGR_F32, np.float64: _lib.MGR_F64}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------ shift
def _shift_model(pos, dim, ends, shifts):
    out, b = pos.copy(), 0
    for r, e in enumerate(ends):
        for d in range(dim):
            s = pos.dtype.type(shifts[r][d])
            if s != 0:
                out[b:e, d] = pos[b:e, d] + s
        b = e
    return out


def _shift_gpu(pos, dim, ends, shifts):
    n, stride = pos.shape
    t = torch.from_numpy(pos.copy()).cuda()
    k = len(ends)
    e = (ctypes.c_int64 * k)(*[int(x) for x in ends])
    s = (ctypes.c_double * (k * dim))(*[float(v) for row in shifts for v in row])
    _lib.call("mgr_shift_regions", _lib.ptr(t) if n else None, CODE[pos.dtype.type], n, stride,
              dim, k, e, s, _lib.stream_handle())
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _positions(n, stride, dt, seed):
    """Random rows with special bit patterns sprinkled in every column."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 2.0, (n, stride)).astype(dt)
    u = pos.view(np.uint32 if dt == np.float32 else np.uint64)
    nan = 0x7FC01234 if dt == np.float32 else 0x7FF8000000001234
    for i in range(0, n, 7):
        pos[i, i % stride] = -0.0
    for i in range(3, n, 11):
        u[i, (i + 1) % stride] = nan
    return pos


def _regions(n, k, rng):
    """k region ends over n rows, non-decreasing, ending at n, with empty
    regions wherever the cuts coincide."""
    cuts = np.sort(rng.integers(0, n + 1, k - 1)) if k > 1 else np.zeros(0, np.int64)
    return [int(c) for c in cuts] + [n]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_shift_regions(n, dt):
    rng = np.random.default_rng(n + 1)
    L = 1.0
    for dim, stride in ((3, 3), (3, 5), (2, 4), (1, 1)):
        pos = _positions(n, stride, dt, seed=n * 10 + stride)
        # column `zc` is never shifted: its -0.0 and NaN payloads must survive as bytes;
        # a NaN in a shifted column would pin the payload of NaN + s, which is not a contract
        zc = dim - 1 if dim > 1 else None
        for d in range(dim):
            if d != zc:
                bad = np.isnan(pos[:, d])
                pos[bad, d] = 0.25
        layouts = []
        # the one-rank halo's shape: 26 pieces, shifts of -L / 0 / +L
        ends = _regions(n, 26, rng)
        layouts.append((ends, [[(L * rng.integers(-1, 2)) if d != zc else 0.0 for d in range(dim)]
                               for _ in ends]))
        # empty first, middle and last regions
        a, b = n // 3, (2 * n) // 3
        layouts.append(([0, a, a, b, n, n],
                        [[0.5 if d != zc else 0.0 for d in range(dim)],
                         [-L if d != zc else 0.0 for d in range(dim)], [7.0] * dim,
                         [0.0] * dim, [L if d == 0 and zc != 0 else 0.0 for d in range(dim)],
                         [3.0] * dim]))
        # 64 regions, values that do not round-trip through float32
        ends = _regions(n, 64, rng)
        layouts.append((ends, [[(0.1 * (r + 1) * (-1) ** r) if d != zc else 0.0
                                for d in range(dim)] for r in range(64)]))
        # one region, nothing to do
        layouts.append(([n], [[0.0] * dim]))
        for ends, shifts in layouts:   # (the [7.0] / [3.0] regions are empty)
            got = _shift_gpu(pos, dim, ends, shifts)
            exp = _shift_model(pos, dim, ends, shifts)
            assert got.tobytes() == exp.tobytes(), (n, np.dtype(dt).name, dim, stride, len(ends))
            if n:
                assert got[:, dim:].tobytes() == pos[:, dim:].tobytes()
                if zc is not None:
                    assert got[:, zc].tobytes() == pos[:, zc].tobytes()


@pytest.mark.parametrize("stride,n", [(8192, 1025), ((1 << 22) + 8, 3)])
def test_shift_regions_wide_rows(stride, n):
    """Strides at which the kernel's slab holds fewer than 1024 rows, and one
    row (a stride beyond 2^22): only the first dim elements of a row move."""
    t = torch.zeros((n, stride), dtype=torch.float32, device="cuda")
    t[:, :4] = torch.arange(n * 4, dtype=torch.float32, device="cuda").reshape(n, 4)
    ends = [n // 2, n]
    e = (ctypes.c_int64 * 2)(*ends)
    s = (ctypes.c_double * 6)(1.0, 0.0, -2.0, 0.0, 4.0, 0.5)
    _lib.call("mgr_shift_regions", _lib.ptr(t), _lib.MGR_F32, n, stride, 3, 2, e, s,
              _lib.stream_handle())
    exp = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
    exp[: n // 2, :3] += np.float32([1.0, 0.0, -2.0])
    exp[n // 2:, :3] += np.float32([0.0, 4.0, 0.5])
    assert np.array_equal(t[:, :4].cpu().numpy(), exp)
    assert int(torch.count_nonzero(t[:, 4:])) == 0


# ------------------------------------------------------------ ghost cells
def _ids_model(pos, n_owned, dim, origin, width, fine, ghost):
    ext = fine + 2 * ghost
    off = np.ones(dim, dtype=np.int64)
    for d in range(dim - 2, -1, -1):
        off[d] = off[d + 1] * ext[d + 1]
    x = pos[:, :dim].astype(np.float64)
    with np.errstate(all="ignore"):
        kd = np.floor((x - origin) / width) + ghost
    owned = (np.arange(len(pos)) < n_owned)[:, None]
    lo = np.where(owned, ghost, 0)
    hi = np.where(owned, ghost + fine - 1, ext - 1)
    inside = (kd >= lo) & (kd <= hi)
    with np.errstate(all="ignore"):
        k = np.where(~(kd >= lo), lo, np.where(kd > hi, hi, np.where(inside, kd, 0)))
    ids = (k.astype(np.int64) * off).sum(axis=1)
    return ids.astype(np.uint16), int((~inside & ~owned).any(axis=1).sum()), k.astype(np.int64)


def _ids_gpu(pos, n_owned, dim, origin, width, fine, ghost, count=True):
    n, stride = pos.shape
    t = torch.from_numpy(pos.copy()).cuda()
    ids = torch.full((max(n, 1),), -1, dtype=torch.int16, device="cuda")
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.call("mgr_ghost_cells", _lib.ptr(t) if n else None, CODE[pos.dtype.type], n, n_owned,
              stride, dim, origin.ctypes.data_as(ctypes.c_void_p),
              width.ctypes.data_as(ctypes.c_void_p), (ctypes.c_int * dim)(*[int(v) for v in fine]),
              (ctypes.c_int * dim)(*[int(v) for v in ghost]), _lib.ptr(ids) if n else None,
              _lib.ptr(out) if count else None, _lib.stream_handle())
    torch.cuda.synchronize()
    return ids[:n].cpu().numpy().view(np.uint16), int(out.item())


FINE = {1: [8], 2: [4, 3], 3: [4, 3, 2]}


def _face_values(dt, origin, width, fine, ghost):
    """Per dimension: every face of the extended grid (and two cells beyond),
    the neighbours one ulp either side of it in the positions' dtype, NaN,
    +-inf, and far outside."""
    vals = []
    for d in range(len(fine)):
        j = np.arange(-ghost[d] - 2, fine[d] + ghost[d] + 3)
        f = (origin[d] + j * width[d]).astype(dt)
        v = np.concatenate([f, np.nextafter(f, dt(np.inf)), np.nextafter(f, dt(-np.inf)),
                            np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0], dtype=dt)])
        vals.append(v)
    return vals


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("g", [0, 2])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_ghost_cells(dim, g, dt):
    fine = np.array(FINE[dim], dtype=np.int64)
    ghost = np.full(dim, g, dtype=np.int64)
    cell = np.full(dim, 0.5)
    origin = np.full(dim, 0.5)
    width = cell / fine
    rng = np.random.default_rng(100 * dim + g)
    vals = _face_values(dt, origin, width, fine, ghost)
    for stride in (dim, dim + 2):
        rows = []
        for d in range(dim):          # every special value in dimension d, the others inside
            blk = rng.uniform(0.5, 1.0, (len(vals[d]), stride)).astype(dt)
            blk[:, d] = vals[d]
            rows.append(blk)
        # corners: special values in every dimension at once
        m = max(len(v) for v in vals)
        blk = rng.uniform(0.5, 1.0, (m, stride)).astype(dt)
        for d in range(dim):
            blk[:, d] = np.resize(rng.permutation(vals[d]), m)
        rows.append(blk)
        lo_, hi_ = 0.5 - (g + 1) * width.max(), 1.0 + (g + 1) * width.max()
        rows.append(rng.uniform(lo_, hi_, (4097, stride)).astype(dt))
        halo = np.concatenate(rows)
        # owned rows: inside the cell, and ON its faces -- the upper face included
        own = rng.uniform(0.5, 1.0, (300, stride)).astype(dt)
        own[0, :dim] = (origin + cell).astype(dt)                # rounds onto the upper face
        own[1, :dim] = origin.astype(dt)
        own[2, :dim] = np.nextafter((origin + cell).astype(dt), dt(np.inf))
        own[3, 0] = np.nan
        pos = np.concatenate([own, halo])
        for n_owned in (len(own), 0):
            got, gout = _ids_gpu(pos, n_owned, dim, origin, width, fine, ghost)
            exp, eout, k = _ids_model(pos, n_owned, dim, origin, width, fine, ghost)
            assert np.array_equal(got, exp), (dim, g, np.dtype(dt).name, stride, n_owned)
            assert gout == eout, (gout, eout)
            assert eout > 0 and int(exp.max()) < int(np.prod(fine + 2 * ghost))
        # the owned row on the upper face stays in the interior, silently
        exp, _, k = _ids_model(pos, len(own), dim, origin, width, fine, ghost)
        assert (k[0] == ghost + fine - 1).all() and (k[2] == ghost + fine - 1).all()
        assert (k[: len(own)] >= ghost).all() and (k[: len(own)] <= ghost + fine - 1).all()
        # owned rows only: nothing is outside, whatever they hold; a NULL counter is fine
        got, gout = _ids_gpu(own, len(own), dim, origin, width, fine, ghost)
        assert gout == 0 and np.array_equal(got, exp[: len(own)])
        got, _ = _ids_gpu(pos, len(own), dim, origin, width, fine, ghost, count=False)
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_ghost_cells_small_n(n):
    """Row counts around the 64-row round (the quad store of a full round, the
    tail's single stores); nothing is written past row n."""
    fine, ghost = np.array([4, 3, 2]), np.array([1, 1, 1])
    origin, width = np.zeros(3), 1.0 / fine
    pos = np.random.default_rng(n).uniform(-0.2, 1.2, (n, 3)).astype(np.float32)
    got, gout = _ids_gpu(pos, n // 2, 3, origin, width, fine, ghost)
    exp, eout, _ = _ids_model(pos, n // 2, 3, origin, width, fine, ghost)
    assert np.array_equal(got, exp) and gout == eout == 0
