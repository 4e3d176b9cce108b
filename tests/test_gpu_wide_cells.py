"""Cell lists beyond 1024 cells: the three kernels alone, the two-digit stable
sort, and ``ghost_cell_sort(..., max_cells=CELLS_MAX)`` end to end, bit for bit
against numpy: cell ids by a float64 floor with the owned rows clamped (as
tests/test_gpu_ghost_halo.py's _model_cells), order by a stable argsort,
offsets by searchsorted."""
import ctypes

import numpy as np
import pytest
import torch

from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import (CELLS_MAX, MPIGridRedistributor, SortRoute,  # noqa: E402
                                       _lib)

F32, F64 = 1, 2
M = 1_000_000


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------ the model
def _model_ids(pos, n_owned, origin, width, fine, ghost):
    """(ids, outside count): float64 floor, owned rows clamped into the
    interior, halo rows into the extended grid and counted when that (or a
    NaN) changed them."""
    fine, ghost = np.asarray(fine, dtype=np.int64), np.asarray(ghost, dtype=np.int64)
    dim = len(fine)
    ext = fine + 2 * ghost
    with np.errstate(invalid="ignore"):
        kd = np.floor((pos[:, :dim].astype(np.float64) - origin) / width) + ghost
    owned = (np.arange(len(pos)) < n_owned)[:, None]
    lo = np.where(owned, ghost, 0).astype(np.float64)
    hi = np.where(owned, ghost + fine - 1, ext - 1).astype(np.float64)
    inside = (kd >= lo) & (kd <= hi)                       # NaN: False
    k = np.where(np.isnan(kd) | (kd < lo), lo, np.minimum(kd, hi)).astype(np.int64)
    off = np.ones(dim, dtype=np.int64)
    for d in range(dim - 2, -1, -1):
        off[d] = off[d + 1] * ext[d + 1]
    outside = int((~owned[:, 0] & ~inside.all(axis=1)).sum())
    return (k * off).sum(axis=1), outside


def _offsets(sorted_ids, ncells):
    return np.searchsorted(sorted_ids, np.arange(ncells + 1)).astype(np.int64)


# ----------------------------------------------------- kernels alone
def _cells_call(name, pos, n_owned, origin, width, fine, ghost, idt):
    n, dim = len(pos), len(fine)
    t = _dev(pos)
    ids = torch.full((n + 8,), -1, dtype=idt, device="cuda")     # 8 guard entries
    out = torch.zeros(1, dtype=torch.int32, device="cuda")
    code = F32 if pos.dtype == np.float32 else F64
    _lib.call(name, _lib.ptr(t), code, n, n_owned, pos.shape[1], dim,
              _vp(np.asarray(origin, dtype=np.float64)), _vp(np.asarray(width, dtype=np.float64)),
              (ctypes.c_int * dim)(*fine), (ctypes.c_int * dim)(*ghost), _lib.ptr(ids),
              _lib.ptr(out), _lib.stream_handle())
    torch.cuda.synchronize()
    assert (ids[n:] == -1).all(), "wrote past n"
    return ids[:n].cpu().numpy(), int(out.item())


# (fine, ghost): 1025, 4096, 24^3 and 2^20 cells, in 1 to 3 dimensions
GRIDS = [([1023], [1]), ([4096], [0]), ([60, 60], [2, 2]), ([33, 30], [0, 1]),
         ([16, 16, 16], [4, 4, 4]), ([126, 126, 62], [1, 1, 1]), ([1024, 1024], [0, 0])]


def _grid_rows(rng, n, fine, ghost, dt, stride):
    """n rows, half owned: owned rows over the cell with some exactly on its
    faces, halo rows over the layers with one a cell beyond them and one NaN."""
    dim = len(fine)
    fine_a, ghost_a = np.asarray(fine, dtype=np.float64), np.asarray(ghost, dtype=np.float64)
    origin = np.full(dim, 0.25)
    width = 0.5 / fine_a
    n_owned = n // 2
    pos = np.zeros((n, stride))
    pos[:, dim:] = 77.0                                       # columns the kernel must not read as coordinates
    pos[:n_owned, :dim] = origin + rng.random((n_owned, dim)) * 0.5
    u = rng.random((n - n_owned, dim))
    pos[n_owned:, :dim] = origin + (u * (fine_a + 2 * ghost_a) - ghost_a) * width
    if n_owned >= 3:
        pos[0, :dim] = origin + 0.5                           # the upper face: clamped inwards
        pos[1, :dim] = origin
        pos[2, 0] = origin[0] + 0.5 + 3 * width[0]            # an owned row outside: clamped, not counted
    if n - n_owned >= 3:
        pos[n_owned, :dim] = origin + 0.5 + (ghost_a + 1.5) * width     # one cell beyond
        pos[n_owned + 1, 0] = np.nan
        pos[n_owned + 2, :dim] = origin - (ghost_a + 0.5) * width       # one cell below
    return pos.astype(dt), n_owned, origin, width


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("fine,ghost", GRIDS)
def test_ghost_cells_wide_matches_the_model(fine, ghost, dt):
    rng = np.random.default_rng(len(fine) * 100 + fine[0])
    dim = len(fine)
    for n in (1, 63, 64, 65, 1000):
        for stride in (dim, dim + 2):
            pos, n_owned, origin, width = _grid_rows(rng, n, fine, ghost, dt, stride)
            got, outside = _cells_call("mgr_ghost_cells_wide", pos, n_owned, origin, width, fine,
                                       ghost, torch.int32)
            exp, exp_out = _model_ids(pos, n_owned, origin, width, fine, ghost)
            assert np.array_equal(got.view(np.uint32), exp.astype(np.uint32)), (n, stride)
            assert outside == exp_out, (n, stride)
            if n == 1000:
                assert exp_out >= 3 and exp.max() >= 1024


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_wide_equals_the_16_bit_entry_on_small_grids(dt):
    rng = np.random.default_rng(5)
    for fine, ghost in (([8, 8, 8], [1, 1, 1]), ([1024], [0]), ([30, 30], [1, 1])):
        for n in (65, 1000):
            pos, n_owned, origin, width = _grid_rows(rng, n, fine, ghost, dt, len(fine) + 1)
            a, ao = _cells_call("mgr_ghost_cells", pos, n_owned, origin, width, fine, ghost,
                                torch.int16)
            b, bo = _cells_call("mgr_ghost_cells_wide", pos, n_owned, origin, width, fine, ghost,
                                torch.int32)
            assert np.array_equal(a.view(np.uint16).astype(np.uint32), b.view(np.uint32))
            assert ao == bo > 0


def test_id_digit():
    rng = np.random.default_rng(9)
    for n in (1, 7, 8, 9, 4097):
        ids = rng.integers(0, 1 << 32, n + 3, dtype=np.uint64).astype(np.uint32)
        ids[: min(n, 4)] = [0xFFFFFFFF, 0, 0x80000001, 0x0001FFFF][: min(n, 4)]
        t = _dev(ids.view(np.int32))
        for shift, bits in ((0, 1), (0, 16), (16, 16), (31, 1), (0, 10), (10, 10), (7, 7),
                            (22, 10)):
            for skew in (0, 1, 3):        # ids (and out) off the 16-byte boundary
                out = torch.full((n + 16,), -1, dtype=torch.int16, device="cuda")
                _lib.call("mgr_id_digit", ctypes.c_void_p(t.data_ptr() + 4 * skew), n, shift, bits,
                          ctypes.c_void_p(out.data_ptr() + 2 * skew), _lib.stream_handle())
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint16)
                exp = ((ids[skew: skew + n] >> np.uint32(shift))
                       & np.uint32((1 << bits) - 1)).astype(np.uint16)
                assert np.array_equal(got[skew: skew + n], exp), (n, shift, bits, skew)
                assert (got[:skew] == 0xFFFF).all() and (got[skew + n:] == 0xFFFF).all()


def _cell_offsets(ids, ncells, with_bad=True):
    n = len(ids)
    t = _dev(np.asarray(ids, dtype=np.uint32).view(np.int32)) if n else None
    offs = torch.full((ncells + 2,), -7, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda") if with_bad else None
    _lib.call("mgr_cell_offsets", _lib.ptr(t), n, ncells, _lib.ptr(offs), _lib.ptr(bad),
              _lib.stream_handle())
    torch.cuda.synchronize()
    assert int(offs[-1]) == -7, "wrote past ncells + 1"
    return offs[:-1].cpu().numpy(), (int(bad.item()) if with_bad else None)


def test_cell_offsets():
    big = 1 << 20
    cases = [
        (np.zeros(1000, dtype=np.int64), 5000),                          # all rows in cell 0
        (np.full(1000, 4999), 5000),                                     # all in the last cell
        (np.repeat([0, big - 1], [300, 700]), big),                      # one long gap
        (np.arange(3000), 3000),                                         # every row its own cell
        (np.arange(3000) * 300 + 17, big),
        (np.sort(np.random.default_rng(1).integers(0, 13824, 20000)), 13824),
        (np.array([5]), 1025), (np.zeros(0, dtype=np.int64), 1025), (np.zeros(0, dtype=np.int64), 1),
        (np.zeros(100, dtype=np.int64), 1),
    ]
    for ids, ncells in cases:
        got, bad = _cell_offsets(ids, ncells)
        assert bad == 0
        assert np.array_equal(got, _offsets(ids, ncells)), (len(ids), ncells)
        assert got[0] == 0 and got[-1] == len(ids)
    got, bad = _cell_offsets(np.arange(100), 200, with_bad=False)        # bad may be NULL
    assert np.array_equal(got, _offsets(np.arange(100), 200))
    # an unsorted input, and an id >= ncells: each counted
    ids = np.arange(1000)
    ids[[10, 500]] = [3, 2]
    assert _cell_offsets(ids, 2000)[1] == 2
    ids = np.arange(1000)
    ids[-1] = 2000
    offs, bad = _cell_offsets(ids, 2000)
    assert bad == 1 and offs[-1] == 999
    assert _cell_offsets(np.array([1 << 20]), 1 << 20)[1] == 1
    assert _cell_offsets(np.array([0xFFFFFFFF, 0]), 8)[1] == 2


# -------------------------------------------------------------- the sort
# Through the public call on a 1-D grid of ``ncells`` fine cells without a halo
# (n_local = n, overload 0: the plain large cell list): the position (id + 0.5)
# / ncells lies in cell id.
RANKED = [(np.int32, ()), (np.int32, (3,)), (np.int32, (9,)), (np.int32, (16,))]   # 4, 12, 36, 64 B
GENERIC = [(np.int16, ()), (np.int16, (3,)), (np.int64, (9,))]                     # 2, 6, 72 B
MIXED = [(np.int32, (3,)), (np.int16, (3,)), (np.int64, ())]
SETS = {"ranked": RANKED, "generic": GENERIC, "mixed": MIXED}


def _fields(n, kinds):
    """Payload = the row index (plus the column), so stability is visible."""
    out = []
    for dt, trailing in kinds:
        a = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * len(trailing))
        a = a + np.arange(int(np.prod(trailing, dtype=np.int64))).reshape(trailing) * 3
        out.append(np.ascontiguousarray(np.broadcast_to(a, (n,) + trailing).astype(dt)))
    return tuple(out)


def _dist(rng, name, n, ncells):
    if name == "uniform":
        return rng.integers(0, ncells, n)
    if name == "one_cell":
        return np.full(n, ncells // 3, dtype=np.int64)
    if name == "two_ends":
        return np.where(rng.random(n) < 0.5, 0, ncells - 1).astype(np.int64)
    return rng.integers(0, 7, n) * (ncells // 7) + rng.integers(0, 2, n)      # heavy duplicates


_R1 = {}


def _red1():
    if "r" not in _R1:
        _R1["r"] = MPIGridRedistributor(None, [1], [1.0])
    return _R1["r"]


@pytest.mark.parametrize("ncells", [1025, 2048, 13824, 1 << 20])
@pytest.mark.parametrize("n", [0, 1, 64, 4095, 4096, 4097, 20000])
def test_wide_sort_matches_the_model(n, ncells):
    R = _red1()
    rng = np.random.default_rng(n * 31 + ncells)
    for dist in ("uniform", "one_cell", "two_ends", "duplicates"):
        ids = _dist(rng, dist, n, ncells)
        pos = ((ids + 0.5) / ncells).reshape(n, 1)
        model, _ = _model_ids(pos, n, np.zeros(1), np.array([1.0]) / np.array([ncells]), [ncells],
                              [0])
        assert np.array_equal(model, ids)
        order = np.argsort(ids, kind="stable")
        exp_offs = _offsets(ids[order], ncells)
        for name, kinds in SETS.items():
            if dist != "uniform" and name == "mixed":
                continue
            fields = _fields(n, kinds)
            srt, spos, offs, sroute = R.ghost_cell_sort(
                fields, pos, n, [ncells], [0.0], return_positions=True, return_route=True,
                max_cells=CELLS_MAX)
            assert offs.dtype == np.int64 and np.array_equal(offs, exp_offs), (dist, name)
            for f, s in zip(fields, srt):
                assert s.dtype == f.dtype and s.tobytes() == f[order].tobytes(), (dist, name)
            assert spos.tobytes() == pos[order].tobytes()
            assert isinstance(sroute, SortRoute) and sroute.n == n and not sroute.released
            back = R.unsort(srt, sroute)
            for f, b in zip(fields, back):
                assert b.tobytes() == f.tobytes(), (dist, name)
            if name == "ranked":     # a result array of another dtype and shape
                vals = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
                assert R.unsort(vals[order], sroute).tobytes() == vals.tobytes()
            sroute.release()
            assert sroute.released
            with pytest.raises(ValueError, match="released"):
                R.unsort(srt, sroute)


def test_both_digit_splits_sort_alike():
    from mpi_grid_redistribute_amd import sort
    n, ncells = 20000, 66 ** 3
    rng = np.random.default_rng(3)
    ids = rng.integers(0, ncells, n)
    order = np.argsort(ids, kind="stable")
    rec = _dev(_fields(n, [(np.int32, (9,))])[0])
    for split in ("balanced", "low10"):
        outs, offs = sort._sort_by_wide_ids([sort._IdField(rec.view(torch.uint8).reshape(-1), 36)],
                                            _dev(ids.astype(np.int32)), n, ncells, rec.device,
                                            split=split)
        assert np.array_equal(offs.cpu().numpy(), _offsets(ids[order], ncells))
        assert np.array_equal(outs[0].cpu().numpy().view(np.int32).reshape(n, 9)[:, 0], order)
    # an id >= ncells: every offset -1 on the device, no sync
    ids[77] = ncells
    _, offs = sort._sort_by_wide_ids([sort._IdField(rec.view(torch.uint8).reshape(-1), 36)],
                                     _dev(ids.astype(np.int32)), n, ncells, rec.device)
    assert (offs == -1).all()


# ------------------------------------------------------------ end to end
ROWS, FINE = 3000, 16
LAYOUTS = {"one_3d": [1, 1, 1], "t_222": [2, 2, 2]}


def _val(ids, q):
    return ids % 11 + 3 * q + 1


def _local_rows(topo, r, rows, dt, seed=7):
    rng = np.random.default_rng(seed + r)
    idx = np.array(np.unravel_index(r, topo))
    pos = ((idx + rng.random((rows, len(topo)))) / np.asarray(topo)).astype(dt)
    return np.arange(rows, dtype=np.int64) + M * r, pos


_cache = {}


def _run(name, dt):
    key = (name, np.dtype(dt).name)
    if key in _cache:
        return _cache[key]
    topo = LAYOUTS[name]
    size = int(np.prod(topo))
    ol = [0.2 / t for t in topo]

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, [1.0] * 3)
        ids, pos = _local_rows(topo, r, ROWS, dt)
        h, p, hroute = R.exchange_overload_by_position(ids, pos, ol, return_positions=True,
                                                       unwrap=True, return_route=True)
        both, bpos = np.concatenate([ids, h]), np.concatenate([pos, p])
        grid = R.ghost_grid([FINE] * 3, ol, max_cells=CELLS_MAX)
        srt, spos, offs, sroute = R.ghost_cell_sort(both, bpos, len(ids), [FINE] * 3, ol,
                                                    return_positions=True, return_route=True,
                                                    max_cells=CELLS_MAX)
        assert isinstance(sroute, SortRoute) and sroute.n == len(both)
        vals = R.unsort(_val(srt, r), sroute)
        summed = R.reduce_overload(vals[len(ids):], hroute, local_values=vals[: len(ids)])
        # the halo-less list of the owned rows, and row-indexed values home through both routes
        (lids, lpos), route = R.redistribute_by_position(ids, pos.copy(), return_positions=True,
                                                         return_route=True)
        lsrt, loffs, lroute = R.ghost_cell_sort(lids, lpos, len(lids), [FINE] * 3, [0.0] * 3,
                                                return_route=True, max_cells=CELLS_MAX)
        home = R.return_to_source(lsrt * 2 + 1, route, sort_route=lroute)
        with pytest.raises(ValueError, match="1024"):
            R.ghost_cell_sort(both, bpos, len(ids), [FINE] * 3, ol)
        torch.cuda.synchronize()
        return dict(ids=ids, pos=pos, h=h, p=p, grid=grid, srt=srt, spos=spos, offs=offs, vals=vals,
                    summed=summed, lids=lids, lsrt=lsrt, loffs=loffs, home=home)

    _cache[key] = run_ranks(size, fn)
    return _cache[key]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_ghost_cell_sort_wide_end_to_end(name, dt):
    topo = LAYOUTS[name]
    size = int(np.prod(topo))
    outs = _run(name, dt)
    for r, o in enumerate(outs):
        ghost, ext, origin, width = o["grid"]
        assert ghost.tolist() == [4] * 3 and ext.tolist() == [24] * 3
        nl = len(o["ids"])
        both, bpos = np.concatenate([o["ids"], o["h"]]), np.concatenate([o["pos"], o["p"]])
        assert len(both) > nl
        cells, outside = _model_ids(bpos, nl, origin, width, [FINE] * 3, ghost)
        assert outside == 0
        # the interior block holds exactly the owned rows
        k = np.stack(np.unravel_index(cells, tuple(int(e) for e in ext)), axis=1)
        interior = ((k >= 4) & (k < 4 + FINE)).all(axis=1)
        assert np.array_equal(interior, np.arange(len(both)) < nl), (name, r)
        order = np.argsort(cells, kind="stable")
        assert o["offs"].dtype == np.int64 and len(o["offs"]) == 24 ** 3 + 1
        assert np.array_equal(o["offs"], _offsets(cells[order], 24 ** 3))
        assert o["srt"].tobytes() == both[order].tobytes()
        assert o["spos"].tobytes() == bpos[order].tobytes()
        assert np.array_equal(o["vals"], _val(both, r))
        # the halo-less list: 16^3 = 4096 cells, all rows owned; values come home
        assert len(o["loffs"]) == FINE ** 3 + 1 and o["loffs"][-1] == len(o["lids"])
        assert sorted(o["lsrt"].tolist()) == sorted(o["lids"].tolist())
        assert np.array_equal(o["home"], o["ids"] * 2 + 1)
    for r, o in enumerate(outs):   # reduce_overload: own value + the values of all copies
        exp = _val(o["ids"], r).copy()
        for q in range(size):
            h = outs[q]["h"]
            m = h // M == r
            np.add.at(exp, h[m] % M, _val(h[m], q))
        assert np.array_equal(o["summed"], exp), (name, r)


# ------------------------------------------- launches, small grids, failures
ALL_KERNELS = _lib.PROFILE_KERNELS + _lib.WIDE_PROFILE_KERNELS


def _count(call):
    torch.cuda.synchronize()
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        res = call()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    got = {k: int(_lib.profile_read(k)[1]) for k in ALL_KERNELS}
    _lib.profile_reset()
    return res, {k: c for k, c in got.items() if c}


def _owned_and_halo(n, ol, seed=2):
    """n owned rows in the unit cell and n / 4 halo rows within ol of it, as
    36-byte records' SoA fields (positions, velocities, masses) on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pos = torch.rand((n + n // 4, 3), generator=g, device="cuda", dtype=torch.float32)
    pos[n:] = pos[n:] * (1 + 1.8 * ol) - 0.9 * ol
    vel = torch.arange(3 * len(pos), device="cuda", dtype=torch.float32).reshape(-1, 3)
    mass = torch.arange(len(pos), device="cuda", dtype=torch.float32)
    return pos, vel, mass, n


def test_small_grids_are_unchanged():
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    pos, vel, mass, nl = _owned_and_halo(3000, 0.1)
    fine, ol = [8, 8, 8], [0.1] * 3                      # 10^3 cells
    for data in (vel, (pos, vel, mass)):
        a, ca = _count(lambda: R.ghost_cell_sort(data, pos, nl, fine, ol, return_positions=True))
        b, cb = _count(lambda: R.ghost_cell_sort(data, pos, nl, fine, ol, return_positions=True,
                                                 max_cells=CELLS_MAX))
        assert ca == cb and not set(cb) & set(_lib.WIDE_PROFILE_KERNELS)
        flat = lambda res: [res[0]] if torch.is_tensor(res[0]) else list(res[0])  # noqa: E731
        for x, y in zip(flat(a) + list(a[1:]), flat(b) + list(b[1:])):
            assert x.dtype == y.dtype and torch.equal(x, y)
        assert int(a[2][-1]) == len(pos)


@pytest.mark.parametrize("soa", [False, True])
def test_wide_launch_counts(soa):
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    pos, vel, mass, nl = _owned_and_halo(3000, 0.2)
    data, F = ((pos, vel, mass), 3) if soa else (vel, 1)
    res, got = _count(lambda: R.ghost_cell_sort(data, pos, nl, [16] * 3, [0.2] * 3,
                                                max_cells=CELLS_MAX))
    print(got)
    assert int(res[1][-1]) == len(pos) and len(res[1]) == 24 ** 3 + 1
    assert got == {"ghost_cells_wide": 1, "id_digit": 2, "count_ids": 2, "scan": 2,
                   "pack_fine": 2 * (F + 1), "cell_offsets": 1}
    # the way back: one launch per pass
    _, _, sroute = R.ghost_cell_sort(data, pos, nl, [16] * 3, [0.2] * 3, return_route=True,
                                     max_cells=CELLS_MAX)
    _, got = _count(lambda: R.unsort(res[0], sroute))
    assert got == {"unpack_ranked": 2}


def test_failure_paths():
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    pos = np.random.default_rng(4).random((101, 3))
    for x in (1.3, np.nan):
        far = pos.copy()
        far[100] = [0.5, x, 0.5]                         # a halo row beyond the 4 layers
        with pytest.raises(_lib.MgrError, match="beyond the ghost layers"):
            R.ghost_cell_sort(np.arange(101), far, 100, [16] * 3, [0.2] * 3, max_cells=CELLS_MAX)
        _, doffs = R.ghost_cell_sort(torch.arange(101).cuda(), _dev(far), 100, [16] * 3, [0.2] * 3,
                                     max_cells=CELLS_MAX)
        assert doffs.is_cuda and len(doffs) == 24 ** 3 + 1 and (doffs == -1).all()
        # the same row as an owned one is clamped into the cell, silently
        _, offs = R.ghost_cell_sort(np.arange(101), far, 101, [16] * 3, [0.2] * 3,
                                    max_cells=CELLS_MAX)
        assert offs[-1] == 101
    with pytest.raises(ValueError, match="1024"):
        R.ghost_cell_sort(np.arange(101), pos, 101, [16] * 3, [0.2] * 3)
    with pytest.raises(ValueError, match="max_cells"):
        R.ghost_cell_sort(np.arange(101), pos, 101, [16] * 3, [0.2] * 3, max_cells=CELLS_MAX + 1)
    with pytest.raises(ValueError, match="n_local"):
        R.ghost_cell_sort(np.arange(101), pos, 102, [16] * 3, [0.2] * 3, max_cells=CELLS_MAX)
    with pytest.raises(TypeError, match="float32 or float64"):
        R.ghost_cell_sort(np.arange(101), pos.astype(np.float16), 101, [16] * 3, [0.2] * 3,
                          max_cells=CELLS_MAX)
