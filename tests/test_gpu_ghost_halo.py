"""Unwrapped halo positions and the ghost fine-cell sort, against a brute-force
model over all ranks' rows.

The payload is the global row id (rank * M + row).  A copy (row j, image s in
{-1, 0, 1}^dim minus 0) exists on a rank iff in every dimension: s_d = 0 and j's
owner has this rank's cell index; s_d = -1, the owner has the left neighbour's
index and x_d > the neighbour's upper limit - ol_d; s_d = +1, the owner has
the right neighbour's and x_d < its lower limit + ol_d.  Its unwrapped position
is x - L_d where the left neighbour is reached across the box boundary (cell
index 0), x + L_d where the right one is (the last index), computed by numpy
in the position dtype: the multiset of (id, position bytes) must be equal.
With a grid extent of 1, or of 2 and ol > cell / 2, the same row arrives as a
left and a right copy -- identical without ``unwrap`` -- which is what these
tests are for.  The sort is checked against a numpy stable argsort of the
model's cell ids; every layout runs once and its results are shared."""
import itertools

import numpy as np
import pytest
import torch

from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import MPIGridRedistributor, SortRoute  # noqa: E402

M = 1_000_000
ROWS = 3000
FINE = 4

# name -> topology (box 1.0 in every dimension)
LAYOUTS = {
    "one_1d": [1], "one_2d": [1, 1], "one_3d": [1, 1, 1],
    "t_211": [2, 1, 1], "t_221": [2, 2, 1], "t_222": [2, 2, 2], "t_122": [1, 2, 2],
}
# overload length as a fraction of the cell: below and above half of it (above:
# on an extent of 1 or 2 a row is both a left and a right copy)
FRACS = {"lt_half": 0.2, "gt_half": 0.6}
CASES = [(n, f, dt) for n in LAYOUTS for f in FRACS for dt in (np.float64, np.float32)
         if dt == np.float64 or n in ("one_3d", "t_222", "t_211")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _local_rows(topo, r, rows, dt, seed=7):
    rng = np.random.default_rng(seed + r)
    idx = np.array(np.unravel_index(r, topo))
    pos = ((idx + rng.random((rows, len(topo)))) / np.asarray(topo)).astype(dt)
    return np.arange(rows, dtype=np.int64) + M * r, pos


def _ol(topo, frac):
    return [frac / t for t in topo]


def _model_copies(topo, ol, r, ids, pos, dt):
    """(ids, unwrapped positions) of every copy rank r must hold."""
    T = np.asarray(topo)
    dim = len(T)
    box = np.ones(dim)
    cl = box / T
    c = np.array(np.unravel_index(r, topo))
    own = np.stack(np.unravel_index(ids // M, topo), axis=1)
    out_i, out_p = [], []
    for s in itertools.product((-1, 0, 1), repeat=dim):
        if not any(s):
            continue
        ok = np.ones(len(ids), dtype=bool)
        shift = np.zeros(dim)
        for d in range(dim):
            x = pos[:, d].astype(np.float64)
            nb = (c[d] + s[d]) % T[d]
            ok &= own[:, d] == nb
            if s[d] == -1:
                ok &= x > (nb + 1) * cl[d] - ol[d]
                shift[d] = -box[d] if c[d] == 0 else 0.0
            elif s[d] == 1:
                ok &= x < nb * cl[d] + ol[d]
                shift[d] = box[d] if c[d] == T[d] - 1 else 0.0
        p = pos[ok].copy()
        for d in range(dim):
            if shift[d]:
                p[:, d] = p[:, d] + dt(shift[d])       # one add in the position dtype
        out_i.append(ids[ok])
        out_p.append(p)
    return np.concatenate(out_i), np.concatenate(out_p)


def _multiset(ids, pos):
    return sorted(zip(ids.tolist(), [p.tobytes() for p in pos]))


def _model_cells(topo, ol, r, pos, n_local):
    """Cell ids over the extended grid by numpy in float64; (ids, ghost, ext)."""
    T = np.asarray(topo)
    dim = len(T)
    cl = np.ones(dim) / T
    width = cl / FINE
    ghost = np.where(np.asarray(ol) == 0, 0, np.ceil(np.asarray(ol) / width)).astype(np.int64)
    ext = FINE + 2 * ghost
    origin = np.array(np.unravel_index(r, topo)) * cl
    k = np.floor((pos[:, :dim].astype(np.float64) - origin) / width).astype(np.int64) + ghost
    owned = (np.arange(len(pos)) < n_local)[:, None]
    k = np.where(owned, np.clip(k, ghost, ghost + FINE - 1), k)
    assert (k >= 0).all() and (k < ext).all(), "a halo row beyond the ghost layers"
    off = np.ones(dim, dtype=np.int64)
    for d in range(dim - 2, -1, -1):
        off[d] = off[d + 1] * ext[d + 1]
    interior = ((k >= ghost) & (k < ghost + FINE)).all(axis=1)
    return (k * off).sum(axis=1), ghost, ext, interior


def _val(ids, q):
    """An int64 value for row id ``ids`` held on rank q."""
    return ids % 11 + 3 * q + 1


_cache = {}


def _run(name, frac, dt, rows=ROWS):
    key = (name, frac, np.dtype(dt).name, rows)
    if key in _cache:
        return _cache[key]
    topo = LAYOUTS[name]
    size = int(np.prod(topo))
    ol = _ol(topo, FRACS[frac])
    fine = [FINE] * len(topo)

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, [1.0] * len(topo))
        ids, pos = _local_rows(topo, r, rows, dt)
        h0, p0 = R.exchange_overload_by_position(ids, pos, ol, return_positions=True)
        h1, p1, hroute = R.exchange_overload_by_position(ids, pos, ol, return_positions=True,
                                                         unwrap=True, return_route=True)
        both, bpos = np.concatenate([ids, h1]), np.concatenate([pos, p1])
        srt, spos, offs, sroute = R.ghost_cell_sort(both, bpos, len(ids), fine, ol,
                                                    return_positions=True, return_route=True)
        assert isinstance(sroute, SortRoute) and sroute.n == len(both)
        # per sorted row a value; back to the owned + halo layout; copies onto owners
        vals = R.unsort(_val(srt, r), sroute)
        summed = R.reduce_overload(vals[len(ids):], hroute, local_values=vals[: len(ids)])
        torch.cuda.synchronize()
        return dict(ids=ids, pos=pos, h0=h0, p0=p0, h1=h1, p1=p1, srt=srt, spos=spos, offs=offs,
                    vals=vals, summed=summed)

    out = run_ranks(size, fn)
    _cache[key] = out
    return out


@pytest.mark.parametrize("name,frac,dt", CASES)
def test_unwrapped_positions_match_the_model(name, frac, dt):
    topo = LAYOUTS[name]
    outs = _run(name, frac, dt)
    ol = _ol(topo, FRACS[frac])
    ids = np.concatenate([o["ids"] for o in outs])
    pos = np.concatenate([o["pos"] for o in outs])
    for r, o in enumerate(outs):
        # data, counts and order are the unwrap=False call's
        assert o["h1"].tobytes() == o["h0"].tobytes(), (name, r)
        assert o["p1"].dtype == np.dtype(dt) and o["p1"].shape == o["p0"].shape
        mi, mp = _model_copies(topo, ol, r, ids, pos, dt)
        assert len(mi) == len(o["h1"]) > 0
        assert _multiset(o["h1"], o["p1"]) == _multiset(mi, mp), (name, frac, r)
        # every copy lies within ol of the cell (up to the rounding of x + L)
        c = np.array(np.unravel_index(r, topo)) / np.asarray(topo)
        lo, hi = c - np.asarray(ol) - 1e-6, c + 1.0 / np.asarray(topo) + np.asarray(ol) + 1e-6
        assert (o["p1"] >= lo).all() and (o["p1"] <= hi).all()
    if frac == "gt_half":
        # the ambiguous case is really there: some row arrives more than once on a rank, and
        # without unwrap two of its copies carry identical positions
        dup = 0
        for o in outs:
            m0 = _multiset(o["h0"], o["p0"])
            dup += len(m0) - len(set(m0))
            m1 = _multiset(o["h1"], o["p1"])
            assert len(m1) == len(set(m1)), "unwrapped copies of a row must differ"
        assert dup > 0


@pytest.mark.parametrize("name,frac,dt", CASES)
def test_ghost_sort_matches_the_model(name, frac, dt):
    topo = LAYOUTS[name]
    size = int(np.prod(topo))
    outs = _run(name, frac, dt)
    ol = _ol(topo, FRACS[frac])
    for r, o in enumerate(outs):
        nl = len(o["ids"])
        both = np.concatenate([o["ids"], o["h1"]])
        bpos = np.concatenate([o["pos"], o["p1"]])
        cells, ghost, ext, interior = _model_cells(topo, ol, r, bpos, nl)
        # the interior block holds exactly the owned rows
        assert np.array_equal(interior, np.arange(len(both)) < nl), (name, r)
        order = np.argsort(cells, kind="stable")
        exp_offs = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=int(np.prod(ext))))])
        assert o["offs"].dtype == np.int64 and np.array_equal(o["offs"], exp_offs)
        assert o["srt"].tobytes() == both[order].tobytes()
        assert o["spos"].tobytes() == bpos[order].tobytes()
        # unsort: every row of the owned + halo layout got the value of its sorted row
        assert np.array_equal(o["vals"], _val(both, r))
    # reduce_overload: own value + the values of all copies, anywhere
    for r, o in enumerate(outs):
        exp = _val(o["ids"], r).copy()
        for q in range(size):
            h = outs[q]["h1"]
            m = h // M == r
            np.add.at(exp, h[m] % M, _val(h[m], q))
        assert np.array_equal(o["summed"], exp), (name, r)


@pytest.mark.parametrize("rows", [0, 1])
def test_tiny_inputs(rows):
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    ol = [0.3] * 3
    ids = np.arange(rows, dtype=np.int64)
    pos = np.full((rows, 3), 0.125)                    # near the low corner: 7 copies
    h, p = R.exchange_overload_by_position(ids, pos, ol, return_positions=True, unwrap=True)
    assert len(h) == 7 * rows and p.shape == (7 * rows, 3)
    if rows:
        exp = sorted(tuple(0.125 + np.array(s)) for s in itertools.product((0, 1), repeat=3)
                     if any(s))
        assert sorted(map(tuple, p)) == exp
    srt, offs = R.ghost_cell_sort(np.concatenate([ids, h]), np.concatenate([pos, p]), rows,
                                  [4, 4, 4], ol)
    ghost, ext, _, _ = R.ghost_grid([4, 4, 4], ol)
    assert len(offs) == int(np.prod(ext)) + 1 and offs[-1] == 8 * rows == len(srt)


def test_non_periodic_shifts_nothing():
    topo, size = [3, 2, 1], 6
    ol = _ol(topo, 0.2)

    def fn(comm, r):
        R = MPIGridRedistributor(comm, topo, [1.0] * 3)
        ids, pos = _local_rows(topo, r, ROWS, np.float64)
        a = R.exchange_overload_by_position(ids, pos, ol, return_positions=True, periodic=False)
        b = R.exchange_overload_by_position(ids, pos, ol, return_positions=True, periodic=False,
                                            unwrap=True)
        torch.cuda.synchronize()
        return a, b

    total = 0
    for (h0, p0), (h1, p1) in run_ranks(size, fn):
        assert h0.tobytes() == h1.tobytes() and p0.tobytes() == p1.tobytes()
        total += len(h0)
    assert total > 0


def test_unwrap_arguments():
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    ids, pos = _local_rows([1, 1, 1], 0, 100, np.float64)
    with pytest.raises(ValueError, match="return_positions"):
        R.exchange_overload_by_position(ids, pos, [0.1] * 3, unwrap=True)
    for bad in (pos.astype(np.float16), (pos * 100).astype(np.int32), pos > 0.5):
        with pytest.raises(TypeError, match="float32 or float64"):
            R.exchange_overload_by_position(ids, bad, [0.1] * 3, return_positions=True,
                                            unwrap=True)
    with pytest.raises(ValueError, match="1024"):
        R.ghost_cell_sort(ids, pos, 100, [8, 8, 8], [0.3] * 3)
    with pytest.raises(ValueError, match="n_local"):
        R.ghost_cell_sort(ids, pos, 101, [4, 4, 4], [0.1] * 3)
    with pytest.raises(TypeError, match="float32 or float64"):
        R.ghost_cell_sort(ids, pos.astype(np.float16), 100, [4, 4, 4], [0.1] * 3)
    # a halo row beyond the ghost layers (or NaN): host results raise, device offsets read -1
    for x in (1.3, np.nan):
        far = np.concatenate([pos, [[0.5, x, 0.5]]])
        with pytest.raises(mgr._lib.MgrError, match="beyond the ghost layers"):
            R.ghost_cell_sort(np.arange(101), far, 100, [4, 4, 4], [0.1] * 3)
        _, doffs = R.ghost_cell_sort(torch.arange(101).cuda(), torch.from_numpy(far).cuda(), 100,
                                     [4, 4, 4], [0.1] * 3)
        assert (torch.diff(doffs) == -1).all()
    # the same row as an owned one is clamped into the cell, silently
    _, offs = R.ghost_cell_sort(np.arange(101), far, 101, [4, 4, 4], [0.1] * 3)
    assert offs[-1] == 101
    # SoA payload, GPU tensors: containers as fine_cell_sort's
    h, p = R.exchange_overload_by_position(ids, pos, [0.1] * 3, return_positions=True,
                                           unwrap=True)
    both, bpos = np.concatenate([ids, h]), np.concatenate([pos, p])
    ref, roffs = R.ghost_cell_sort(both, bpos, 100, [4, 4, 4], [0.1] * 3)
    (a, b), offs = R.ghost_cell_sort((torch.from_numpy(both).cuda(), torch.from_numpy(bpos).cuda()),
                                     torch.from_numpy(bpos).cuda(), 100, [4, 4, 4], [0.1] * 3)
    assert a.is_cuda and offs.is_cuda and np.array_equal(a.cpu().numpy(), ref)
    assert np.array_equal(offs.cpu().numpy(), roffs)


ONE_CALL = [("one_3d", "gt_half", np.float32), ("one_3d", "lt_half", np.float64),
            ("t_211", "gt_half", np.float64), ("t_222", "lt_half", np.float32),
            ("t_122", "gt_half", np.float64)]


@pytest.mark.parametrize("name,frac,dt", ONE_CALL)
def test_one_call_equals_composed(name, frac, dt):
    """redistribute_by_position(overload_lengths=, fine_cells=) is the composed
    form: redistribute, halo with unwrap, ghost_cell_sort."""
    topo = LAYOUTS[name]
    size = int(np.prod(topo))
    ol = _ol(topo, FRACS[frac])
    fine = [FINE] * len(topo)

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, [1.0] * len(topo))
        pos = np.random.default_rng(40 + r).uniform(-0.2, 1.2, (ROWS, len(topo))).astype(dt)
        ids = np.arange(ROWS, dtype=np.int64) + M * r
        one = R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, fine_cells=fine,
                                         return_positions=True)
        short = R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, fine_cells=fine)
        lids, lpos = R.redistribute_by_position(ids, pos.copy(), return_positions=True)
        h, p = R.exchange_overload_by_position(lids, lpos, ol, return_positions=True, unwrap=True)
        comp = R.ghost_cell_sort(np.concatenate([lids, h]), np.concatenate([lpos, p]), len(lids),
                                 fine, ol, return_positions=True)
        with pytest.raises(NotImplementedError):
            R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, fine_cells=fine,
                                       return_route=True)
        with pytest.raises(ValueError):
            R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, fine_cells=fine,
                                       reduce_route=True)
        torch.cuda.synchronize()
        return one, short, comp, len(lids)

    for one, short, comp, nl in run_ranks(size, fn):
        assert len(one) == 3 and len(short) == 2
        for a, b in zip(one, comp):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert short[0].tobytes() == one[0].tobytes() and np.array_equal(short[1], one[2])
        assert one[2][-1] == len(one[0]) > nl > 0
