"""The way back through the fine-cell sort on the GPU: the kernel
(mgr_unpack_ranked_fields after mgr_rank_ids + mgr_scan + mgr_pack_ranked), the
Python layer (``fine_cell_sort(..., return_route=True)`` + ``unsort``) and the
whole return path (``return_to_source(..., sort_route=)``), ranks as threads.
The reference everywhere is numpy: ``perm = np.argsort(ids, kind="stable")``,
the expected unsort of ``values`` is ``values[inv(perm)]``; byte-exact."""
import numpy as np
import pytest
import torch

from oracle import redist_oracle as ro
from tests import golden_io as G
from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

from mpi_grid_redistribute_amd import MPIGridRedistributor, Route, SortRoute, _lib  # noqa: E402
from mpi_grid_redistribute_amd.redistributor import _i64s, _ptrs  # noqa: E402

ROWS = [1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 17, 9 * 4096 + 5]
NBINS = [1, 2, 27, 64, 512, 1000, 1024]
DISTS = ["uniform", "one", "ends", "saw"]
VAL_RB = [1, 2, 3, 4, 8, 12, 16, 24, 36, 40, 100, 300]
FILL, GUARD = 0xCD, 64


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ids(dist, n, nbins, rng):
    if dist == "uniform":
        return rng.integers(0, nbins, n).astype(np.uint16)
    if dist == "one":        # every row in one cell: ranks reach tile_rows - 1
        return np.full(n, nbins // 2, dtype=np.uint16)
    if dist == "ends":       # only the first and the last cell
        return (rng.integers(0, 2, n) * (nbins - 1)).astype(np.uint16)
    return (np.arange(n) % nbins).astype(np.uint16)


def _inv(perm):
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def _vals(perm, rb, f):
    """n rows of rb bytes in sorted order, functions of the sorted row indices."""
    j = np.arange(rb, dtype=np.int64)
    return ((perm[:, None] * (2 * j + 3) + 11 * f + j) & 255).astype(np.uint8)


def _dev(a, shift=0):
    """The bytes of ``a`` on the device, ``shift`` bytes past an aligned address."""
    flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = torch.empty(flat.size + shift + 16, dtype=torch.uint8, device="cuda")
    v = buf[shift: shift + flat.size]
    v.copy_(torch.from_numpy(flat))
    return v


class Out:
    """An output of n rows of rb bytes between two guard zones, all FILL."""

    def __init__(self, n, rb, shift=0):
        self.nbytes = n * rb
        self.buf = torch.full((GUARD + shift + self.nbytes + GUARD,), FILL, dtype=torch.uint8,
                              device="cuda")
        self.view = self.buf[GUARD + shift: GUARD + shift + self.nbytes]
        self.shift, self.rb = shift, rb

    def get(self):
        h = self.buf.cpu().numpy()
        a = GUARD + self.shift
        assert (h[:a] == FILL).all() and (h[a + self.nbytes:] == FILL).all(), "wrote out of bounds"
        return h[a: a + self.nbytes].reshape(-1, self.rb)


class Forward:
    """mgr_rank_ids + mgr_scan + mgr_pack_ranked of an int64 row-index field (and
    of ``extra`` more fields of these row bytes) by ``ids``; tile_rows =
    mgr_ranked_tile_rows(the widest field packed, nbins)."""

    def __init__(self, ids, nbins, extra=()):
        lib = _lib.load()
        self.n = n = len(ids)
        self.nbins = nbins
        self.tile_rows = tr = int(lib.mgr_ranked_tile_rows(max((8,) + tuple(extra)), nbins))
        assert tr in (2048, 4096)
        s = _lib.stream_handle()
        T = (n + tr - 1) // tr
        self.ids = torch.from_numpy(ids.view(np.int16)).cuda()
        self.ws = torch.empty(int(lib.mgr_workspace_bytes(n, nbins, tr)), dtype=torch.uint8,
                              device="cuda")
        self.ranks = torch.empty(2 * n + 16, dtype=torch.uint8, device="cuda")
        self.tstarts = torch.empty(8 * max(T * nbins, 1), dtype=torch.uint8, device="cuda")
        self.counts = torch.empty(nbins, dtype=torch.int64, device="cuda")
        _lib.call("mgr_rank_ids", _lib.ptr(self.ids), n, nbins, tr, _lib.ptr(self.ranks),
                  _lib.ptr(self.tstarts), None, _lib.ptr(self.ws), s)
        _lib.call("mgr_scan", n, nbins, tr, _lib.ptr(self.ws), _lib.ptr(self.counts), s)
        self.perm = np.argsort(np.minimum(ids, nbins - 1), kind="stable")

    def pack(self, src_np, rb):
        src = _dev(src_np)
        out = torch.empty(self.n * rb, dtype=torch.uint8, device="cuda")
        _lib.call("mgr_pack_ranked", _lib.ptr(src), rb, self.n, _lib.ptr(self.ids),
                  _lib.ptr(self.ranks), _lib.ptr(self.tstarts), self.nbins, self.tile_rows,
                  _lib.ptr(self.ws), _lib.ptr(out), _lib.stream_handle())
        return out.cpu().numpy()

    def check_forward(self):
        """The sort itself: the index field comes out as numpy's stable argsort."""
        got = self.pack(np.arange(self.n, dtype=np.int64), 8).view(np.int64)
        assert np.array_equal(got, self.perm)

    def unpack(self, srcs, rbs, outs):
        _lib.call("mgr_unpack_ranked_fields", len(rbs), _ptrs([t.data_ptr() for t in srcs]),
                  _i64s(rbs), self.n, _lib.ptr(self.ids), _lib.ptr(self.ranks),
                  _lib.ptr(self.tstarts), self.nbins, self.tile_rows, _lib.ptr(self.ws),
                  _ptrs([o.view.data_ptr() for o in outs]), _lib.stream_handle())


def _check_fields(fw, rbs, shifts=None, one_per_call=True):
    """All fields in one call, then one per call: both equal numpy."""
    n = fw.n
    shifts = shifts or [0] * len(rbs)
    inv = _inv(fw.perm)
    vals = [_vals(fw.perm, rb, f) for f, rb in enumerate(rbs)]
    srcs = [_dev(v, sh) for v, sh in zip(vals, shifts)]
    outs = [Out(n, rb, sh) for rb, sh in zip(rbs, shifts)]
    fw.unpack(srcs, rbs, outs)
    got = [o.get() for o in outs]
    for f, rb in enumerate(rbs):
        assert np.array_equal(got[f], vals[f][inv]), (f, rb, "one launch")
    if one_per_call:
        for f, rb in enumerate(rbs):
            one = Out(n, rb, shifts[f])
            fw.unpack([srcs[f]], [rb], [one])
            assert np.array_equal(one.get(), got[f]), (f, rb, "one per call")


@pytest.mark.parametrize("mode", ["auto", "hook2048", "field64"])
@pytest.mark.parametrize("n", ROWS)
def test_kernel_row_counts_bins_and_widths(n, mode):
    """Every row count with every id distribution, over all bin counts, on both
    tile sizes (2048 by the hook rank_rows and by a 64-byte field in the forward
    set); the twelve value widths in one launch and one per call."""
    i = ROWS.index(n) + ["auto", "hook2048", "field64"].index(mode)
    rng = np.random.default_rng(1000 + 7 * i)
    if mode == "hook2048":
        _lib.test_hook("rank_rows", 2048)
    try:
        for d, dist in enumerate(DISTS):
            nbins = NBINS[(i + 2 * d) % len(NBINS)]
            fw = Forward(_ids(dist, n, nbins, rng), nbins, extra=(64,) if mode == "field64" else ())
            assert fw.tile_rows == (4096 if mode == "auto" else 2048)
            fw.check_forward()
            if mode == "field64":
                wide = rng.integers(0, 256, (n, 64), dtype=np.uint8)
                assert np.array_equal(fw.pack(wide, 64).reshape(n, 64), wide[fw.perm])
            _check_fields(fw, VAL_RB)
    finally:
        _lib.test_hook("rank_rows", _lib.HOOK_DEFAULTS["rank_rows"])


@pytest.mark.parametrize("nbins", NBINS)
def test_kernel_every_bin_count_full_tiles(nbins):
    """Every bin count with every distribution at more than 8 tiles (the XCD
    dealing wraps) and in one cell (ranks up to tile_rows - 1)."""
    n = ROWS[-1]
    rng = np.random.default_rng(nbins)
    for dist in DISTS:
        fw = Forward(_ids(dist, n, nbins, rng), nbins)
        fw.check_forward()
        _check_fields(fw, [12, 12, 4, 8])
        _check_fields(fw, [3, 300, 16], one_per_call=False)


@pytest.mark.parametrize("unpack_kernel", [0, 1])
def test_kernel_field_sets(unpack_kernel):
    """16 fields in one launch and config 5's four (12, 12, 4, 8) equal the
    same fields one per call; one field 4-byte but not 16-byte aligned.  Hook
    unpack_kernel 1: the run-time field table also for templated signatures."""
    n, nbins = 3 * 4096 + 17, 512
    rng = np.random.default_rng(5)
    fw = Forward(_ids("uniform", n, nbins, rng), nbins)
    fw.check_forward()
    _lib.test_hook("unpack_kernel", unpack_kernel)
    try:
        _check_fields(fw, [12, 12, 4, 8])
        _check_fields(fw, [12, 12, 4, 8], shifts=[4, 0, 0, 8])
        _check_fields(fw, VAL_RB + [16, 12, 8, 6], shifts=[0] * 12 + [4, 4, 0, 2])
        _check_fields(fw, [16], shifts=[4])
    finally:
        _lib.test_hook("unpack_kernel", 0)


def test_kernel_clamps_ids_like_the_pack():
    """ids >= nbins are clamped to nbins - 1 by the rank, the pack and the
    unpack alike: the unpack still inverts what the pack did."""
    n, nbins = 2 * 4096 + 100, 27
    rng = np.random.default_rng(6)
    ids = rng.integers(0, nbins + 9, n).astype(np.uint16)
    ids[::97] = 65535
    fw = Forward(ids, nbins)
    fw.check_forward()
    _check_fields(fw, [8, 12, 3])


def test_failed_scan_writes_nothing():
    """After a failed scan (hook scan_poison_chunk) nothing is written: the
    outputs keep their fill, from both the templated and the run-time kernel."""
    n, nbins = 300_000, 512
    rng = np.random.default_rng(8)
    _lib.test_hook("scan_poison_chunk", 0)
    try:
        fw = Forward(_ids("uniform", n, nbins, rng), nbins)
        counts = fw.counts.cpu().numpy()
        for hook, rbs in ((0, [12, 12, 4, 8]), (1, [12, 12, 4, 8]), (0, [3, 300])):
            _lib.test_hook("unpack_kernel", hook)
            srcs = [_dev(np.zeros((n, rb), np.uint8)) for rb in rbs]
            outs = [Out(n, rb) for rb in rbs]
            for o in outs:
                o.buf.fill_(0xAB)
            fw.unpack(srcs, rbs, outs)
            torch.cuda.synchronize()
            for o in outs:
                assert bool((o.buf == 0xAB).all()), "an unpack wrote after a failed scan"
    finally:
        _lib.test_hook("scan_poison_chunk", _lib.HOOK_DEFAULTS["scan_poison_chunk"])
        _lib.test_hook("unpack_kernel", 0)
    assert (counts == -1).all(), counts


# ------------------------------------------------------------------ Python
TOPO1, BOX = [1, 1, 1], [1.0, 1.0, 1.0]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _as(x, use_torch):
    return torch.from_numpy(x).cuda() if use_torch else x


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (n, 3))
    idx = np.arange(n, dtype=np.int64)
    return pos, idx


def _values(key):
    """Three per-row results of different dtypes and shapes, functions of key."""
    v1 = key * 3 + 1
    v2 = np.stack([key % 1000, key % 77, -(key % 13)], axis=1).astype(np.float32)
    v3 = (key & 255).astype(np.uint8)
    return v1, v2, v3


@pytest.mark.parametrize("fine", [[8, 8, 8], [3, 1, 5], [16, 16, 8]])
@pytest.mark.parametrize("use_torch", [False, True])
def test_fine_cell_sort_route_and_unsort(fine, use_torch):
    """numpy and GPU torch, one array and a tuple, with return_positions; the
    2048 cells of [16, 16, 8] take the non-ranked sort."""
    n = 30_011
    pos, idx = _rows(n, 3)
    perm = np.argsort(ro.fine_cell_ids(TOPO1, fine, BOX, pos), kind="stable")
    inv = _inv(perm)
    R = MPIGridRedistributor(None, TOPO1, BOX)
    p_in, i_in = _as(pos.copy(), use_torch), _as(idx.copy(), use_torch)
    plain = R.fine_cell_sort(i_in, p_in, fine)
    assert len(plain) == 2                               # without return_route: today's tuple
    res = R.fine_cell_sort(i_in, p_in, fine, return_route=True)
    assert len(res) == 3 and isinstance(res[2], SortRoute)
    srt, off, sroute = res
    assert G.same_bytes(_np(srt), perm) and G.same_bytes(_np(srt), _np(plain[0]))
    assert G.same_bytes(_np(off), _np(plain[1]))
    assert sroute.n == n and sroute.nbins == int(np.prod(fine)) and not sroute.released
    assert sroute.ranked == (int(np.prod(fine)) <= 1024)
    back = R.unsort(srt, sroute)                         # one array
    assert isinstance(back, torch.Tensor if use_torch else np.ndarray)
    assert G.same_bytes(_np(back), idx)
    vals = _values(perm)
    got = R.unsort(tuple(_as(v, use_torch) for v in vals), sroute)      # a tuple, the route reused
    assert isinstance(got, tuple) and len(got) == 3
    for g, v in zip(got, vals):
        if use_torch:
            assert g.is_cuda
        assert G.same_bytes(_np(g), v[inv])
    # a tuple payload with return_positions: (data, positions, offsets, route)
    (s_idx, s_pos32), s_pos, off2, sroute2 = R.fine_cell_sort(
        (i_in, _as(pos.astype(np.float32), use_torch)), p_in, fine, return_positions=True,
        return_route=True)
    assert G.same_bytes(_np(s_pos), pos[perm]) and G.same_bytes(_np(s_idx), perm)
    assert G.same_bytes(_np(R.unsort(s_pos, sroute2)), pos)
    assert G.same_bytes(_np(R.unsort([s_pos32], sroute2)[0]), pos.astype(np.float32))
    assert G.same_bytes(_np(R.unsort(s_pos, sroute)), pos)              # the first route still serves


@pytest.mark.parametrize("device_ids", [False, True])
def test_fine_ids_given_and_alias_copy(device_ids):
    """fine_ids given; a caller's device tensor is overwritten before unsort
    (the route keeps its own copy)."""
    n, fine = 20_003, [8, 8, 8]
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 512, n).astype(np.uint16)
    perm = np.argsort(ids, kind="stable")
    pos, idx = _rows(n, 5)
    R = MPIGridRedistributor(None, TOPO1, BOX)
    given = torch.from_numpy(ids.view(np.int16)).cuda() if device_ids else ids
    srt, off, sroute = R.fine_cell_sort(torch.from_numpy(idx).cuda(), torch.from_numpy(pos).cuda(),
                                        fine, fine_ids=given, return_route=True)
    assert G.same_bytes(_np(srt), perm)
    if device_ids:
        given.fill_(7)
        torch.cuda.synchronize()
    v = _values(perm)[1]
    assert G.same_bytes(_np(R.unsort(torch.from_numpy(v).cuda(), sroute)), v[_inv(perm)])


def test_six_byte_field_takes_the_non_ranked_path():
    n, fine = 10_007, [8, 8, 8]
    pos, idx = _rows(n, 6)
    perm = np.argsort(ro.fine_cell_ids(TOPO1, fine, BOX, pos), kind="stable")
    six = np.stack([idx % 251, idx % 13, idx % 7], axis=1).astype(np.uint16)     # 6-byte rows
    R = MPIGridRedistributor(None, TOPO1, BOX)
    srt, off, sroute = R.fine_cell_sort(six, pos, fine, return_route=True)
    assert G.same_bytes(srt, six[perm]) and not sroute.ranked
    assert G.same_bytes(R.unsort(srt, sroute), six)
    assert G.same_bytes(R.unsort(perm, sroute), idx)


def test_empty_and_live_routes_and_errors():
    fine = [8, 8, 8]
    R = MPIGridRedistributor(None, TOPO1, BOX)
    # n = 0
    e_srt, e_off, e_route = R.fine_cell_sort(np.zeros(0, np.int64), np.zeros((0, 3)), fine,
                                             return_route=True)
    assert e_route.n == 0 and len(e_srt) == 0
    e_back = R.unsort((np.zeros((0, 3), np.float32), np.zeros(0, np.int64)), e_route)
    assert e_back[0].shape == (0, 3) and e_back[1].shape == (0,)
    # later sorts on the same redistributor do not disturb a live route
    pos, idx = _rows(25_000, 7)
    srt, off, sroute = R.fine_cell_sort(idx, pos, fine, return_route=True)
    pos2, idx2 = _rows(61_000, 8)
    srt2, off2, sroute2 = R.fine_cell_sort(idx2, pos2, fine, return_route=True)
    R.fine_cell_sort(idx2[:500], pos2[:500], fine)
    R.fine_cell_sort(idx2, pos2, [3, 1, 5], return_route=True)
    for _ in range(2):                                       # the route can be used twice
        assert G.same_bytes(R.unsort(srt * 5, sroute), idx * 5)
    assert G.same_bytes(R.unsort(srt2, sroute2), idx2)
    # errors
    with pytest.raises(ValueError, match="rows"):
        R.unsort(np.zeros(sroute.n + 1), sroute)
    with pytest.raises(ValueError, match="rows"):
        R.unsort((srt, srt[:-1]), sroute)
    with pytest.raises(TypeError):
        R.unsort(srt, None)
    lids, route = R.redistribute_by_position(idx, pos.copy(), return_route=True)
    with pytest.raises(TypeError):
        R.unsort(srt, route)                                 # a Route is not a SortRoute
    with pytest.raises(TypeError):
        R.return_to_source(lids, route, sort_route=route)
    with pytest.raises(ValueError, match="rows"):
        R.return_to_source(np.zeros(route.n_local), route, sort_route=sroute2)
    sroute.release()
    assert sroute.released
    with pytest.raises(ValueError, match="released"):
        R.unsort(srt, sroute)
    with pytest.raises(ValueError, match="released"):
        R.return_to_source(lids, route, sort_route=sroute)
    with pytest.raises(NotImplementedError, match="fine_cells"):
        R.redistribute_by_position(idx, pos.copy(), fine_cells=fine, return_route=True)


# -------------------------------------------------- end to end, ranks as threads
SIZE, TOPO = 4, [2, 2, 1]
SIZES = [20_000, 0, 3_000, 45_000]


def _rank_recipe(comm, r, chunks, use_torch):
    R = MPIGridRedistributor(comm, TOPO, BOX)
    R.exchange_chunks = chunks
    n = SIZES[r]
    rng = np.random.default_rng(71 + r)
    pos = rng.uniform(-0.5, 1.5, (n, 3))
    ids = np.arange(n, dtype=np.int64) + 1_000_000 * r
    fine = [8, 8, 8]
    p_in = _as(pos.copy(), use_torch)
    (lids, lpos), route = R.redistribute_by_position(_as(ids.copy(), use_torch), p_in,
                                                     return_positions=True, return_route=True)
    assert isinstance(route, Route)
    (sids, spos), offsets, sroute = R.fine_cell_sort((lids, lpos), lpos, fine, return_route=True)
    assert isinstance(sroute, SortRoute) and sroute.n == route.n_local
    # sorted: the fine cells of the sorted positions ascend
    cells = ro.fine_cell_ids(TOPO, fine, BOX, _np(spos))
    assert (np.diff(cells) >= 0).all()
    vals = _values(_np(sids))                               # computed in sorted order
    back = R.return_to_source(tuple(_as(v, use_torch) for v in vals), route, sort_route=sroute)
    assert isinstance(back, tuple) and len(back) == 3
    for b, w in zip(back, _values(ids)):
        assert isinstance(b, torch.Tensor if use_torch else np.ndarray)
        assert G.same_bytes(_np(b), w), r
    wrapped = ((pos % 1.0) + 1.0) % 1.0
    bpos = R.return_to_source(spos, route, sort_route=sroute)           # one array, routes reused
    assert G.same_bytes(_np(bpos), wrapped), r
    # and the same along the two separate steps
    two = R.return_to_source(R.unsort(spos, sroute), route)
    assert G.same_bytes(_np(two), wrapped), r
    return True


@pytest.mark.parametrize("chunks", [1, 4])
def test_recipe_threads(chunks):
    assert all(run_ranks(SIZE, lambda comm, r: _rank_recipe(comm, r, chunks, chunks == 4)))
