"""The halo's return path (reduce_overload, HaloRoute), pinned by global row
ids and independent of the exchange's structure.

Every row carries a unique int64 id (rank * M + row).  After the halo exchange
every rank gives its overload row j a value of small integers that depend on
(rank, j) -- exactly representable, so every add order gives the same bits.
The expectation for the owned row with id g is ``np.add.at`` over all ranks'
overload rows with that id, plus the local value; compared byte for byte for
float32 / float64 / int32 / int64, ncomp 1 and 3, numpy and torch.  Each layout
asserts that some owner received several contributions (a copy of a copy: the
nested path), so a chain that never forwards would not pass unnoticed.
"""
import numpy as np
import pytest
import torch

from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import HaloRoute, MPIGridRedistributor  # noqa: E402

BOX = [1.0, 1.0, 1.0]
M = 1_000_000
ROWS = 10_000          # per rank: the 4096-row selection tiles are crossed
DTYPES = [np.float32, np.float64, np.int32, np.int64]

# (topology, ranks, periodic, rank left empty, least contributions some owner must get)
LAYOUTS = {
    "self_111": ([1, 1, 1], 1, True, None, 3),
    "twice_211": ([2, 1, 1], 2, True, None, 3),          # a == b: a row arrives twice
    "selfdim_121": ([1, 2, 1], 2, True, None, 3),        # a self dimension inside the general path
    "p4_221": ([2, 2, 1], 4, True, None, 3),
    "p8_222": ([2, 2, 2], 8, True, None, 3),
    "p6_321_nonperiodic": ([3, 2, 1], 6, False, None, 2),   # x and y only: 2-D
    "empty_rank_221": ([2, 2, 1], 4, True, 2, 3),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _local_rows(topo, r, rows, seed):
    """rows rows inside rank r's cell (already redistributed), ids r * M + i."""
    rng = np.random.default_rng(seed + r)
    idx = np.array(np.unravel_index(r, topo))
    pos = (idx + rng.random((rows, 3))) / np.asarray(topo)
    return np.arange(rows, dtype=np.int64) + M * r, pos


def _ol(topo):
    return [0.25 / t for t in topo]


def _vals(q, n, ncomp, dt, salt=0):
    """Small integers that depend on (rank, row, component)."""
    j = np.arange(n, dtype=np.int64)
    v = ((q * 7 + j * 3 + salt)[:, None] + np.arange(ncomp)) % 11 - 5
    return v.astype(dt).reshape((n, ncomp) if ncomp > 1 else (n,))


def _expected(size, n_own, hids, hvals, lvals):
    """exp[r][i] = lvals[r][i] + sum of hvals over every overload row, on any
    rank, with id r * M + i; cnt[r][i] = how many there are."""
    exp = [lv.copy() for lv in lvals]
    cnt = [np.zeros(n, dtype=np.int64) for n in n_own]
    for q in range(size):
        owner, idx = hids[q] // M, hids[q] % M
        for r in range(size):
            m = owner == r
            np.add.at(exp[r], idx[m], hvals[q][m])
            np.add.at(cnt[r], idx[m], 1)
    return exp, cnt


def _conv(as_torch):
    if as_torch:
        return lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return lambda x: x


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def _run(name, body, rows=ROWS, seed=11):
    topo, size, periodic, empty, _ = LAYOUTS[name]

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, BOX)
        ids, pos = _local_rows(topo, r, 0 if r == empty else rows, seed)
        hids, route = R.exchange_overload_by_position(ids, pos, _ol(topo), periodic=periodic,
                                                      return_route=True)
        assert isinstance(route, HaloRoute)
        assert route.n_local == len(ids) and route.n_halo == len(hids)
        out = body(R, r, ids, hids, route)
        torch.cuda.synchronize()
        return ids, hids, out

    return run_ranks(size, fn)


COMBOS = [(dt, nc, t) for dt in DTYPES for nc in (1, 3) for t in (False, True)]


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_reduce_pinned_by_ids(name):
    topo, size, _, _, least = LAYOUTS[name]

    def body(R, r, ids, hids, route):
        res = []
        for dt, nc, as_torch in COMBOS:
            c = _conv(as_torch)
            got = R.reduce_overload(c(_vals(r, len(hids), nc, dt)), route,
                                    local_values=c(_vals(r, len(ids), nc, dt, salt=1)))
            assert isinstance(got, torch.Tensor) == as_torch
            res.append(_np(got))
        # no local values: the sums alone; a route serves any number of calls
        res.append(R.reduce_overload(_vals(r, len(hids), 3, np.int64), route))
        return res

    outs = _run(name, body)
    ids = [o[0] for o in outs]
    hids = [o[1] for o in outs]
    n_own = [len(i) for i in ids]
    for r in range(size):
        assert np.array_equal(ids[r], np.arange(n_own[r]) + M * r)
    cnt = None
    for ci, (dt, nc, _) in enumerate(COMBOS):
        exp, cnt = _expected(size, n_own, hids,
                             [_vals(q, len(hids[q]), nc, dt) for q in range(size)],
                             [_vals(q, n_own[q], nc, dt, salt=1) for q in range(size)])
        for r in range(size):
            got = outs[r][2][ci]
            assert got.dtype == np.dtype(dt) and got.shape == exp[r].shape
            assert got.tobytes() == exp[r].tobytes(), (name, r, np.dtype(dt).name, nc)
    exp, _ = _expected(size, n_own, hids,
                       [_vals(q, len(hids[q]), 3, np.int64) for q in range(size)],
                       [np.zeros((n, 3), np.int64) for n in n_own])
    for r in range(size):
        assert outs[r][2][-1].tobytes() == exp[r].tobytes(), (name, r)
    # the nested path was reached: some owner got a copy of a copy back
    assert max(int(c.max()) for c in cnt if len(c)) >= least, name
    assert sum(len(h) for h in hids) > 0


def test_float_random_values_reproducible_and_bounded():
    """Random float32 values on 8 ranks: two runs are bit-identical, and the
    result is within k * eps * sum|v| of the float64 sum (k = the row's number
    of contributions: the standard bound for k sequential adds)."""
    name = "p8_222"
    size = LAYOUTS[name][1]

    def fvals(q, n, salt):
        return np.random.default_rng(100 * q + salt).uniform(-1, 1, (n, 3)).astype(np.float32)

    def body(R, r, ids, hids, route):
        v, lv = fvals(r, len(hids), 0), fvals(r, len(ids), 1)
        a = R.reduce_overload(v, route, local_values=lv)
        b = R.reduce_overload(torch.from_numpy(v).cuda(), route,
                              local_values=torch.from_numpy(lv).cuda())
        return a, _np(b)

    outs = _run(name, body)
    hids = [o[1] for o in outs]
    n_own = [len(o[0]) for o in outs]
    hv = [fvals(q, len(hids[q]), 0) for q in range(size)]
    lv = [fvals(q, n_own[q], 1) for q in range(size)]
    exact, cnt = _expected(size, n_own, hids, [v.astype(np.float64) for v in hv],
                           [v.astype(np.float64) for v in lv])
    mag, _ = _expected(size, n_own, hids, [np.abs(v).astype(np.float64) for v in hv],
                       [np.abs(v).astype(np.float64) for v in lv])
    eps = float(np.finfo(np.float32).eps)
    assert max(int(c.max()) for c in cnt) >= 3 and max(int(c.max()) for c in cnt) <= 27
    for r in range(size):
        a, b = outs[r][2]
        assert a.tobytes() == b.tobytes(), r
        err = np.abs(a.astype(np.float64) - exact[r])
        assert (err <= cnt[r][:, None] * eps * mag[r]).all(), (r, float(err.max()))


@pytest.mark.parametrize("name", ["self_111", "twice_211", "p8_222", "empty_rank_221"])
def test_all_the_way_home(name):
    """The routes compose: redistribute_by_position(return_positions,
    return_route), exchange_overload_by_position(return_route) on what arrived,
    values on owned + overload rows, reduce_overload, return_to_source --
    original row i gets its own value plus the values of all its copies,
    anywhere.  (One call with overload_lengths and return_route raises and
    names this route and reduce_route=True.)"""
    topo, size, _, empty, least = LAYOUTS[name]
    ol = _ol(topo)

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, BOX)
        n = 0 if r == empty else ROWS
        pos = np.random.default_rng(300 + r).uniform(-0.2, 1.2, (n, 3))
        ids = np.arange(n, dtype=np.int64) + M * r
        with pytest.raises(NotImplementedError, match="reduce_overload"):
            R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, return_route=True)
        (lids, lpos), route = R.redistribute_by_position(ids, pos, return_positions=True,
                                                         return_route=True)
        hids, hroute = R.exchange_overload_by_position(lids, lpos, ol, return_route=True)
        nl = len(lids)
        assert route.n_source == n and route.n_local == nl == hroute.n_local
        out = np.concatenate([lids, hids])
        v64 = _vals(r, len(out), 1, np.int64)
        v32 = _vals(r, len(out), 3, np.float32)
        b64 = R.return_to_source(R.reduce_overload(v64[nl:], hroute, local_values=v64[:nl]),
                                 route)
        t32 = torch.from_numpy(v32).cuda()
        b32 = R.return_to_source(R.reduce_overload(t32[nl:], hroute, local_values=t32[:nl]),
                                 route)
        hroute.release()
        assert hroute.released and not route.released
        with pytest.raises(ValueError, match="released"):
            R.reduce_overload(v64[nl:], hroute)
        torch.cuda.synchronize()
        return n, out, b64, _np(b32)

    _check_home(name, run_ranks(size, fn), size, least)


def _check_home(name, outs, size, least):
    """outs[r] = (source rows, ids of the rows rank r held, int64 result,
    float32 x 3 result): original row i got the values of its owner's copy and
    of every overload copy, on any rank."""
    n_src = [o[0] for o in outs]
    rows = [o[1] for o in outs]
    for nc, dt, k in ((1, np.int64, 2), (3, np.float32, 3)):
        exp, cnt = _expected(size, n_src, rows,
                             [_vals(q, len(rows[q]), nc, dt) for q in range(size)],
                             [np.zeros((n, nc) if nc > 1 else (n,), dt) for n in n_src])
        for r in range(size):
            assert outs[r][k].tobytes() == exp[r].tobytes(), (name, r, nc)
    assert min(int(c.min()) for c in cnt if len(c)) >= 1          # every row has its owner
    assert max(int(c.max()) for c in cnt if len(c)) >= least + 1


@pytest.mark.parametrize("name", ["self_111", "twice_211", "p8_222", "empty_rank_221"])
def test_one_call_form(name):
    """redistribute_by_position(..., overload_lengths=, reduce_route=True), then
    return_to_source of n_local + n_halo values: original row i gets its own
    value plus the values of all its copies, anywhere; release() frees both."""
    topo, size, _, empty, least = LAYOUTS[name]
    ol = _ol(topo)

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, BOX)
        n = 0 if r == empty else ROWS
        pos = np.random.default_rng(300 + r).uniform(-0.2, 1.2, (n, 3))
        ids = np.arange(n, dtype=np.int64) + M * r
        out, route = R.redistribute_by_position(ids, pos, overload_lengths=ol, reduce_route=True)
        assert isinstance(route.halo, HaloRoute) and route.n_source == n
        assert route.n_local + route.n_halo == len(out)
        v64 = _vals(r, len(out), 1, np.int64)
        v32 = _vals(r, len(out), 3, np.float32)
        b64 = R.return_to_source(v64, route)
        b32 = R.return_to_source(torch.from_numpy(v32).cuda(), route)
        with pytest.raises(ValueError, match="rows"):
            R.return_to_source(np.zeros(route.n_local + route.n_halo + 1), route)
        with pytest.raises(TypeError, match="float32, float64, int32 or int64"):
            R.return_to_source(v64.astype(np.int16), route)
        route.release()
        assert route.released and route.halo.released
        with pytest.raises(ValueError, match="released"):
            R.return_to_source(v64, route)
        torch.cuda.synchronize()
        return n, out, b64, _np(b32)

    _check_home(name, run_ranks(size, fn), size, least)


def test_one_call_form_arguments():
    R = MPIGridRedistributor(None, [1, 1, 1], BOX)
    ids, pos = _local_rows([1, 1, 1], 0, 100, seed=3)
    with pytest.raises(ValueError, match="reduce_route"):
        R.redistribute_by_position(ids, pos, reduce_route=True)             # no halo
    with pytest.raises(ValueError, match="reduce_route"):
        R.redistribute_by_position(ids, pos, overload_lengths=[0.1] * 3, return_route=True,
                                   reduce_route=True)
    (out, pout), route = R.redistribute_by_position(ids, pos, overload_lengths=[0.1] * 3,
                                                    return_positions=True, reduce_route=True)
    assert len(out) == len(pout) == route.n_local + route.n_halo and route.n_local == 100


def test_soa_values_and_route_reuse():
    """A tuple of three arrays of different dtypes in one call; the route
    survives a later exchange on the same redistributor and serves twice."""
    name = "p4_221"
    topo, size = LAYOUTS[name][0], LAYOUTS[name][1]
    kinds = [(np.float32, 3), (np.int64, 1), (np.float64, 2)]

    def body(R, r, ids, hids, route):
        vals = tuple(_vals(r, len(hids), nc, dt, salt=s) for s, (dt, nc) in enumerate(kinds))
        first = R.reduce_overload(vals, route)
        assert isinstance(first, tuple) and len(first) == 3
        # a later call on the same redistributor, with rows of its own
        ids2, pos2 = _local_rows(topo, r, 3000, seed=77)
        R.exchange_overload_by_position(ids2, pos2, _ol(topo))
        again = R.reduce_overload(list(vals), route)
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
        return first

    outs = _run(name, body)
    hids = [o[1] for o in outs]
    n_own = [len(o[0]) for o in outs]
    for s, (dt, nc) in enumerate(kinds):
        exp, _ = _expected(size, n_own, hids,
                           [_vals(q, len(hids[q]), nc, dt, salt=s) for q in range(size)],
                           [np.zeros((n, nc) if nc > 1 else (n,), dt) for n in n_own])
        for r in range(size):
            got = outs[r][2][s]
            assert got.dtype == np.dtype(dt) and got.tobytes() == exp[r].tobytes(), (s, r)


def test_route_validation():
    def body(R, r, ids, hids, route):
        return R, route

    outs = _run("twice_211", body, rows=2000)
    (R0, route0), (R1, route1) = outs[0][2], outs[1][2]
    nh = route0.n_halo
    with pytest.raises(ValueError, match="rows"):
        R0.reduce_overload(np.zeros(nh + 1), route0)
    with pytest.raises(ValueError, match="rows"):
        R0.reduce_overload((np.zeros(nh), np.zeros(nh - 1)), route0)
    with pytest.raises(ValueError, match="rows"):
        R0.reduce_overload(np.zeros(nh), route0, local_values=np.zeros(route0.n_local + 1))
    with pytest.raises(TypeError, match="float32, float64, int32 or int64"):
        R0.reduce_overload(np.zeros(nh, dtype=np.int16), route0)
    with pytest.raises(ValueError, match="another redistributor"):
        R0.reduce_overload(np.zeros(route1.n_halo), route1)      # another rank's route
    other = MPIGridRedistributor(None, [1, 1, 1], BOX)
    with pytest.raises(ValueError, match="another redistributor"):
        other.reduce_overload(np.zeros(nh), route0)
    with pytest.raises(TypeError):
        R0.reduce_overload(np.zeros(nh), None)
    route0.release()
    with pytest.raises(ValueError, match="released"):
        R0.reduce_overload(np.zeros(nh), route0)


def test_without_route_the_result_is_unchanged():
    """return_route=False returns what it always did; with it, the overload
    rows are the same and the route comes last (after the positions)."""
    topo = [1, 1, 1]
    ids, pos = _local_rows(topo, 0, 5000, seed=5)
    R = MPIGridRedistributor(None, topo, BOX)
    plain = R.exchange_overload_by_position(ids, pos, _ol(topo))
    h, p, route = R.exchange_overload_by_position(ids, pos, _ol(topo), return_positions=True,
                                                  return_route=True)
    assert isinstance(plain, np.ndarray) and plain.tobytes() == h.tobytes()
    assert len(p) == len(h) and isinstance(route, HaloRoute)
