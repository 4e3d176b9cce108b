"""The return path end to end on the GPU, ranks as threads: redistribute
with ``return_route=True``, compute per-row values at the destination, bring
them back with ``return_to_source``.  The map is a bijection that the ids pin,
so every source rank must get exactly the same functions of its OWN ids, in
its original row order -- no oracle needed.  Byte-exact."""
import numpy as np
import pytest
import torch

from tests import golden_io as G
from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

from mpi_grid_redistribute_amd import MPIGridRedistributor, Route  # noqa: E402

SIZE, TOPO, BOX = 4, [2, 2, 1], [1.0, 1.0, 1.0]
SIZES = [20_000, 0, 3_000, 45_000]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(rank, n, seed=71):
    rng = np.random.default_rng(seed + rank)
    pos = rng.uniform(-0.5, 1.5, (n, 3))
    ids = np.arange(n, dtype=np.int64) + 1_000_000 * rank
    return pos, ids


def _values(ids):
    """Three per-row results of different dtypes and shapes, functions of ids."""
    v1 = ids * 3 + 1
    v2 = np.stack([ids % 1000, ids % 77, -(ids % 13)], axis=1).astype(np.float32)
    v3 = (ids & 255).astype(np.uint8)
    return v1, v2, v3


def _wrapped(pos):
    return ((pos % 1.0) + 1.0) % 1.0


def _as(x, use_torch):
    return torch.from_numpy(x).cuda() if use_torch else x


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _rank_round_trip(comm, r, use_torch, chunks, sizes=SIZES, topo=TOPO):
    R = MPIGridRedistributor(comm, topo, BOX)
    R.exchange_chunks = chunks
    pos, ids = _inputs(r, sizes[r])
    p_in, i_in = _as(pos.copy(), use_torch), _as(ids.copy(), use_torch)
    (lpos, lids), route = R.redistribute_by_position((p_in, i_in), p_in, return_route=True)
    fwd = R.last_traffic
    assert isinstance(route, Route)
    assert route.n_source == sizes[r] and route.n_local == len(lids)
    sc, rc = R.last_counts
    assert np.array_equal(route.send_counts, sc) and np.array_equal(route.recv_counts, rc)
    vals = _values(_np(lids))
    back = R.return_to_source(tuple(_as(v, use_torch) for v in vals), route)
    bwd = R.last_traffic
    assert isinstance(back, tuple) and len(back) == 3
    for b, w in zip(back, _values(ids)):
        assert isinstance(b, torch.Tensor if use_torch else np.ndarray)
        if use_torch:
            assert b.is_cuda
        b = _np(b)
        assert b.dtype == w.dtype and b.shape == w.shape
        assert G.same_bytes(b, w), r
    # the received positions come back as the source's wrapped positions
    bpos = _np(R.return_to_source(lpos, route))            # a single array, the route reused
    assert G.same_bytes(bpos, _wrapped(pos)), r
    assert G.same_bytes(_np(p_in), _wrapped(pos)), r       # (the forward call wrapped them in place)
    return fwd, bwd, chunks


def _check_traffic(fwd, bwd, chunks, size):
    """The return's traffic is the forward call's with the directions swapped,
    minus the count messages, at the values' row bytes (8 + 12 + 1 against the
    forward 24 + 8)."""
    k = 1 if (chunks == 1 or size == 1) else 1 + chunks     # int64 words of a count message
    for p in range(size):
        fs, fr = fwd["send_per_peer"][p], fwd["recv_per_peer"][p]
        if fs == 0 and fr == 0:          # this rank itself
            assert bwd["send_per_peer"][p] == 0 and bwd["recv_per_peer"][p] == 0
            continue
        assert (fs - 8 * k) % 32 == 0 and (fr - 8 * k) % 32 == 0
        assert bwd["recv_per_peer"][p] == (fs - 8 * k) // 32 * 21
        assert bwd["send_per_peer"][p] == (fr - 8 * k) // 32 * 21


@pytest.mark.parametrize("use_torch", [False, True])
@pytest.mark.parametrize("chunks", [1, 4])
def test_round_trip_threads(use_torch, chunks):
    res = run_ranks(SIZE, lambda comm, r: _rank_round_trip(comm, r, use_torch, chunks))
    for fwd, bwd, k in res:
        _check_traffic(fwd, bwd, k, SIZE)


def test_round_trip_single_rank():
    fwd, bwd, _ = _rank_round_trip(None, 0, True, None, sizes=[30_000], topo=[1, 1, 1])
    assert bwd["send_bytes"] == 0 and bwd["recv_bytes"] == 0
    _rank_round_trip(None, 0, False, None, sizes=[0], topo=[1, 1, 1])


def test_cell_number_route_with_drops():
    """redistribute_by_cell_number with out-of-range ids: the dropped rows come
    back zero, every other row gets its own value."""
    def fn(comm, r):
        R = MPIGridRedistributor(comm, TOPO, BOX)
        n = SIZES[r]
        rng = np.random.default_rng(500 + r)
        ids = np.arange(n, dtype=np.int64) + 1_000_000 * r
        to = rng.integers(-1, SIZE + 1, n)                  # -1 and SIZE are dropped
        (lids, ltag), route = R.redistribute_by_cell_number((ids, to.astype(np.int16)), to,
                                                            return_route=True)
        assert (ltag == r).all()
        assert route.n_source == n and route.n_local == len(lids)
        v1, v2, _ = _values(lids)
        b1, b2 = R.return_to_source([v1, v2], route)
        kept = (to >= 0) & (to < SIZE)
        w1, w2, _ = _values(ids)
        w1[~kept] = 0
        w2[~kept] = 0
        assert n == 0 or (~kept).any()
        assert G.same_bytes(b1, w1) and G.same_bytes(b2, w2), r
        return True

    assert all(run_ranks(SIZE, fn))


def test_route_survives_later_calls_and_reuse():
    """A second forward call of another size between making and using a route
    must not disturb it (the route took its buffers out of the scratch); a
    route may be used any number of times; release() ends it."""
    def fn(comm, r):
        R = MPIGridRedistributor(comm, TOPO, BOX)
        pos, ids = _inputs(r, SIZES[r])
        lids, route = R.redistribute_by_position(ids, pos.copy(), return_route=True)
        # another redistribution, larger, on the same redistributor and stream
        pos2, ids2 = _inputs(r, 2 * SIZES[r] + 777, seed=900)
        lids2, route2 = R.redistribute_by_position(ids2, pos2.copy(), return_route=True)
        R.redistribute_by_position(ids2[:100], pos2[:100].copy())       # and one without a route
        for _ in range(2):
            assert G.same_bytes(R.return_to_source(lids * 3 + 1, route), ids * 3 + 1), r
        assert G.same_bytes(R.return_to_source(lids2, route2), ids2), r
        assert G.same_bytes(R.return_to_source(lids * 5, route), ids * 5), r
        route.release()
        return R, route, route2, lids2

    res = run_ranks(SIZE, fn)
    R, route, route2, lids2 = res[0]
    with pytest.raises(ValueError, match="released"):
        R.return_to_source(np.zeros(route.n_local), route)


def test_errors():
    def fn(comm, r):
        R = MPIGridRedistributor(comm, [2, 1, 1], BOX)
        pos, ids = _inputs(r, 1000)
        lids, route = R.redistribute_by_position(ids, pos.copy(), return_route=True)
        return R, route, lids

    (R0, route0, lids0), (R1, route1, lids1) = run_ranks(2, fn)
    with pytest.raises(ValueError, match="rows"):
        R0.return_to_source(np.zeros(route0.n_local + 1), route0)
    with pytest.raises(ValueError, match="rows"):
        R0.return_to_source((lids0, lids0[:-1]), route0)
    with pytest.raises(ValueError, match="another redistributor"):
        R0.return_to_source(lids1, route1)                  # another rank's route
    other = MPIGridRedistributor(None, [1, 1, 1], BOX)
    with pytest.raises(ValueError, match="another redistributor"):
        other.return_to_source(lids0, route0)               # another size and plan
    with pytest.raises(TypeError):
        R0.return_to_source(lids0, None)
    pos, ids = _inputs(0, 100)
    with pytest.raises(NotImplementedError, match="overload_lengths"):
        other.redistribute_by_position(ids, pos, overload_lengths=[0.1] * 3, return_route=True)
    with pytest.raises(NotImplementedError, match="fine_cells"):
        other.redistribute_by_position(ids, pos, fine_cells=[4, 4, 4], return_route=True)
    with pytest.raises(ValueError):
        other.return_to_source((), route0)
