"""``exchange_overload(..., return_route=True)`` and ``reduce_overload`` on the
CPU: the general (multi-rank) path forwards and backwards on threaded ranks,
the selections and the inverse selection add done by NumPy stand-ins.  The
payload is one int64 global row id per row, so the expected sums come by brute
force over every rank's overload ids: the owner's row with id g ends as its
own value plus every value on a copy of g anywhere.  Integers: compared
exactly."""
import numpy as np
import pytest

from mpi_grid_redistribute_amd import _lib
from mpi_grid_redistribute_amd.comm import MpiHostComm
from mpi_grid_redistribute_amd.halo import reduce_overload
from tests.fake_mpi import run_ranks
from tests.test_halo_cpu import CpuSelect, GeoRank, _flat
from tests.test_halo_trace_cpu import exchange, inputs

ID_BITS = 20                                              # id = rank << 20 | local row
_ELEM_NP = {_lib.MGR_ELEM_I32: np.dtype(np.int32), _lib.MGR_ELEM_I64: np.dtype(np.int64)}


class RouteSelect(CpuSelect):
    """CpuSelect with what a route needs: ``take`` and the inverse of
    msel_pack with an add (mgr_msel_unpack_add)."""

    def take(self, name):
        pass

    def msel_unpack_add(self, handle, acc_flat, elem, ncomp, srcs):
        dt = _ELEM_NP[elem]
        acc = acc_flat.numpy().view(dt).reshape(-1, ncomp)   # shares the tensor's memory
        for idx, s in zip(handle, srcs):                     # ascending k
            if s is not None and len(idx):
                rows = s.numpy()[: len(idx) * ncomp * dt.itemsize].view(dt).reshape(-1, ncomp)
                acc[idx] += rows


def _values(r, rows, elem, ncomp):
    """The value on row j of rank r: a fixed function of both."""
    j = np.arange(rows, dtype=np.int64)
    v = (r + 1) * 100003 + 17 * j + 1
    return np.stack([v * (c + 1) * (-1) ** c for c in range(ncomp)], axis=1).astype(_ELEM_NP[elem])


@pytest.mark.parametrize("spare", [None, 10**6, "outgrown"])
@pytest.mark.parametrize("nfields", [1, 2])
@pytest.mark.parametrize("case", ["halo_p8_f64_rec32.npz", "halo_p6_321_i32.npz",
                                  "halo_direct_p6_321_nonperiodic.npz"])
def test_route_and_reduce(case, nfields, spare):
    """``outgrown``: an arena one row short of the rank's halo, so the store
    moves in the last dimension that appends rows and copies the earlier
    dimensions' rows (every rank of the periodic layouts receives rows in all
    three dimensions; of the non-periodic one ranks 1, 3 and 5 in two, the
    others in dimension 0 only, where the move has nothing to copy)."""
    f, per_rank, periodic = inputs(case)
    size = int(f["size"])
    kinds = [(_lib.MGR_ELEM_I64, 1), (_lib.MGR_ELEM_I32, 2)][:nfields]
    halo_rows = None
    if spare == "outgrown":
        halo_rows = run_ranks(size, lambda comm, r: exchange(
            f, r, MpiHostComm(comm), CpuSelect(), np.zeros(len(per_rank[r][1]), np.int8),
            per_rank[r][1], periodic)[2])
        assert min(halo_rows) >= 2

    def fn(comm, r):
        p = per_rank[r][1]
        ids = (np.int64(r) << ID_BITS) + np.arange(len(p), dtype=np.int64)
        payload = [ids, (ids % 1000).astype(np.int32)][:nfields]
        t, sel = MpiHostComm(comm), RouteSelect()
        sp = halo_rows[r] - 1 if halo_rows else spare
        ov, _, m, in_arena, route = exchange(f, r, t, sel, payload if nfields > 1 else ids, p,
                                             periodic, spare=sp, return_route=True)
        assert (route.n_local, route.n_halo) == (len(p), m)
        if sp is not None:
            assert in_arena == (m <= sp)
        local = [_values(size + r, len(p), e, c) for e, c in kinds]
        accs = [_flat(x) for x in local]
        vals = [_flat(_values(r, m, e, c)) for e, c in kinds]
        elems, ncomps = [e for e, _ in kinds], [c for _, c in kinds]
        R = GeoRank(f["topology"], f["box"], size, r)
        if nfields > 1:
            reduce_overload(R, t, route, accs, vals, elems, ncomps, sel=sel)
        else:
            reduce_overload(R, t, route, accs[0], vals[0], elems[0], ncomps[0], sel=sel)
        ov_ids = (ov[0] if nfields > 1 else ov).numpy().view(np.int64).copy()
        return ov_ids, [a.numpy().view(_ELEM_NP[e]).reshape(-1, c)
                        for a, (e, c) in zip(accs, kinds)]

    res = run_ranks(size, fn)
    exp = [[_values(size + r, len(per_rank[r][1]), e, c) for e, c in kinds] for r in range(size)]
    copies = 0
    for r, (ov_ids, _) in enumerate(res):
        owner, row = ov_ids >> ID_BITS, ov_ids & ((1 << ID_BITS) - 1)
        copies += len(ov_ids)
        for i, (e, c) in enumerate(kinds):
            v = _values(r, len(ov_ids), e, c)
            for o in np.unique(owner):
                np.add.at(exp[o][i], row[owner == o], v[owner == o])
    assert copies > 0
    for r, (_, got) in enumerate(res):
        for i in range(nfields):
            assert np.array_equal(got[i], exp[r][i]), (case, r, i)
