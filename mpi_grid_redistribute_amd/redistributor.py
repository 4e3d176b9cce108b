"""MPIGridRedistributor -- the reference API (redist.py) on MI355X.

Drop-in for ``dkorytov/mpi_grid_redistribute``'s ``MPIGridRedistributor``
(redist.py:15-329) and ``mpi_grid_redistribute`` (redist.py:11-13): same
constructor, method names, argument meaning, array layout and results
(bit-exact, tests/test_gpu_parity.py), with the hot path
``redistribute_by_position`` (redist.py:115-166) running as hand-written HIP
kernels (libmgr.so) and the ``comm.alltoall`` exchange (redist.py:199)
replaced by RCCL grouped send/recv over xGMI (comm.RcclComm).

Per call of ``redistribute_by_position`` (one rank = one GPU):
  1. bin_count   wrap + write back positions, cell id per row, tile histograms
  2. scan        device-wide exclusive scan -> per-(bin, tile) segment starts
  3. counts      RCCL all-to-all of the count row, one host sync (sizes)
  4. pack        stable LDS-staged partition of every payload field into the
                 send buffer; the self segment goes straight into the output
  5. exchange    grouped ncclSend/ncclRecv, receives land at source-ordered
                 offsets of the output (S7): no unpack pass.

Documented divergences from the reference:
  * a rank with no particles returns what it receives instead of raising
    ValueError at redist.py:158 (S5);
  * ``mpi_grid_redistribute`` works (the reference's calls a misspelled
    method, redist.py:13, S13);
  * ``return_positions=True`` returns ``(data, positions)`` (the reference
    documents it as not implemented and ignores it, redist.py:141-145);
  * the overload (halo) exchange (redist.py:202-309, halo.py) needs one rank
    per grid cell (the reference deadlocks otherwise);
  * payloads are moved as bytes: object dtypes are refused (the reference
    pickles them).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._arrays import Positions, Rows, id_array, device, pos_code
from ._stage import (_TORCH_POS, MAX_FIELDS, Scratch, _alias_rows, _i64s, _offsets_like, _payload,
                     _Plan, _ptrs, _results, _scratch, _tile_hint, bin_count, _FinePlans,
                     pack_fields, scan, unpack_fields)
from .comm import SelfComm, as_transport
from .exchange import (check_counts, exchange, exchange_back, exchange_pipelined, host_read_start,
                       host_read_wait)
from .halo import (DeviceSelect, HaloRoute, exchange_overload, halo_capacity, reduce_overload,
                   thresholds)
from .partitioner import GridPartitioner   # noqa: F401  (re-exported, as the names below)
from .sort import (CELLS_MAX, GHOST_MAX_CELLS, SortRoute, _check_sort_route,  # noqa: F401
                   _fine_sort, _IdField, _sort_by_cells, _sort_by_ids, _unsort_into, ghost_grid)


class Route:
    """What ``return_to_source`` needs to send per-row results back along a
    redistribution (``return_route=True``): the rows' destination bytes, the
    workspace as the scan left it (every (bin, tile) segment start), the tile
    size, bin count and drop bin, and the exchange's layout.  The two device
    buffers are TAKEN OUT of the redistributor's scratch -- no copy; the next
    call on the redistributor allocates a new workspace and destination array
    -- so a route stays valid across later calls and may be used any number
    of times.  Memory per live route: about n_source * mgr_dest_bytes(nbins) +
    mgr_workspace_bytes(n_source, nbins, tile_rows) bytes (1-2 bytes per row
    plus 12 bytes per (bin, tile)), freed by ``release()``.  ``halo``: the
    HaloRoute of a call with ``overload_lengths`` and ``reduce_route=True``
    (else None); ``n_halo`` the overload rows that call appended after the
    ``n_local`` redistributed ones.  ``release()`` releases both."""

    def __init__(self, owner, dest, ws, tile_rows, nbins, drop_bin, n_source, layout, halo=None):
        self._owner = owner
        self._dest, self._ws = dest, ws
        self.tile_rows, self.nbins, self.drop_bin = int(tile_rows), int(nbins), int(drop_bin)
        self.n_source = int(n_source)
        self.n_local = int(layout.total_recv)
        self.layout = layout
        self.halo = halo

    @property
    def n_halo(self):
        """Overload rows appended after the n_local rows (0 without a halo)."""
        return self.halo.n_halo if self.halo is not None else 0

    @property
    def send_counts(self):
        """Rows the forward call sent to every rank (host int64, a copy)."""
        return self.layout.send_counts.copy()

    @property
    def recv_counts(self):
        """Rows the forward call received from every rank (host int64, a copy)."""
        return self.layout.recv_counts.copy()

    @property
    def released(self):
        return self._ws is None

    def release(self):
        """Free the route's device memory (its halo route's too); it cannot be
        used afterwards."""
        self._dest = self._ws = None
        if self.halo is not None:
            self.halo.release()


# reduce_overload's element types: numpy / torch dtype -> (mgr_elem_t, numpy dtype)
_REDUCE_ELEMS = {"float32": _lib.MGR_ELEM_F32, "float64": _lib.MGR_ELEM_F64,
                 "int32": _lib.MGR_ELEM_I32, "int64": _lib.MGR_ELEM_I64}


def _reduce_elem(f, what):
    """(mgr_elem_t, ncomp) of a Rows field, or TypeError naming the four types."""
    name = str(f.dtype).replace("torch.", "")
    if name not in _REDUCE_ELEMS:
        raise TypeError(f"{what}: dtype {f.dtype} cannot be reduced (float32, float64, int32 "
                        "or int64)")
    return _REDUCE_ELEMS[name], max(int(np.prod(f.trailing, dtype=np.int64)), 1)


def exchange_chunks_for(size, row_bytes):
    """Product default of the pipelined exchange's chunk count: 4 chunks on
    more than one rank (each chunk's rows travel while the next packs), 1 on
    one rank (nothing travels).  Rank-independent by construction (world
    size and the fields' row bytes are the same on every rank), as the
    protocol requires: the per-chunk counts are part of the count message.
    A size threshold is deliberately absent: the count of chunks cannot depend
    on this rank's row count (an empty rank must agree with a full one)."""
    return 4 if int(size) > 1 and int(row_bytes) > 0 else 1


class MPIGridRedistributor(_FinePlans):
    """Redistributes data by position onto a Cartesian grid of ranks
    (redist.py:15-61).  ``comm``: an ``RcclComm`` (one process per GPU), a
    ``SelfComm``/None (one rank), or any mpi4py-style communicator."""

    def __init__(self, comm, grid_topology, box_length):
        _lib.require_gpu()
        self.comm = as_transport(comm)
        # redist.py:40 np.array(..., dtype=np.int): truncating integer cast
        self.grid_topology = np.array(grid_topology).astype(np.int64)
        self.rank = self.comm.Get_rank()
        self.size = self.comm.Get_size()
        ranks_required = int(np.prod(self.grid_topology))
        assert ranks_required <= self.size, (
            "We have have {} ranks. The topology {} requires at least {} ranks".format(
                self.size, self.grid_topology, ranks_required))
        self.dim = len(self.grid_topology)
        self.box_length = np.array(box_length)
        assert self.dim == len(self.box_length), (
            "The number dimensions in grid_topoloby ({}), must be the same as in box_length "
            "({})".format(len(self.grid_topology), len(self.box_length)))
        self.cell_length = np.zeros(self.dim)
        for d in range(self.dim):
            self.cell_length[d] = self.box_length[d] / self.grid_topology[d]
        self.cell_index_offset = np.zeros(self.dim, dtype=np.int64)
        off = 1
        for j in range(self.dim - 1, -1, -1):
            self.cell_index_offset[j] = off
            off *= int(self.grid_topology[j])
        self.rank_cell_index = self.get_indexes_from_cell_number(np.array([self.rank]))[0]
        self.rank_cell_limits = self.get_cell_limits_from_indexes(
            np.array([self.rank_cell_index]))[0]
        self._plan = _Plan(self.grid_topology, self.box_length, self.size)
        self._fine_plans = {}
        self._dev = device()
        self._scratch = Scratch(self._dev)
        # > 1: the pack and the row exchange overlap in this many chunks of
        # tiles (exchange_pipelined); 1: pack everything, then one exchange;
        # None: the product default (exchange_chunks_for: 4 on > 1 rank)
        self.exchange_chunks = None

    def set_write_back(self, mode):
        """How the periodic wrap writes ``position`` back (redist.py:68 mutates
        it in place): "changed" (default) stores a 64-row slab only if one of
        its coordinates changed, "all" stores every slab -- the same bytes in
        memory either way; "all" is the cost of fresh input (bench.py).  Per
        redistributor (mgr_plan_set_write_back), not process-wide."""
        self._plan.set_write_back(mode)

    # ------------------------------------------------------ binning (L1)
    def get_cell_indexes_from_position(self, position, periodic=True):
        """redist.py:63-71: (N, dim) int64 cell indexes; wraps ``position`` in
        place when periodic."""
        return self._cell_ids(position, periodic, want_idx=True)[1]

    def get_cell_number_from_position(self, position, periodic=True):
        """redist.py:87-90 (indexes always wrap, :90)."""
        return self._cell_ids(position, periodic, want_idx=False)[0]

    def _cell_ids(self, position, periodic, want_idx):
        pos = Positions(position, self.dim, self._dev)
        n = pos.n
        cell = torch.empty(n, dtype=torch.int64, device=self._dev)
        idx = torch.empty((n, self.dim), dtype=torch.int64, device=self._dev) if want_idx else None
        _lib.call("mgr_cell_ids", self._plan.h, ctypes.c_void_p(pos.addr), pos.code, n,
                  pos.stride, int(bool(periodic)), _lib.ptr(cell), _lib.ptr(idx),
                  _lib.stream_handle())
        pos.finish()
        return self._like(position, cell), (self._like(position, idx) if want_idx else None)

    def get_cell_number_from_indexes(self, indexes, periodic=True, check_range=True):
        """redist.py:73-85.  Non-periodic: plain dot; the reference's range
        check uses ``&`` (redist.py:80) and never selects, kept as is."""
        t = indexes if isinstance(indexes, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(indexes)))
        t = t.to(self._dev, dtype=torch.int64).contiguous()
        if t.dim() != 2 or t.shape[1] != self.dim:
            raise ValueError(f"indexes must be (N, {self.dim})")
        cell = torch.empty(t.shape[0], dtype=torch.int64, device=self._dev)
        _lib.call("mgr_cell_number_from_indexes", self._plan.h, _lib.ptr(t), t.shape[0],
                  int(bool(periodic)), _lib.ptr(cell), _lib.stream_handle())
        return self._like(indexes, cell)

    def get_indexes_from_cell_number(self, cell_numbers):
        """redist.py:92-97 (host geometry helper: true division, truncation)."""
        torch_in = isinstance(cell_numbers, torch.Tensor)
        c = cell_numbers.cpu().numpy() if torch_in else np.asarray(cell_numbers)
        out = np.zeros((len(c), self.dim), dtype=int)
        for d in range(self.dim):
            out[:, d] = c / self.cell_index_offset[d]
            c = c % self.cell_index_offset[d]
        return torch.from_numpy(out).to(cell_numbers.device) if torch_in else out

    def get_cell_limits_from_indexes(self, cell_indexes):
        """redist.py:99-113 (host geometry helper)."""
        torch_in = isinstance(cell_indexes, torch.Tensor)
        ci = cell_indexes.cpu().numpy() if torch_in else np.asarray(cell_indexes)
        lim = np.zeros((len(ci), self.dim, 2))
        for d in range(self.dim):
            lim[:, d, 0] = ci[:, d] * self.cell_length[d]
            lim[:, d, 1] = (ci[:, d] + 1) * self.cell_length[d]
        return torch.from_numpy(lim).to(cell_indexes.device) if torch_in else lim

    # ------------------------------------------------- redistribution (L2)
    def redistribute_by_position(self, data, position, periodic=True, overload_lengths=None,
                                 return_positions=False, fine_cells=None, return_route=False,
                                 reduce_route=False):
        """redist.py:115-166.  Returns the rows of ``data`` whose position
        falls in this rank's cell, from every rank, in source-rank order;
        ``position`` is wrapped in place when periodic (S1).  ``data`` may be
        one array or -- SoA -- a tuple / list of arrays sharing axis 0 (e.g.
        ``(pos, vel, mass, ids)``): every field moves with the same
        destinations (one binning, one scan, one count exchange, one pack
        launch, one RCCL group) and the result is a tuple in the same order.
        With ``overload_lengths`` the halo rows follow (redist.py:161-166; the
        halo exchange always runs periodic, :165).  With ``fine_cells``
        (config 5, no reference counterpart) the received rows come back
        stably sorted by fine cell with their offsets, = ``fine_cell_sort``
        of the plain result, computed from fine cells binned at the source.
        ``return_positions``: (data, positions) -- (data, [positions,]
        offsets) with ``fine_cells``; ``data`` is the tuple of fields for a
        SoA payload.  ``overload_lengths`` together with ``fine_cells`` (one
        array, float32 / float64 positions): the ghost cell list -- the
        received rows and their halo rows, the halo positions unwrapped,
        sorted over the extended grid: what ``ghost_cell_sort`` returns for
        them, (data, [positions,] offsets[prod(extents) + 1]).
        ``return_route``: (result, route) -- ``result`` is what
        the call returns otherwise, ``route`` a Route for ``return_to_source``
        (rows of any dtype go back one to one).  Not with ``overload_lengths``:
        halo rows are copies and their return is a reduction, a different
        contract, which ``reduce_route=True`` selects: (result, route) where
        the Route also holds the halo exchange's HaloRoute (``route.halo``;
        ``route.n_local`` redistributed rows, ``route.n_halo`` appended
        overload rows).  ``return_to_source`` then takes values of n_local +
        n_halo rows (the layout this call returned) of float32, float64, int32
        or int64, sums every overload row's value onto the row it is a copy of
        (``reduce_overload``) and sends the n_local sums home;
        ``route.release()`` releases both.  (The same in separate calls:
        ``return_positions=True, return_route=True``, then
        ``exchange_overload_by_position(..., return_route=True)``,
        ``reduce_overload`` and ``return_to_source``.)  Not with ``fine_cells``
        in this one call: redistribute with ``return_route=True``, then
        ``fine_cell_sort(..., return_route=True)``, and give both routes to
        ``return_to_source(values, route, sort_route=...)``."""
        if reduce_route and (overload_lengths is None or fine_cells is not None or return_route):
            raise ValueError("reduce_route=True goes with overload_lengths alone (no fine_cells, "
                             "no return_route): it is the route of a call with a halo")
        if return_route and (overload_lengths is not None or fine_cells is not None):
            raise NotImplementedError(
                "return_route together with overload_lengths or fine_cells: halo rows are "
                "copies, their return is a reduction onto the owners -- with overload_lengths "
                "pass reduce_route=True (return_to_source then takes n_local + n_halo values "
                "and sums the halo part onto the owners), or call "
                "redistribute_by_position(..., return_positions=True, return_route=True), "
                "exchange_overload_by_position(..., return_route=True), "
                "reduce_overload(halo_values, halo_route, local_values=...) and "
                "return_to_source(sums, route); for fine_cells use the "
                "two-call route -- redistribute_by_position(..., return_positions=True, "
                "return_route=True), then fine_cell_sort(..., return_route=True), then "
                "return_to_source(values, route, sort_route=...)")
        fields, multi = _payload(data, self._dev)
        for d in (data if multi else [data]):
            self._check_host_alias(d, position)
        self.comm.reset_traffic()
        pos = Positions(position, self.dim, self._dev, data_rows=_alias_rows(position, fields))
        n = fields[0].n
        if pos.n != n:
            raise ValueError(f"data has {n} rows, position has {pos.n}")
        if fine_cells is not None and overload_lengths is not None:
            # the ghost cell list: owned + halo rows, halo positions unwrapped,
            # sorted over the extended grid
            if multi:
                raise NotImplementedError(
                    "overload_lengths and fine_cells with a SoA (tuple) payload in one call: "
                    "redistribute_by_position(fields, pos, return_positions=True), then "
                    "exchange_overload_by_position(fields, local_pos, overload_lengths, "
                    "return_positions=True, unwrap=True), then ghost_cell_sort on the "
                    "concatenated fields")
            self._check_halo(overload_lengths)
            if pos.code not in _TORCH_POS:
                raise TypeError("overload_lengths with fine_cells: float32 or float64 positions")
            self.ghost_grid(fine_cells, overload_lengths)   # refuse a grid too large up front
            info = {}
            both, both_pos = self._redistribute_halo(data, position, fields[0], pos, periodic,
                                                     overload_lengths, True, unwrap=True,
                                                     info=info)
            return self.ghost_cell_sort(both, both_pos, info["n_local"], fine_cells,
                                        overload_lengths, return_positions=return_positions)
        if fine_cells is not None:
            return self._redistribute_fine(data, position, fields, multi, pos, periodic,
                                           fine_cells, return_positions)
        halo = overload_lengths is not None
        if halo:
            if multi:
                raise NotImplementedError(
                    "overload_lengths with a SoA (tuple) payload in one call: use "
                    "redistribute_by_position(fields, pos, return_positions=True), then "
                    "exchange_overload_by_position(fields, local_pos, overload_lengths) on "
                    "the result, and concatenate the two per field")
            self._check_halo(overload_lengths)
            return self._redistribute_halo(data, position, fields[0], pos, periodic,
                                           overload_lengths, return_positions, reduce_route)
        outs, m, prow, ran = self._forward(fields, position, pos, periodic, return_positions)
        res = _results(fields, outs[:len(fields)], m, multi)
        if return_positions:
            res = res, prow.wrap(outs[-1], m)
        return (res, self._take_route(ran)) if return_route else res

    def _forward(self, fields, position, pos, periodic, return_positions, side=None, fine=None,
                 halo=None, **run_kw):
        """_run of the payload ``fields``, then the rows' 2-byte ``side`` field
        if any (fine cells, halo flags), then with ``return_positions`` the
        wrapped position rows (redist.py:164), binned by bin_count(fine=, halo=).
        Returns (outs in that order, m, the positions' Rows, _run's value)."""
        run_fields = list(fields) + ([side] if side is not None else [])
        hint = [f.row_bytes for f in run_fields]
        if return_positions:
            run_fields.append(None)   # known after the wrap
            hint.append(int(position.shape[1]) * _lib.POS_ITEMSIZE[pos.code])

        def binner(dest, tile_rows, ws):
            bin_count(self._plan, pos, periodic, dest, tile_rows, ws, _lib.stream_handle(),
                      fine=fine, halo=halo)
            pos.finish()
            if return_positions:   # the wrapped positions, full rows
                run_fields[-1] = Rows(position, self._dev)

        outs, m, ran = self._run(run_fields, binner, fields[0].n, drop=False,
                                 row_bytes_hint=hint,
                                 side=len(fields) if side is not None else None, **run_kw)
        return outs, m, run_fields[-1] if return_positions else None, ran

    def _take_route(self, ran):
        """The Route of the _run that returned ``ran``; ws and dest leave the scratch."""
        ws, dest = self._scratch.take("ws"), self._scratch.take("dest")
        return Route(self, dest, ws, *ran)

    def unsort(self, values, sort_route):
        """The inverse of the ``fine_cell_sort`` that made ``sort_route``
        (``return_route=True``): ``values`` -- one array, or a tuple / list of
        up to MAX_FIELDS arrays, of ``sort_route.n`` rows each, of any dtype
        and trailing shape, in sorted order (forces, densities, tags computed
        per sorted row) -- come back in the order the rows had before the
        sort: row i is the value of the row that was row i.  Containers as
        ``return_to_source``.  One launch for all fields
        (mgr_unpack_ranked_fields; mgr_unpack_fields for a sort that took the
        non-ranked path); nothing is ranked or scanned again."""
        _check_sort_route(sort_route)
        fields, multi = _payload(values, self._dev)
        n = sort_route.n
        for i, f in enumerate(fields):
            if f.n != n:
                raise ValueError(f"values field {i} has {f.n} rows, the sort route has {n}")
        rbs = [f.row_bytes for f in fields]
        outs = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=self._dev) for rb in rbs]
        _unsort_into(sort_route, [f.flat for f in fields], rbs, outs)
        return _results(fields, outs, n, multi)

    def return_to_source(self, values, route, sort_route=None):
        """The inverse of the redistribution that made ``route``: ``values``
        -- one array, or a tuple / list of up to MAX_FIELDS arrays, of
        ``route.n_local`` rows each, of any dtype and trailing shape (per-row
        results computed on the owning rank: forces, densities, tags ...) --
        go back to the ranks and rows they came from.  Returns arrays of
        ``route.n_source`` rows in the container of ``values`` (numpy in,
        numpy out; GPU torch in, GPU torch out): row i is the value computed
        for the call's original row i; a row ``redistribute_by_cell_number``
        dropped is zero.  One reverse row exchange (exchange_back: the forward
        messages with sender and receiver swapped, no count exchange, no host
        sync) and one mgr_unpack_fields call; nothing is binned or scanned
        again.  ``sort_route`` (a SortRoute of ``fine_cell_sort(...,
        return_route=True)`` on the rows the route delivered): ``values`` are
        in fine-cell order; they are unsorted straight into the buffers the
        reverse exchange sends from (one mgr_unpack_ranked_fields launch, no
        further copy).  A route of a call with ``overload_lengths`` and
        ``reduce_route=True`` (``route.halo``): ``values`` have ``route.n_local
        + route.n_halo`` rows, the layout that call returned, of float32,
        float64, int32 or int64; the halo part is first summed onto the rows it
        copies (``reduce_overload``), so original row i gets its own value
        plus the values of all its overload copies."""
        if not isinstance(route, Route):
            raise TypeError("route: a Route of redistribute_by_position(..., return_route=True)")
        if route.released:
            raise ValueError("the route was released")
        self._check_owner(route._owner)
        halo = route.halo
        if halo is not None and sort_route is not None:
            raise NotImplementedError("sort_route with a route that holds a halo: unsort, then "
                                      "reduce_overload, then return_to_source")
        if sort_route is not None:
            _check_sort_route(sort_route)
            if sort_route.n != route.n_local:
                raise ValueError(f"the sort route has {sort_route.n} rows, the route delivered "
                                 f"{route.n_local}")
        fields, multi = _payload(values, self._dev)
        n_in = route.n_local + route.n_halo
        for i, f in enumerate(fields):
            if f.n != n_in:
                raise ValueError(f"values field {i} has {f.n} rows, the route delivered "
                                 f"{n_in}")
        self.comm.reset_traffic()
        n, stream = route.n_source, _lib.stream_handle()
        rbs = [f.row_bytes for f in fields]
        flats = [f.flat for f in fields]
        if halo is not None:
            # the halo part summed onto the first n_local rows (a copy: the
            # caller's values are not written), which then go home
            self._check_halo_route(halo)
            kinds = [_reduce_elem(f, f"values field {i}") for i, f in enumerate(fields)]
            nl = route.n_local
            accs = [self._scratch.get(f"halo_red_acc{i}", nl * rb) for i, rb in enumerate(rbs)]
            for a, t, rb in zip(accs, flats, rbs):
                a[: nl * rb].copy_(t[: nl * rb])
            self._reduce_into(halo, accs, [t[nl * rb:] for t, rb in zip(flats, rbs)], kinds)
            flats = [a[: nl * rb] for a, rb in zip(accs, rbs)]
        if sort_route is not None:   # out of fine-cell order, into the send buffers
            flats = [self._scratch.get(f"unsort{i}", route.n_local * rb)
                     for i, rb in enumerate(rbs)]
            _unsort_into(sort_route, [f.flat for f in fields], rbs, flats)

        def unpack_all(stagings, vals, redirect_bin, offs):
            outs = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=self._dev)
                    for rb in rbs]
            # an empty field has no address: no row reads it, any pointer serves
            reds = [(v.data_ptr() or s.data_ptr()) + o for v, s, o in zip(vals, stagings, offs)]
            unpack_fields([s.data_ptr() for s in stagings], rbs, n, route._dest, route.nbins,
                          route.drop_bin, route.tile_rows, route._ws,
                          [t.data_ptr() for t in outs], stream, redirect_bin, reds)
            return outs

        outs = exchange_back(self.comm, rbs, route.layout, flats, self.rank,
                             self._dev, unpack_all, scratch=self._scratch.get)
        return _results(fields, outs, n, multi)

    def _redistribute_halo(self, data, position, rows, pos, periodic, overload_lengths,
                           return_positions, return_route=False, unwrap=False, info=None):
        """redist.py:157-166 with overload_lengths: the binning kernel also
        writes every row's halo face flags against the cell it lands in
        (mgr_bin_count_halo); rows, flags (a side field of the same pack) and
        wrapped positions (:164) are redistributed together; the overload
        exchange (halo.py) then starts from the received flags and appends
        the halo rows in place after the m received rows while they fit the
        spare capacity (no concatenation copies).  ``unwrap``: the halo rows'
        positions come back unwrapped (halo.exchange_overload); ``info``: a
        dict that receives ``n_local``, the redistributed rows before the
        halo's."""
        flags_src = self._scratch.get("halo_flags_src", max(rows.n, 1) * 2)
        rp = bool(return_positions)
        # one rank: the rows keep their order (one bin, nothing dropped), so the
        # selections read the binning's flags in place -- no flag field packed
        one = self.size == 1
        cl = np.ascontiguousarray(self.cell_length, dtype=np.float64)
        ol = np.ascontiguousarray(np.asarray(overload_lengths, dtype=np.float64))
        extra = lambda m_: halo_capacity(self, m_, overload_lengths)  # noqa: E731
        pending = []   # one rank: the scan's counts checked at the halo's host read
        outs, m, prow, ran = self._forward(
            [rows], position, pos, periodic, rp, side=None if one else _IdField(flags_src),
            halo=(flags_src, cl, ol), extra_rows=extra, deferred=pending)
        rbd = rows.row_bytes
        rbp = prow.row_bytes if rp else 0
        cap = outs[0].numel() // max(rbd, 1) - m
        fsrc = flags_src if one else outs[1]
        flags = fsrc[: 2 * m].view(torch.int16) if m else torch.empty(
            0, dtype=torch.int16, device=self._dev)
        op = outs[-1] if rp else None
        route = None
        if return_route:   # before the halo: its selections reuse scratch names
            route = self._take_route(ran)
            if one:   # the binning's flags stay with the route
                self._scratch.take("halo_flags_src")
        ov_d, ov_p, mo, in_place, *hr = exchange_overload(
            self, self.comm, outs[0][: m * rbd], rbd, op[: m * rbp] if rp else None,
            int(position.shape[1]), pos.code, m, list(overload_lengths), periodic=True,
            sel=DeviceSelect(self._dev, self._scratch),
            arena=(outs[0], op, m, cap), flags=flags, pending=pending,
            return_route=return_route, unwrap=unwrap)
        if return_route:
            route.halo = hr[0]
        if info is not None:
            info["n_local"] = m
        if in_place:   # redist.py:166: concatenate(data, overload)
            res_d = outs[0][: (m + mo) * rbd]
            res_p = op[: (m + mo) * rbp] if rp else None
        else:
            res_d = torch.cat([outs[0][: m * rbd], ov_d])
            res_p = torch.cat([op[: m * rbp], ov_p]) if rp else None
        res = rows.wrap(res_d, m + mo)
        if rp:
            res = res, prow.wrap(res_p, m + mo)
        return (res, route) if return_route else res

    def _redistribute_fine(self, data, position, fields, multi, pos, periodic, fine_cells,
                           return_positions):
        """Source: bin + fine cell of every row (mgr_bin_count_fine), the
        fine cells packed and exchanged as a 2-byte side field beside the
        payload's fields; destination: rank -> scan -> pack of every field by
        the received fine cells."""
        fplan = self._fine_plan(fine_cells)
        n, nd = fields[0].n, len(fields)
        fids = self._scratch.get("fine_src", max(n, 1) * 2)
        outs, m, prow, _ = self._forward(fields, position, pos, periodic, return_positions,
                                         side=_IdField(fids), fine=(fplan, fids))
        ids = outs[nd][: 2 * m].view(torch.int16) if m else torch.empty(0, dtype=torch.int16,
                                                                         device=self._dev)
        recv = [_IdField(outs[i + (i >= nd)], f.row_bytes)   # every field but the ids
                for i, f in enumerate(fields + ([prow] if prow else []))]
        sorted_, counts = _sort_by_ids(recv, ids, m, fplan.nbins, self._dev, self._scratch,
                                       check_ids=False)   # binned here: in range
        res = [_results(fields, sorted_[:nd], m, multi)]
        if return_positions:
            res.append(prow.wrap(sorted_[nd], m))
        return tuple(res) + (_offsets_like(fields[0].obj, counts, self._dev),)

    def exchange_overload_by_position(self, data, position, overload_lengths,
                                      return_positions=False, periodic=True, return_route=False,
                                      unwrap=False):
        """redist.py:202-309: the overload (halo) rows of this rank's cell
        from its neighbours; ``data``/``position`` are this rank's local rows
        (already redistributed).  ``return_positions`` (ignored by the
        reference) returns (data, positions).  ``data`` may be a SoA payload,
        a tuple / list of arrays sharing axis 0 as in
        ``redistribute_by_position``: every field's overload rows move with
        the same selections (one flags pass, one selection count and one pack
        launch per step, one message group per dimension) and come back as a
        tuple in the same order -- what the reference gives called once per
        field with the same positions.  ``return_route``: a HaloRoute for
        ``reduce_overload`` is appended to the result (it owns the rows' face
        flags and the selections' workspaces, about 2 * (n_local + n_halo)
        bytes plus the workspaces, until ``release()``); without it nothing
        more is allocated, copied or launched.  ``unwrap`` (with
        ``return_positions``; float32 / float64 positions): the returned
        positions of the overload rows are the periodic images beside this
        rank's cell -- a row that came across the box boundary reads x + L or
        x - L, so a left and a right copy of the same row differ -- instead of
        the owners' coordinates (the reference's); what ``ghost_cell_sort``
        takes.  The data rows, their count and order do not change."""
        self._check_halo(overload_lengths)
        if unwrap and not return_positions:
            raise ValueError("unwrap=True needs return_positions=True (the positions are what "
                             "it changes)")
        fields, multi = _payload(data, self._dev)
        self.comm.reset_traffic()
        rows = fields[0]
        prow = Rows(position, self._dev)
        if not (isinstance(position, (np.ndarray, torch.Tensor)) and position.ndim == 2
                and position.shape[1] >= self.dim):
            raise ValueError(f"position must be (N, >= {self.dim})")
        code = pos_code(position.dtype)
        if prow.n != rows.n:
            raise ValueError(f"data has {rows.n} rows, position has {prow.n}")
        sel = DeviceSelect(self._dev, self._scratch)
        ncols = int(position.shape[1])
        flags, pflat = None, prow.flat
        if not return_positions:   # the flags are all the selections read
            hi, lo = thresholds(self, overload_lengths)
            flags = sel.flags(prow.flat, rows.n, ncols, code, self.dim, hi, lo)
            pflat = None
        ov_d, ov_p, mo, _, *hr = exchange_overload(
            self, self.comm, [f.flat for f in fields] if multi else rows.flat,
            [f.row_bytes for f in fields] if multi else rows.row_bytes, pflat, ncols, code,
            rows.n, list(overload_lengths), periodic=bool(periodic), sel=sel, flags=flags,
            return_route=return_route, unwrap=bool(unwrap))
        res = _results(fields, ov_d if multi else [ov_d], mo, multi)
        if return_positions:
            res = res, prow.wrap(ov_p, mo)
        if not return_route:
            return res
        return (res + (hr[0],)) if return_positions else (res, hr[0])

    def _check_halo_route(self, halo_route):
        if not isinstance(halo_route, HaloRoute):
            raise TypeError("halo_route: a HaloRoute of exchange_overload_by_position(..., "
                            "return_route=True)")
        if halo_route.released:
            raise ValueError("the halo route was released")
        self._check_owner(halo_route._owner)

    def _check_owner(self, o):
        if o is not self and (o.size != self.size or o.rank != self.rank
                              or not np.array_equal(o.grid_topology, self.grid_topology)
                              or not np.array_equal(o.box_length, self.box_length)):
            raise ValueError("the route was made by another redistributor (different size, "
                             "rank or plan)")

    def reduce_overload(self, values, halo_route, local_values=None):
        """The halo exchange that made ``halo_route``, backwards, with a sum
        (``exchange_overload_by_position(..., return_route=True)``): ``values``
        -- one array, or a tuple / list of up to MAX_FIELDS arrays, of
        ``halo_route.n_halo`` rows each (results computed on the overload
        rows: force contributions, deposits, neighbour counts ...), float32,
        float64, int32 or int64 with any trailing shape -- are summed onto the
        rows they are copies of.  Returns arrays of ``halo_route.n_local``
        rows in the container of ``values`` (numpy in, numpy out; GPU torch
        in, GPU torch out): row i is ``local_values[i]`` (same shapes and
        dtypes as ``values`` with n_local rows; zero when None) plus the
        values on every overload copy of local row i, anywhere in the world
        -- the copies of copies in edge and corner regions included.  Neither
        ``values`` nor ``local_values`` is written.

        Nothing is binned, scanned or counted again and no host sync is
        needed: per dimension, backwards, one message group with the forward
        sizes swapped, and one mgr_msel_unpack_add call per field and step
        (halo.reduce_overload).

        Summation order: a row's contributions are added one at a time in an
        order fixed by the grid and the rank count, so results are
        bit-identical from run to run.  For floats they may differ in the
        last bits between layouts (one rank adds a row's pieces flat, several
        ranks add them nested, dimension by dimension); integer types and
        exactly representable sums are identical everywhere."""
        self._check_halo_route(halo_route)
        fields, multi = _payload(values, self._dev)
        for i, f in enumerate(fields):
            if f.n != halo_route.n_halo:
                raise ValueError(f"values field {i} has {f.n} rows, the halo route has "
                                 f"{halo_route.n_halo} overload rows")
        kinds = [_reduce_elem(f, f"values field {i}") for i, f in enumerate(fields)]
        n = halo_route.n_local
        if local_values is None:
            accs = [torch.zeros(max(n * f.row_bytes, 1), dtype=torch.uint8, device=self._dev)
                    for f in fields]
        else:
            lf, lmulti = _payload(local_values, self._dev)
            if lmulti != multi or len(lf) != len(fields):
                raise ValueError("local_values: the same fields as values")
            accs = []
            for i, (l_, f) in enumerate(zip(lf, fields)):
                if l_.n != n:
                    raise ValueError(f"local_values field {i} has {l_.n} rows, the halo route "
                                     f"has {n} local rows")
                if l_.dtype != f.dtype or l_.trailing != f.trailing:
                    raise ValueError(f"local_values field {i}: dtype and trailing shape of "
                                     f"values field {i}")
                a = torch.empty(max(n * f.row_bytes, 1), dtype=torch.uint8, device=self._dev)
                a[: n * f.row_bytes].copy_(l_.flat[: n * f.row_bytes])
                accs.append(a)
        self.comm.reset_traffic()
        self._reduce_into(halo_route, accs, [f.flat for f in fields], kinds)
        return _results(fields, accs, n, multi)

    def _reduce_into(self, halo_route, accs, halo_flats, kinds):
        """accs[f] (flat, n_local rows) += the overload rows' halo_flats[f]."""
        reduce_overload(self, self.comm, halo_route, accs, halo_flats, [k[0] for k in kinds],
                        [k[1] for k in kinds], sel=DeviceSelect(self._dev, self._scratch))

    def fine_cell_sort(self, data, position, fine_cells, return_positions=False, fine_ids=None,
                       return_route=False):
        """Destination-side stable sort of this rank's rows by fine cell, for
        particle-mesh deposition (the reference has
        no such step).  The fine cell of a row is the reference's binning
        (redist.py:63-90) over the global grid grid_topology * fine_cells,
        reduced to the index inside the rank's cell (k_d % fine_cells[d]) and
        numbered row-major.  ``position`` is read, never wrapped (the rows were
        wrapped by the redistribution).  Returns (sorted data, offsets
        [prod(fine_cells)+1]) -- or (data, positions, offsets) with
        ``return_positions`` -- in the containers of the inputs.
        ``fine_ids``: the rows' fine cells as computed at the source
        (uint16, ``GridPartitioner.partition_device(..., fine_cells=...)`` /
        mgr_bin_count_fine); the rows are then not binned again.
        ``return_route``: a SortRoute is appended to the tuple, for ``unsort``
        and ``return_to_source(..., sort_route=)``; it owns the sort's ids,
        ranks, tile starts and workspace (SortRoute: about 4 B/row + 2 * T *
        nbins + the workspace) until ``release()``.  Without it nothing more
        is allocated, copied or launched than the sort itself."""
        return _fine_sort(self._fine_plan(fine_cells), self._plan, self.dim, self._dev, data,
                          position, return_positions, fine_ids, return_route)

    def ghost_grid(self, fine_cells, overload_lengths, max_cells=GHOST_MAX_CELLS):
        """(ghost, extents, origin, width) of this rank's extended fine grid
        (host numpy; the module's ``ghost_grid`` on this rank's cell): width =
        cell_length / fine_cells, ghost[d] = ceil(overload_lengths[d] /
        width[d]) layers on either side, extents = fine_cells + 2 * ghost,
        origin = the cell's lower corner.  ValueError beyond 1024 cells, or
        beyond ``max_cells`` (up to CELLS_MAX = 2^20) when given."""
        return ghost_grid(self.cell_length, self.rank_cell_limits, fine_cells, overload_lengths,
                          max_cells)

    def ghost_cell_sort(self, data, position, n_local, fine_cells, overload_lengths,
                        return_positions=False, return_route=False, max_cells=GHOST_MAX_CELLS):
        """The cell list a neighbour search, an SPH step or a CIC/TSC deposit
        needs: this rank's owned rows AND its halo rows, stably sorted over the
        extended grid of ``ghost_grid(fine_cells, overload_lengths)`` -- the
        rank's fine cells with ghost layers around them.  ``data``: one array
        or a SoA tuple / list of ``n_local + n_halo`` rows, the layout the halo
        calls return (owned rows first; the two-call form: concatenate the
        redistributed rows and the overload rows per field); ``position``
        ((N, >= dim) float32 / float64): their positions, the halo rows'
        unwrapped (``exchange_overload_by_position(..., unwrap=True)``).
        Returns (sorted data, offsets[prod(extents) + 1]) -- (data, positions,
        offsets) with ``return_positions`` -- in the containers of the inputs,
        plus a SortRoute with ``return_route`` (``unsort`` brings per-row
        results back to the n_local + n_halo layout, where ``reduce_overload``
        takes them).  Cell ids are row-major over ``extents``, last axis
        fastest; the block [ghost, ghost + fine) in every dimension holds
        exactly the owned rows (an owned row that rounds onto a face of the
        cell is clamped into it), the layers around it only halo rows.  A halo
        row beyond the ghost layers (a position that was not unwrapped, a NaN)
        is counted on the device and turns the offsets' counts to -1: host
        results raise, as after a failed scan.  One mgr_ghost_cells launch,
        then the ranked sort of fine_cell_sort (_sort_by_ids), unchanged.

        ``max_cells`` (up to CELLS_MAX = 2^20) opts into grids beyond 1024
        cells -- the cell counts a pair loop wants, tens of rows per cell.  A
        grid of at most 1024 cells takes the path above whatever ``max_cells``
        is; a larger one within ``max_cells`` gets 32-bit cell ids
        (mgr_ghost_cells_wide, the same arithmetic) and the two-digit stable
        sort (sort._sort_by_wide_ids: two passes of the 16-bit sort over digits
        of at most 10 bits, offsets from the sorted ids by mgr_cell_offsets).
        Inputs, results, the SortRoute (a WideSortRoute: ``unsort`` and
        ``return_to_source(..., sort_route=)`` take two launches) and the
        failure convention are the same; on the device a failure turns every
        offset to -1.  Device memory of a wide sort beside the inputs: about
        twice the payload + 12 B/row, of its route about 8 B/row.  With
        ``n_local = n`` and ``overload_lengths = 0`` this is a plain large
        cell list without a halo: the supported route to more than 4096 fine
        cells (fine_cell_sort and the one-call form keep their bounds)."""
        ghost, ext, origin, width = self.ghost_grid(fine_cells, overload_lengths, max_cells)
        dev, outside = self._dev, []
        wide = int(np.prod(ext)) > GHOST_MAX_CELLS

        def cell_ids(pos, n, fields):
            nl = int(n_local)
            if not 0 <= nl <= n:
                raise ValueError(f"n_local {nl} outside 0..{n}")
            # int32 ids: _sort_by_cells then runs the two-digit sort
            ids = torch.empty(max(n, 1), dtype=torch.int32 if wide else torch.int16, device=dev)
            outside.append(torch.zeros(1, dtype=torch.int32, device=dev))
            fine = np.array(fine_cells).astype(np.int64)
            _lib.call("mgr_ghost_cells_wide" if wide else "mgr_ghost_cells",
                      ctypes.c_void_p(pos.addr), pos.code, n, nl, pos.stride,
                      self.dim, origin.ctypes.data_as(ctypes.c_void_p),
                      width.ctypes.data_as(ctypes.c_void_p),
                      (ctypes.c_int * self.dim)(*[int(x) for x in fine]),
                      (ctypes.c_int * self.dim)(*[int(x) for x in ghost]), _lib.ptr(ids),
                      _lib.ptr(outside[0]), _lib.stream_handle())
            # read with the offsets: no sync of its own
            return (ids if wide else ids[:n], False,
                    lambda counts: counts.masked_fill_(outside[0].ne(0), -1))

        return _sort_by_cells(
            data, position, self.dim, dev, int(np.prod(ext)), cell_ids, return_positions,
            return_route, floats="ghost_cell_sort",
            failed="ghost_cell_sort: a halo row lies beyond the ghost layers (a position that "
                   "was not unwrapped or is NaN, or overload_lengths smaller than the halo's)")

    def get_cell_number_from_indexes_host(self, indexes, periodic=True):
        """redist.py:73-85 on the host (neighbour ranks of the halo exchange)."""
        indexes = np.asarray(indexes, dtype=np.int64)
        cell = np.zeros(len(indexes), dtype=np.int64)
        for d in range(self.dim):
            k = indexes[:, d]
            if periodic:
                n = self.grid_topology[d]
                k = ((k % n) + n) % n
            cell += self.cell_index_offset[d] * k
        return cell

    def _check_halo(self, overload_lengths):
        assert len(overload_lengths) == self.dim, \
            "Overload lengths must be the same length as the dimensions"  # redist.py:245
        if int(np.prod(self.grid_topology)) != self.size:
            # ranks without a cell have no neighbours: the reference's isend/irecv
            # pattern leaves them waiting forever
            raise NotImplementedError("overload exchange needs one rank per grid cell "
                                      f"({int(np.prod(self.grid_topology))} cells, "
                                      f"{self.size} ranks)")

    def redistribute_by_cell_number(self, data, rank_to_send, return_route=False):
        """redist.py:169-200: send row i to rank ``rank_to_send[i]``; ids
        outside [0, size) are dropped (S6).  ``data``: one array or a tuple /
        list of arrays sharing axis 0 (SoA), all sent with the same ids in one
        pass; the result is then a tuple in the same order.  ``return_route``:
        (result, route) for ``return_to_source``, where a dropped row comes
        back as zero bytes."""
        self.comm.reset_traffic()
        fields, multi = _payload(data, self._dev)
        n = fields[0].n
        ids, code = id_array(rank_to_send, self._dev)
        if ids.numel() != n:
            raise ValueError(f"data has {n} rows, rank_to_send has {ids.numel()}")

        def binner(dest, tile_rows, ws):
            _lib.call("mgr_bin_ids", self._plan.h, _lib.ptr(ids), code, n, _lib.ptr(dest),
                      tile_rows, _lib.ptr(ws), _lib.stream_handle())

        outs, m, ran = self._run(fields, binner, n, drop=True)
        res = _results(fields, outs, m, multi)
        return (res, self._take_route(ran)) if return_route else res

    def _run(self, fields, binner, n, drop, row_bytes_hint=None, extra_rows=None, side=None,
             deferred=None):
        """bin -> scan -> count exchange -> pack -> row exchange.  Every field
        (the payload's SoA fields, positions, side fields) is partitioned by
        the same destinations in one mgr_pack_fields call.  ``side``: the
        index of the rows' 2-byte side field (fine cells, halo flags), moved
        by the kernel that moves the other fields.  ``deferred`` (a
        list): on one rank without drops the counts are not read back; the
        scan's count tensor is appended to it for the caller's next host read
        to check.  Returns (outs, rows received, (tile rows, bins, drop bin, n,
        layout) for _take_route); the layout also stays for ``last_counts``."""
        P = self.size
        nb, drop_bin = (P + 1, P) if drop else (P, -1)
        hint = row_bytes_hint or [f.row_bytes for f in fields]
        tile_rows, ws, dest = _scratch(n, nb, _tile_hint(hint, side), self._dev,
                                       self._scratch)
        binner(dest, tile_rows, ws)
        stream = _lib.stream_handle()
        bin_counts = torch.empty(nb, dtype=torch.int64, device=self._dev)
        scan(n, nb, tile_rows, ws, bin_counts, stream)
        main = [f for f in range(len(fields)) if f != side]
        rbs = [f.row_bytes for f in fields]

        def pack(sends, outs, redirect_bin, offs, t0=0, t1=-1):
            """Every field, the 2-byte side field among them, in ONE
            mgr_pack_fields call; the redirect bin's rows straight into ``outs``."""
            r = redirect_bin >= 0
            sd = (None, None, None)
            if side is not None:
                sd = (fields[side].flat.data_ptr(), sends[side].data_ptr(),
                      outs[side].data_ptr() + offs[side] if r else None)
            pack_fields([fields[f].flat.data_ptr() for f in main], [rbs[f] for f in main], n,
                        dest, nb, drop_bin, tile_rows, ws, [sends[f].data_ptr() for f in main],
                        stream, redirect_bin,
                        [outs[f].data_ptr() + offs[f] for f in main] if r else None, sd, t0, t1)

        T = (n + tile_rows - 1) // tile_rows
        # the chunk count is part of the exchange protocol: the same on every
        # rank whatever its row count (a rank with fewer tiles than chunks --
        # an empty one included -- packs empty chunks); the size rule reads
        # only rank-independent inputs
        k = (exchange_chunks_for(P, sum(hint)) if self.exchange_chunks is None
             else max(1, int(self.exchange_chunks)))
        known, read = None, None
        if k > 1 and P > 1:
            # pipelined: pack the tiles in k chunks, each chunk's pieces travel
            # while the next is packed (exchange_pipelined)
            bounds = [T * c // k for c in range(k + 1)]

            def chunk_offsets():
                out = torch.empty((k + 1) * nb, dtype=torch.int64, device=self._dev)
                arr = (ctypes.c_int64 * (k + 1))(*bounds)
                _lib.call("mgr_tile_offsets", _lib.ptr(ws), n, nb, tile_rows, arr, k + 1,
                          _lib.ptr(out), stream)
                return out.view(k + 1, nb)[:, :P]   # device: read with the count message

            def pack_chunk(c, sends, outs, redirect_bin, offs):
                pack(sends, outs, redirect_bin, offs, bounds[c], bounds[c + 1])

            outs, lay = exchange_pipelined(self.comm, rbs, bin_counts[:P], self.rank, self._dev,
                                           chunk_offsets, pack_chunk, k, extra_rows=extra_rows,
                                           scratch=self._scratch.get)
        else:
            if P == 1 and not drop:
                # one rank keeping every row: the output size is n, so the pack is
                # launched without reading the counts first; they are checked (a
                # failed scan) by the caller's next host read, or here by a read
                # enqueued ahead of the pack and waited for while it runs
                known = n
                if deferred is not None:
                    deferred.append(bin_counts)
                else:
                    read = host_read_start([bin_counts])
            outs, lay = exchange(self.comm, rbs, bin_counts[:P], self.rank, self._dev, None,
                                 extra_rows=extra_rows, scratch=self._scratch.get,
                                 pack_all=pack, known_rows=known)
            if read is not None:
                check_counts(host_read_wait(read)[0], [])
        self._last_layout = lay
        return outs, lay.total_recv, (tile_rows, nb, drop_bin, n, lay)

    @property
    def last_counts(self):
        """(send_counts, recv_counts) of the last redistribution on this rank:
        host int64 arrays of rows sent to / received from every rank (this
        rank's row and column of the count matrix, redist.py:199's alltoall;
        ``exchange.count_skew`` turns the gathered matrix into the load
        imbalance).  None before the first call."""
        lay = getattr(self, "_last_layout", None)
        return None if lay is None else (lay.send_counts.copy(), lay.recv_counts.copy())

    @property
    def last_traffic(self):
        """Off-rank bytes of the last redistribution call on this rank
        (comm.Traffic.as_dict): sent to / received from every other rank,
        computed from the exchange's real layout -- every field's rows, side
        fields (fine cells, halo flags), count messages and the halo's
        messages included.  bench.py's xGMI figures come from it."""
        t = self.comm.traffic
        return t.as_dict() if t is not None else None

    # ------------------------------------------------------------ helpers
    def stack_position(self, xyz_list):
        """redist.py:311-312: columns -> (N, d)."""
        if all(isinstance(c, torch.Tensor) for c in xyz_list):
            return torch.stack(list(xyz_list), dim=1)
        return np.vstack(xyz_list).T

    def unstack_position(self, position):
        """Intended behaviour of redist.py:314-318 (which is broken): columns."""
        return [position[:, d] for d in range(self.dim)]

    @staticmethod
    def _check_host_alias(data, position):
        if (isinstance(data, torch.Tensor) and isinstance(position, torch.Tensor)
                and not data.is_cuda and not position.is_cuda
                and data.untyped_storage().data_ptr() == position.untyped_storage().data_ptr()):
            raise NotImplementedError("CPU torch tensors where position aliases data: pass "
                                      "GPU tensors or numpy arrays")

    def _like(self, ref, t):
        """Return ``t`` (device tensor) in the container type of ``ref``."""
        if isinstance(ref, torch.Tensor):
            return t if ref.is_cuda else t.to(ref.device)
        return t.cpu().numpy()


def mpi_grid_redistribute(data, pos, grid_topology, box_lengths, comm, overload_lengths=None,
                          periodic=True):
    """redist.py:11-13 with its intended behaviour (the reference calls a
    misspelled method and always raises AttributeError, S13)."""
    redist = MPIGridRedistributor(comm, grid_topology, box_lengths)
    return redist.redistribute_by_position(data, pos, overload_lengths=overload_lengths,
                                           periodic=periodic)


__all__ = ["MPIGridRedistributor", "GridPartitioner", "Route", "mpi_grid_redistribute",
           "SelfComm"]
