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
from ._arrays import Positions, Rows, box_dtype_code, device, id_array, pos_code
from .comm import SelfComm, as_transport
from .exchange import (check_counts, exchange, exchange_back, exchange_pipelined, host_read_start,
                       host_read_wait)
from .halo import (DeviceSelect, HaloRoute, exchange_overload, halo_capacity, reduce_overload,
                   thresholds)


_WRITE_BACK = {"changed": _lib.MGR_WRITE_BACK_CHANGED, "all": _lib.MGR_WRITE_BACK_ALL}
_TORCH_POS = {_lib.MGR_F32: torch.float32, _lib.MGR_F64: torch.float64}


class _Plan:
    """Owns one native mgr_plan (geometry + number of destinations), or with
    ``fine`` a fine-cell plan (mgr_plan_create_fine, prod(fine) bins)."""

    def set_write_back(self, mode):
        if mode not in _WRITE_BACK:
            raise ValueError(f"write_back must be one of {sorted(_WRITE_BACK)} (got {mode!r})")
        _lib.call("mgr_plan_set_write_back", self.h, _WRITE_BACK[mode])

    def __init__(self, grid_topology: np.ndarray, box_length: np.ndarray, nbins: int,
                 fine=None):
        topo = np.ascontiguousarray(grid_topology.astype(np.int64))
        box = np.ascontiguousarray(box_length.astype(np.float64))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        h = ctypes.c_void_p()
        if fine is None:
            _lib.call("mgr_plan_create", len(topo), vp(topo), vp(box),
                      box_dtype_code(box_length), int(nbins), ctypes.byref(h))
        else:
            fn = np.ascontiguousarray(np.asarray(fine).astype(np.int64))
            _lib.call("mgr_plan_create_fine", len(topo), vp(topo), vp(fn), vp(box),
                      box_dtype_code(box_length), ctypes.byref(h))
            nbins = int(np.prod(fn))
        self.h = h
        self.nbins = int(nbins)
        self.dim = len(topo)

    def __del__(self):
        try:
            if self.h:
                _lib.load().mgr_plan_destroy(self.h)
        except Exception:
            pass


def _as_ids(fine_ids, n, dev, nbins):
    """uint16 device ids of n rows (torch int16/uint16 tensor or numpy array),
    every id < nbins.  Host ids are range-checked before the cast (a negative
    or >= 65536 id would wrap); device ids are checked by the kernels
    (mgr_rank_ids / mgr_count_ids clamp them and flag the call, whose counts
    then read -1)."""
    if isinstance(fine_ids, torch.Tensor):
        t = fine_ids
        if t.dtype not in (torch.int16, torch.uint16):
            raise TypeError(f"fine_ids must be 16-bit (got {t.dtype})")
        t = t.to(dev).contiguous().reshape(-1)   # range: flagged by the kernels
    else:
        a = np.asarray(fine_ids).reshape(-1)
        if a.dtype.kind not in "iu":
            raise TypeError(f"fine_ids must be integers (got {a.dtype})")
        if a.size and (int(a.min()) < 0 or int(a.max()) >= nbins):
            raise ValueError(f"fine_ids out of range [0, {nbins})")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.uint16)).view(np.int16)).to(dev)
    if t.numel() != n:
        raise ValueError(f"fine_ids has {t.numel()} entries for {n} rows")
    return t


class SortRoute:
    """What ``unsort`` / ``return_to_source(..., sort_route=)`` need to bring
    per-row results out of fine-cell order (``fine_cell_sort(...,
    return_route=True)``): for the ranked sort (<= 1024 fine cells, sorted
    fields of 4-byte multiples <= 64 B) the rows' ids, their ranks, the tiles'
    cell starts and the workspace as mgr_rank_ids + mgr_scan left them -- the
    inverse is one mgr_unpack_ranked_fields launch; for the other sorts the
    destination bytes and workspace of mgr_count_ids + mgr_scan -- the inverse
    is mgr_unpack_fields (bin = id, no drop bin, no redirect).  Buffers that
    came from a Scratch are TAKEN OUT of it (the next call allocates anew),
    fresh ones are kept; ids the caller's device tensor would alias are copied
    (2 B/row), so later calls and the caller's writes leave a live route
    alone, and it may be used any number of times.  Memory per live route,
    ranked: about 4 B/row (ids + ranks) + 2 * T * nbins (T = ceil(n /
    tile_rows)) + mgr_workspace_bytes(n, nbins, tile_rows); else 1-2 B/row +
    the workspace.  Freed by ``release()``."""

    def __init__(self, n, nbins, tile_rows, ws, ids=None, ranks=None, tile_starts=None, dest=None):
        self.n, self.nbins, self.tile_rows = int(n), int(nbins), int(tile_rows)
        self.ranked = dest is None
        self._ws, self._ids, self._ranks, self._tstarts, self._dest = (ws, ids, ranks,
                                                                        tile_starts, dest)

    @property
    def released(self):
        return self._ws is None

    def release(self):
        """Free the route's device memory; it cannot be used afterwards."""
        self._ws = self._ids = self._ranks = self._tstarts = self._dest = None


def _unsort_into(sroute, srcs, rbs, outs):
    """outs[f][r] = srcs[f][slot(r)] for the sort that made ``sroute``: flat
    device tensors of sroute.n rows of rbs[f] bytes; one launch."""
    n, s = sroute.n, _lib.stream_handle()
    if n == 0:
        return
    if sroute.ranked:
        _lib.call("mgr_unpack_ranked_fields", len(rbs), _ptrs([t.data_ptr() for t in srcs]),
                  _i64s(rbs), n, _lib.ptr(sroute._ids), _lib.ptr(sroute._ranks),
                  _lib.ptr(sroute._tstarts), sroute.nbins, sroute.tile_rows,
                  _lib.ptr(sroute._ws), _ptrs([t.data_ptr() for t in outs]), s)
    else:
        _lib.call("mgr_unpack_fields", len(rbs), _ptrs([t.data_ptr() for t in srcs]), _i64s(rbs),
                  n, _lib.ptr(sroute._dest), sroute.nbins, -1, sroute.tile_rows,
                  _lib.ptr(sroute._ws), _ptrs([t.data_ptr() for t in outs]), -1, None, 0, -1, s)


def _check_sort_route(sort_route):
    if not isinstance(sort_route, SortRoute):
        raise TypeError("sort_route: a SortRoute of fine_cell_sort(..., return_route=True)")
    if sort_route.released:
        raise ValueError("the sort route was released")


def _sort_by_ids(fields, ids, n, nb, dev, scratch=None, check_ids=True, route=False):
    """Stable sort of every field by the uint16 ids (the fine cells): rank
    (mgr_rank_ids) or count (mgr_count_ids) -> scan -> pack.  Returns ([sorted
    flat fields], counts).  ``check_ids``: ids from the caller (not from this
    library's binning) -- an id >= nb is clamped by the kernels and turns the
    counts into -1 (the failed-scan convention: host results raise).
    ``route``: ([sorted], counts, SortRoute) -- the sort's buffers leave the
    scratch and ``ids`` is kept, so the caller passes ids it owns."""
    hint = max([f.row_bytes for f in fields] + [1])
    s = _lib.stream_handle()
    counts = torch.empty(nb, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if check_ids else None
    # <= 1024 fine cells, 4-byte-multiple rows <= 64 B on 4-byte-aligned
    # storage: ranks computed once, the ranked pack only places rows
    # (mgr_rank_ids + mgr_pack_ranked), on its own tiles (mgr_ranked_tile_rows);
    # other rows: count + scan + the generic stable pack
    rtr = int(_lib.load().mgr_ranked_tile_rows(int(hint), int(nb)))
    ranked = (rtr > 0 and all(f.row_bytes % 4 == 0 and f.row_bytes <= 64
                              and f.flat.data_ptr() % 4 == 0 for f in fields))
    tile_rows, ws, dest = _scratch(n, nb, hint, dev, scratch, dest=not ranked,
                                   tag="_fine", tile_rows=rtr if ranked else None)
    outs = []
    if ranked:
        T = (n + tile_rows - 1) // tile_rows
        get = scratch.get if scratch is not None else (
            lambda name, nbytes: torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev))
        # tile slots (+ 16 B: the ranked pack reads u16 quads, the last one
        # a row past n when n is odd)
        ranks = get("ranks_fine", 2 * max(n, 1) + 16)
        tstarts = get("tstarts_fine", 8 * max(T * nb, 1))   # u16 starts, or u32 x 2 halves
        _lib.call("mgr_rank_ids", _lib.ptr(ids), n, nb, tile_rows, _lib.ptr(ranks),
                  _lib.ptr(tstarts), _lib.ptr(bad), _lib.ptr(ws), s)
        _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(ws), _lib.ptr(counts), s)
        for f in fields:
            o = torch.empty(max(n * f.row_bytes, 1), dtype=torch.uint8, device=dev)
            _lib.call("mgr_pack_ranked", _lib.ptr(f.flat), f.row_bytes, n, _lib.ptr(ids),
                      _lib.ptr(ranks), _lib.ptr(tstarts), nb, tile_rows, _lib.ptr(ws),
                      _lib.ptr(o), s)
            outs.append(o)
    else:
        _lib.call("mgr_count_ids", _lib.ptr(ids), n, nb, tile_rows, _lib.ptr(dest),
                  _lib.ptr(bad), _lib.ptr(ws), s)
        _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(ws), _lib.ptr(counts), s)
        for f in fields:
            o = torch.empty(max(n * f.row_bytes, 1), dtype=torch.uint8, device=dev)
            _lib.call("mgr_pack", _lib.ptr(f.flat), f.row_bytes, n, _lib.ptr(dest), nb, -1,
                      tile_rows, _lib.ptr(ws), _lib.ptr(o), -1, None, s)
            outs.append(o)
    if bad is not None:
        counts.masked_fill_(bad.ne(0), -1)
    if not route:
        return outs, counts
    if scratch is not None:   # the route owns them: the next sort allocates anew
        for name in ("ws_fine", "dest_fine", "ranks_fine", "tstarts_fine"):
            scratch.take(name)
    if ranked:
        sroute = SortRoute(n, nb, tile_rows, ws, ids=ids, ranks=ranks, tile_starts=tstarts)
    else:
        sroute = SortRoute(n, nb, tile_rows, ws, dest=dest)
    return outs, counts, sroute


def _payload(data, dev):
    """The payload of a call as a list of fields (Rows): one array, or --
    SoA -- a tuple / list of arrays sharing axis 0 (positions, velocities,
    masses, ids ...), each of any dtype and trailing shape, moved with the
    same destinations (redist.py:160-164 redistributes ``position`` with the
    ``rank_to_send`` computed for ``data``: the reference's multi-field
    pattern).  Returns (fields, multi)."""
    if isinstance(data, (tuple, list)):
        if not data:
            raise ValueError("data: an empty sequence of fields")
        if len(data) > MAX_FIELDS:
            raise ValueError(f"data: at most {MAX_FIELDS} fields (got {len(data)})")
        fields = [Rows(d, dev) for d in data]
        for i, f in enumerate(fields[1:], 1):
            if f.n != fields[0].n:
                raise ValueError(f"data field {i} has {f.n} rows, field 0 has {fields[0].n}")
        return fields, True
    return [Rows(data, dev)], False


def _alias_rows(position, fields):
    """The numpy payload field ``position`` shares memory with (the wrap then
    writes into that field's device copy, Positions), else None."""
    if not isinstance(position, np.ndarray):
        return None
    for f in fields:
        if f.kind == "numpy" and f.n and np.shares_memory(position, f.host):
            return f
    return fields[0] if len(fields) == 1 else None


def _pos_field(addrs, row_bytes, pos_addr, pos_stride_bytes, esz):
    """(field, byte offset) when three coordinates at ``pos_addr`` lie inside the
    first row of one of the fields at ``addrs`` and step by that field's row
    bytes -- the positions are that field, or a strided view inside it --
    else (-1, 0)."""
    for f, (a, rb) in enumerate(zip(addrs, row_bytes)):
        o = pos_addr - a
        if 0 <= o and o + 3 * esz <= rb and pos_stride_bytes == rb:
            return f, o
    return -1, 0


def _results(fields, outs, m, multi):
    """Outputs of m rows in the caller's containers: one array, or a tuple in
    the order of the fields."""
    res = tuple(f.wrap(o, m) for f, o in zip(fields, outs))
    return res if multi else res[0]


MAX_FIELDS = _lib.MAX_FIELDS   # mgr.h MGR_MAX_FIELDS


# The row size the tile policy sizes multi-field packs for: the cooperative
# pack's 32-byte rows (512-row tiles up to 16 bins, 1024 up to 64).  A/B,
# round 6, config 5's four arrays at 64M rows (profiles/round6/soa_ab.json):
# 1.25 ms at 512-row tiles against 1.39 / 1.39 ms at 256 / 1024 (the LDS-image
# kernel: 1.38-1.44 ms at 512-2048).
_FIELDS_TILE_HINT = 32


def _tile_hint(row_bytes, side=None):
    """The row size the tile policy (mgr_tile_rows) sizes tiles for: one
    field's row bytes, or _FIELDS_TILE_HINT when several fields move together
    through the multi-field kernels; a 2-byte side field (index ``side``)
    rides along and does not count."""
    rb = [int(b) for i, b in enumerate(row_bytes) if i != side]
    return _FIELDS_TILE_HINT if len(rb) > 1 else max(rb + [1])


def _ptrs(addrs):
    """A C array of device addresses (void* const*)."""
    return (ctypes.c_void_p * len(addrs))(*[int(a) for a in addrs])


def _i64s(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _offsets_like(data, counts, dev):
    """offsets[nb+1] from device counts, in the container of ``data``; host
    results are checked for a failed scan (-1 counts) at the copy, device
    results stay asynchronous."""
    nb = counts.numel()
    offsets = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    if isinstance(data, torch.Tensor) and data.is_cuda:
        return offsets
    check_counts(counts.cpu().numpy(), [])
    return offsets.cpu() if isinstance(data, torch.Tensor) else offsets.cpu().numpy()


GHOST_MAX_CELLS = 1024   # the ranked sort's bound (mgr_rank_ids + mgr_pack_ranked)


def ghost_grid(cell_length, cell_limits, fine_cells, overload_lengths):
    """The extended fine grid of a rank's cell with ghost layers -- the single
    definition ``MPIGridRedistributor.ghost_grid`` / ``ghost_cell_sort`` and
    mgr_ghost_cells share (host numpy, no GPU).  ``cell_length[d]`` and
    ``cell_limits[d] = (low, high)`` describe the cell.  Returns (ghost,
    extents, origin, width):

      width[d]   = cell_length[d] / fine_cells[d]              (float64)
      ghost[d]   = ceil(overload_lengths[d] / width[d]), 0 for a zero length
      extents[d] = fine_cells[d] + 2 * ghost[d]
      origin[d]  = cell_limits[d, 0]

    Cell k of dimension d covers [origin + (k - ghost) * width, origin + (k -
    ghost + 1) * width); cells ghost .. ghost + fine - 1 are the rank's own.
    ValueError: prod(extents) beyond 1024 cells, a fine cell count < 1, a
    negative or non-finite overload length."""
    cl = np.asarray(cell_length, dtype=np.float64)
    fine = np.array(fine_cells).astype(np.int64)
    ol = np.asarray(overload_lengths, dtype=np.float64)
    dim = len(cl)
    if fine.ndim != 1 or len(fine) != dim or ol.ndim != 1 or len(ol) != dim:
        raise ValueError(f"fine_cells and overload_lengths must have {dim} entries")
    if (fine < 1).any():
        raise ValueError(f"fine_cells {fine.tolist()}: at least 1 per dimension")
    if not np.isfinite(ol).all() or (ol < 0).any():
        raise ValueError(f"overload_lengths {ol.tolist()}: finite and >= 0")
    width = cl / fine
    if not np.isfinite(width).all() or (width <= 0).any():
        raise ValueError(f"cell lengths {cl.tolist()}: positive and finite")
    ghost = np.where(ol == 0, 0.0, np.ceil(ol / width))
    if (ghost > GHOST_MAX_CELLS).any():
        raise ValueError(f"ghost layers of {ghost.tolist()} cells: beyond {GHOST_MAX_CELLS}")
    ghost = ghost.astype(np.int64)
    extents = fine + 2 * ghost
    cells = 1
    for e in extents:
        cells *= int(e)
    if cells > GHOST_MAX_CELLS:
        raise ValueError(f"extended grid {extents.tolist()} has {cells} cells: at "
                         f"most {GHOST_MAX_CELLS} (the ranked sort's bound); use fewer fine cells")
    origin = np.ascontiguousarray(np.asarray(cell_limits, dtype=np.float64)[:, 0])
    return ghost, extents, origin, width


def _fine_sort(plan, coarse, dim, dev, data, position, return_positions, fine_ids=None,
               return_route=False):
    """The fine cells of the rows -- ``fine_ids`` as given (computed at the
    source), else one read of the positions (mgr_bin_count_fine against the
    coarse plan, periodic=0: no wrap, no write-back; the fine cell is the fine
    plan's binning by construction, mgr_device.h bin_coord) -- then the
    stable sort by them (_sort_by_ids).  ``return_route``: the SortRoute of
    the sort is appended to the result."""
    rows, multi = _payload(data, dev)
    pos = Positions(position, dim, dev, data_rows=_alias_rows(position, rows))
    if pos.n != rows[0].n:
        raise ValueError(f"data has {rows[0].n} rows, position has {pos.n}")
    n, nb = rows[0].n, plan.nbins
    prow = Rows(position, dev) if return_positions else None
    fields = rows + ([prow] if prow else [])
    check = fine_ids is not None
    if fine_ids is None:
        ids = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        hint = max(f.row_bytes for f in fields)
        tile_rows, ws, dest = _scratch(n, coarse.nbins, hint, dev)
        _lib.call("mgr_bin_count_fine", coarse.h, plan.h, ctypes.c_void_p(pos.addr), pos.code, n,
                  pos.stride, 0, _lib.ptr(dest), _lib.ptr(ids), tile_rows, _lib.ptr(ws),
                  _lib.stream_handle())
        ids = ids[:n]
    else:
        ids = _as_ids(fine_ids, n, dev, nb)
        if (return_route and isinstance(fine_ids, torch.Tensor) and n
                and ids.untyped_storage().data_ptr() == fine_ids.untyped_storage().data_ptr()):
            ids = ids.clone()   # the caller's tensor: the route keeps its own copy
    sroute = None
    if return_route:
        outs, counts, sroute = _sort_by_ids(fields, ids, n, nb, dev, check_ids=check, route=True)
    else:
        outs, counts = _sort_by_ids(fields, ids, n, nb, dev, check_ids=check)
    nd = len(rows)
    res = [_results(rows, outs[:nd], n, multi)]
    if prow:
        res.append(prow.wrap(outs[nd], n))
    res.append(_offsets_like(rows[0].obj, counts, dev))
    return tuple(res) + ((sroute,) if return_route else ())


class _IdField:
    """A 2-byte-row field of n rows: the fine cells travelling with the rows."""

    row_bytes = 2

    def __init__(self, flat):
        self.flat = flat


class Scratch:
    """Reusable device buffers of one redistributor (workspace, destination
    bytes, send buffers): grown geometrically, never shrunk, so repeated
    calls with varying sizes (skewed counts) stop allocating after the first
    few.  Buffers are kept per CUDA stream (the current stream at the call):
    calls on one stream run in order and reuse them safely; a call on another
    stream gets buffers of its own, so calls overlapping on two streams never
    share a workspace or a send buffer.  Memory: one full set per stream used,
    for at most MAX_STREAMS streams -- a call on a further stream first waits
    for the least recently used stream and frees its set."""

    GROWTH = 1.25
    MAX_STREAMS = 4

    def __init__(self, dev):
        self.dev = dev
        self.bufs = {}
        self.streams = {}          # stream handle -> torch stream, least recently used first

    def _stream_key(self):
        st = torch.cuda.current_stream(self.dev)
        key = st.cuda_stream
        if key in self.streams:
            self.streams[key] = self.streams.pop(key)     # most recently used last
            return key
        while len(self.streams) >= self.MAX_STREAMS:
            old_key, old = next(iter(self.streams.items()))
            old.synchronize()                             # its calls are done with the set
            del self.streams[old_key]
            for k in [k for k in self.bufs if k[1] == old_key]:
                del self.bufs[k]
        self.streams[key] = st
        return key

    def get(self, name, nbytes):
        nbytes = max(int(nbytes), 1)
        key = (name, self._stream_key())
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None:
                nbytes = max(nbytes, int(b.numel() * self.GROWTH))
            del b
            self.bufs.pop(key, None)
            b = self.bufs[key] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return b

    def take(self, name):
        """Remove and return the current stream's buffer ``name`` (None if there
        is none): the caller owns it, and the next get() allocates anew."""
        return self.bufs.pop((name, self._stream_key()), None)

    def release(self):
        self.bufs.clear()
        self.streams.clear()


def _scratch(n, nbins, max_row_bytes, dev, cache=None, dest=True, tag="", tile_rows=None):
    """(tile_rows, workspace, dest) for n rows and nbins bins; from ``cache``
    (a Scratch, buffers named with ``tag``) when given, else fresh.
    ``tile_rows``: a kernel family's own tiles (default mgr_tile_rows)."""
    if tile_rows is None:
        tile_rows = _lib.load().mgr_tile_rows(int(max_row_bytes), int(nbins))
    wsb = _lib.load().mgr_workspace_bytes(int(n), int(nbins), int(tile_rows))
    if wsb < 0:
        raise _lib.MgrError("mgr_workspace_bytes: bad arguments")
    db = max(int(n), 1) * _lib.load().mgr_dest_bytes(int(nbins))
    if cache is not None:
        return (tile_rows, cache.get("ws" + tag, wsb),
                cache.get("dest" + tag, db) if dest else None)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=dev)
    d = torch.empty(db, dtype=torch.uint8, device=dev) if dest else None
    return tile_rows, ws, d


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


class MPIGridRedistributor:
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
        nd = len(fields)
        run_fields = list(fields) + ([None] if return_positions else [])

        def binner(dest, tile_rows, ws):
            _lib.call("mgr_bin_count", self._plan.h, ctypes.c_void_p(pos.addr), pos.code, pos.n,
                      pos.stride, int(bool(periodic)), _lib.ptr(dest), tile_rows, _lib.ptr(ws),
                      _lib.stream_handle())
            pos.finish()
            if return_positions:  # the wrapped positions, full rows
                run_fields[nd] = Rows(position, self._dev)

        row_bytes_hint = [f.row_bytes for f in fields]
        if return_positions:
            row_bytes_hint.append(self._pos_row_bytes(position, pos))
        outs, m = self._run(run_fields, binner, n, drop=False, row_bytes_hint=row_bytes_hint)
        res = _results(fields, outs[:nd], m, multi)
        if return_positions:
            res = res, run_fields[nd].wrap(outs[nd], m)
        return (res, self._take_route()) if return_route else res

    def _take_route(self):
        """The Route of the _run just made: its destination bytes and
        workspace leave the scratch (Route)."""
        tile_rows, nb, drop_bin, n = self._last_run
        ws, dest = self._scratch.take("ws"), self._scratch.take("dest")
        return Route(self, dest, ws, tile_rows, nb, drop_bin, n, self._last_layout)

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
            _lib.call("mgr_unpack_fields", len(rbs), _ptrs([s.data_ptr() for s in stagings]),
                      _i64s(rbs), n, _lib.ptr(route._dest), route.nbins, route.drop_bin,
                      route.tile_rows, _lib.ptr(route._ws), _ptrs([t.data_ptr() for t in outs]),
                      redirect_bin, _ptrs(reds) if redirect_bin >= 0 else None, 0, -1, stream)
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
        fields = [rows] + ([] if one else [_IdField(flags_src)]) + ([None] if rp else [])
        ip = len(fields) - 1                                 # the positions' field
        cl = np.ascontiguousarray(self.cell_length, dtype=np.float64)
        ol = np.ascontiguousarray(np.asarray(overload_lengths, dtype=np.float64))

        def binner(dest, tile_rows, ws):
            _lib.call("mgr_bin_count_halo", self._plan.h, ctypes.c_void_p(pos.addr), pos.code,
                      pos.n, pos.stride, int(bool(periodic)), _lib.ptr(dest), _lib.ptr(flags_src),
                      cl.ctypes.data_as(ctypes.c_void_p), ol.ctypes.data_as(ctypes.c_void_p),
                      tile_rows, _lib.ptr(ws), _lib.stream_handle())
            pos.finish()
            if rp:   # redist.py:164: the wrapped positions travel with the rows
                fields[ip] = Rows(position, self._dev)

        hint = ([rows.row_bytes] + ([] if one else [2])
                + ([self._pos_row_bytes(position, pos)] if rp else []))
        extra = lambda m_: halo_capacity(self, m_, overload_lengths)  # noqa: E731
        pending = []   # one rank: the scan's counts checked at the halo's host read
        outs, m = self._run(fields, binner, rows.n, drop=False, row_bytes_hint=hint,
                            extra_rows=extra, side=None if one else 1, deferred=pending)
        rbd = rows.row_bytes
        rbp = fields[ip].row_bytes if rp else 0
        cap = outs[0].numel() // max(rbd, 1) - m
        fsrc = flags_src if one else outs[1]
        flags = fsrc[: 2 * m].view(torch.int16) if m else torch.empty(
            0, dtype=torch.int16, device=self._dev)
        op = outs[ip] if rp else None
        route = None
        if return_route:   # before the halo: its selections reuse scratch names
            route = self._take_route()
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
            res = res, fields[ip].wrap(res_p, m + mo)
        return (res, route) if return_route else res

    def _fine_plan(self, fine_cells):
        fine = np.array(fine_cells).astype(np.int64)
        if fine.ndim != 1 or len(fine) != self.dim:
            raise ValueError(f"fine_cells must have {self.dim} entries")
        key = tuple(int(x) for x in fine)
        plan = self._fine_plans.get(key)
        if plan is None:
            plan = self._fine_plans[key] = _Plan(self.grid_topology, self.box_length, 0,
                                                 fine=fine)
        return plan

    def _redistribute_fine(self, data, position, fields, multi, pos, periodic, fine_cells,
                           return_positions):
        """Source: bin + fine cell of every row (mgr_bin_count_fine), the
        fine cells packed and exchanged as a 2-byte side field beside the
        payload's fields; destination: rank -> scan -> pack of every field by
        the received fine cells."""
        fplan = self._fine_plan(fine_cells)
        n = fields[0].n
        nd = len(fields)
        fids = self._scratch.get("fine_src", max(n, 1) * 2)
        run_fields = list(fields) + [_IdField(fids)] + ([None] if return_positions else [])

        def binner(dest, tile_rows, ws):
            _lib.call("mgr_bin_count_fine", self._plan.h, fplan.h, ctypes.c_void_p(pos.addr),
                      pos.code, pos.n, pos.stride, int(bool(periodic)), _lib.ptr(dest),
                      _lib.ptr(fids), tile_rows, _lib.ptr(ws), _lib.stream_handle())
            pos.finish()
            if return_positions:
                run_fields[nd + 1] = Rows(position, self._dev)

        hint = [f.row_bytes for f in fields] + [2]
        if return_positions:
            hint.append(self._pos_row_bytes(position, pos))
        outs, m = self._run(run_fields, binner, n, drop=False, row_bytes_hint=hint, side=nd)
        ids = outs[nd][: 2 * m].view(torch.int16) if m else torch.empty(0, dtype=torch.int16,
                                                                         device=self._dev)
        sort = [i for i in range(len(run_fields)) if i != nd]
        recv = []
        for i in sort:
            r = _IdField(outs[i])
            r.row_bytes = run_fields[i].row_bytes
            recv.append(r)
        sorted_, counts = _sort_by_ids(recv, ids, m, fplan.nbins, self._dev, self._scratch,
                                       check_ids=False)   # binned here: in range
        res = [_results(fields, sorted_[:nd], m, multi)]
        if return_positions:
            res.append(run_fields[nd + 1].wrap(sorted_[nd], m))
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
        plan = self._fine_plan(fine_cells)
        return _fine_sort(plan, self._plan, self.dim, self._dev, data, position,
                          return_positions, fine_ids, return_route)

    def ghost_grid(self, fine_cells, overload_lengths):
        """(ghost, extents, origin, width) of this rank's extended fine grid
        (host numpy; the module's ``ghost_grid`` on this rank's cell): width =
        cell_length / fine_cells, ghost[d] = ceil(overload_lengths[d] /
        width[d]) layers on either side, extents = fine_cells + 2 * ghost,
        origin = the cell's lower corner.  ValueError beyond 1024 cells."""
        return ghost_grid(self.cell_length, self.rank_cell_limits, fine_cells, overload_lengths)

    def ghost_cell_sort(self, data, position, n_local, fine_cells, overload_lengths,
                        return_positions=False, return_route=False):
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
        then the ranked sort of fine_cell_sort (_sort_by_ids), unchanged."""
        ghost, ext, origin, width = self.ghost_grid(fine_cells, overload_lengths)
        dev = self._dev
        rows, multi = _payload(data, dev)
        pos = Positions(position, self.dim, dev, data_rows=_alias_rows(position, rows))
        if pos.code not in _TORCH_POS:
            raise TypeError("ghost_cell_sort: float32 or float64 positions")
        n = rows[0].n
        if pos.n != n:
            raise ValueError(f"data has {n} rows, position has {pos.n}")
        n_local = int(n_local)
        if not 0 <= n_local <= n:
            raise ValueError(f"n_local {n_local} outside 0..{n}")
        nb = int(np.prod(ext))
        prow = Rows(position, dev) if return_positions else None
        fields = rows + ([prow] if prow else [])
        ids = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        outside = torch.zeros(1, dtype=torch.int32, device=dev)
        fine = np.array(fine_cells).astype(np.int64)
        _lib.call("mgr_ghost_cells", ctypes.c_void_p(pos.addr), pos.code, n, n_local, pos.stride,
                  self.dim, origin.ctypes.data_as(ctypes.c_void_p),
                  width.ctypes.data_as(ctypes.c_void_p),
                  (ctypes.c_int * self.dim)(*[int(x) for x in fine]),
                  (ctypes.c_int * self.dim)(*[int(x) for x in ghost]), _lib.ptr(ids),
                  _lib.ptr(outside), _lib.stream_handle())
        ids = ids[:n]
        sroute = None
        if return_route:
            outs, counts, sroute = _sort_by_ids(fields, ids, n, nb, dev, check_ids=False,
                                                route=True)
        else:
            outs, counts = _sort_by_ids(fields, ids, n, nb, dev, check_ids=False)
        counts.masked_fill_(outside.ne(0), -1)   # read with the offsets: no sync of its own
        nd = len(rows)
        res = [_results(rows, outs[:nd], n, multi)]
        if prow:
            res.append(prow.wrap(outs[nd], n))
        try:
            res.append(_offsets_like(rows[0].obj, counts, dev))
        except _lib.MgrError as e:
            raise _lib.MgrError("ghost_cell_sort: a halo row lies beyond the ghost layers (a "
                                "position that was not unwrapped or is NaN, or overload_lengths "
                                f"smaller than the halo's), or: {e}") from None
        return tuple(res) + ((sroute,) if return_route else ())

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

    @staticmethod
    def _pos_row_bytes(position, pos):
        return int(position.shape[1]) * _lib.POS_ITEMSIZE[pos.code]

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

        outs, m = self._run(fields, binner, n, drop=True)
        res = _results(fields, outs, m, multi)
        return (res, self._take_route()) if return_route else res

    def _run(self, fields, binner, n, drop, row_bytes_hint=None, extra_rows=None, side=None,
             deferred=None):
        """bin -> scan -> count exchange -> pack -> row exchange.  Every field
        (the payload's SoA fields, positions, side fields) is partitioned by
        the same destinations in one mgr_pack_fields call.  ``side``: the
        index of the rows' 2-byte side field (fine cells, halo flags), moved
        by the kernel that moves the other fields.  ``deferred`` (a
        list): on one rank without drops the counts are not read back; the
        scan's count tensor is appended to it for the caller's next host read
        to check."""
        P = self.size
        nb = P + 1 if drop else P
        hint = row_bytes_hint or [f.row_bytes for f in fields]
        tile_rows, ws, dest = _scratch(n, nb, _tile_hint(hint, side), self._dev,
                                       self._scratch)
        binner(dest, tile_rows, ws)
        self._last_run = (tile_rows, nb, P if drop else -1, n)
        stream = _lib.stream_handle()
        bin_counts = torch.empty(nb, dtype=torch.int64, device=self._dev)
        _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(ws), _lib.ptr(bin_counts), stream)

        # the rows' 2-byte side field travels inside the pack of the other
        # fields (one ranking for all of them)
        side_ids = side is not None
        side_i = side if side_ids else -1
        main = [f for f in range(len(fields)) if f != side_i]

        def pack_fields(sends, outs, redirect_bin, offs, t0=0, t1=-1):
            """Every field in ONE mgr_pack_fields call: one ranking of the
            destinations for all of them (the multi-field kernel where the
            fields allow); the redirect bin's rows straight into ``outs``."""
            r = redirect_bin >= 0
            _lib.call("mgr_pack_fields", len(main),
                      _ptrs([fields[f].flat.data_ptr() for f in main]),
                      _i64s([fields[f].row_bytes for f in main]), n, _lib.ptr(dest), nb,
                      P if drop else -1, tile_rows, _lib.ptr(ws),
                      _ptrs([sends[f].data_ptr() for f in main]), redirect_bin,
                      _ptrs([outs[f].data_ptr() + offs[f] for f in main]) if r else None,
                      _lib.ptr(fields[side_i].flat) if side_ids else None,
                      _lib.ptr(sends[side_i]) if side_ids else None,
                      ctypes.c_void_p(outs[side_i].data_ptr() + offs[side_i])
                      if side_ids and r else None, t0, t1, stream)

        T = (n + tile_rows - 1) // tile_rows
        # the chunk count is part of the exchange protocol: the same on every
        # rank whatever its row count (a rank with fewer tiles than chunks --
        # an empty one included -- packs empty chunks); the size rule reads
        # only rank-independent inputs
        k = (exchange_chunks_for(P, sum(hint)) if self.exchange_chunks is None
             else max(1, int(self.exchange_chunks)))
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
                pack_fields(sends, outs, redirect_bin, offs, bounds[c], bounds[c + 1])

            outs, lay = exchange_pipelined(self.comm, [f.row_bytes for f in fields],
                                           bin_counts[:P], self.rank, self._dev, chunk_offsets,
                                           pack_chunk, k, extra_rows=extra_rows,
                                           scratch=self._scratch.get)
            self._last_layout = lay
            return outs, lay.total_recv
        known, read = None, None
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
        outs, lay = exchange(self.comm, [f.row_bytes for f in fields], bin_counts[:P], self.rank,
                             self._dev, None, extra_rows=extra_rows, scratch=self._scratch.get,
                             pack_all=pack_fields, known_rows=known)
        if read is not None:
            check_counts(host_read_wait(read)[0], [])
        self._last_layout = lay
        return outs, lay.total_recv

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


class GridPartitioner:
    """The 1-GPU local stage (BASELINE config 2): bin + scan + stable pack of
    one payload into ``prod(grid_topology)`` virtual subdomains, no exchange.
    Output = concat_d data[dest == d] plus offsets[nbins+1], i.e. the
    reference's send_buff (redist.py:195-198) laid end to end."""

    def __init__(self, grid_topology, box_length):
        _lib.require_gpu()
        self.grid_topology = np.array(grid_topology).astype(np.int64)
        self.box_length = np.array(box_length)
        self.dim = len(self.grid_topology)
        assert self.dim == len(self.box_length)
        self.nbins = int(np.prod(self.grid_topology))
        self._plan = _Plan(self.grid_topology, self.box_length, self.nbins)
        self._dev = device()
        self._cache = {}
        self._fine_plans = {}
        self._fine_buf = None
        self.last_counts = None

    def set_write_back(self, mode):
        """"changed" (default) / "all": MPIGridRedistributor.set_write_back."""
        self._plan.set_write_back(mode)

    def buffers(self, n, row_bytes):
        key = (int(n), int(row_bytes))
        if key not in self._cache:
            tile_rows, ws, dest = _scratch(n, self.nbins, row_bytes, self._dev)
            out = torch.empty(max(n * row_bytes, 1), dtype=torch.uint8, device=self._dev)
            counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
            self._cache = {key: (tile_rows, ws, dest, out, counts)}
        return self._cache[key]

    def partition_device(self, data_flat, row_bytes, pos_tensor, periodic=True, stream=None,
                         fine_cells=None):
        """Hot-path call on device buffers (no host sync).  ``data_flat``:
        uint8 device tensor of n*row_bytes; ``pos_tensor``: (n, >=dim)
        device tensor of any position dtype, unit column stride (wrapped in
        place).  Returns (out_flat, bin_counts) device tensors; with
        ``fine_cells`` (config 5's source side) also every row's fine cell
        inside its destination cell, partitioned like the rows (uint16 ids
        for ``MPIGridRedistributor.fine_cell_sort(..., fine_ids=)``):
        (out_flat, fine_ids_out, bin_counts)."""
        n = int(pos_tensor.shape[0])
        tile_rows, ws, dest, out, counts = self.buffers(n, row_bytes)
        self._last_part = (int(n), int(row_bytes))
        self.last_counts = counts   # device bin counts of the last device call
        code = pos_code(pos_tensor.dtype)
        s = _lib.stream_handle(stream)
        if fine_cells is None:
            _lib.call("mgr_partition_by_position", self._plan.h, _lib.ptr(pos_tensor), code, n,
                      pos_tensor.stride(0), int(bool(periodic)), _lib.ptr(data_flat), row_bytes,
                      _lib.ptr(out), _lib.ptr(dest), _lib.ptr(counts), tile_rows, _lib.ptr(ws), s)
            return out, counts
        fplan = self._fine_plan(fine_cells)
        fid, fid_out = self.fine_buffers(n)
        _lib.call("mgr_bin_count_fine", self._plan.h, fplan.h, _lib.ptr(pos_tensor), code, n,
                  pos_tensor.stride(0), int(bool(periodic)), _lib.ptr(dest), _lib.ptr(fid),
                  tile_rows, _lib.ptr(ws), s)
        _lib.call("mgr_scan", n, self.nbins, tile_rows, _lib.ptr(ws), _lib.ptr(counts), s)
        _lib.call("mgr_pack_ids", _lib.ptr(data_flat), row_bytes, n, _lib.ptr(dest), self.nbins,
                  -1, tile_rows, _lib.ptr(ws), _lib.ptr(out), -1, None, _lib.ptr(fid),
                  _lib.ptr(fid_out), None, s)
        return out, fid_out.view(torch.int16)[:n], counts

    def fine_buffers(self, n):
        if self._fine_buf is None or self._fine_buf[0].numel() < 2 * max(n, 1):
            self._fine_buf = tuple(torch.empty(2 * max(n, 1), dtype=torch.uint8, device=self._dev)
                                   for _ in range(2))
        return self._fine_buf

    def partition_fields_device(self, flats, row_bytes, pos_tensor, periodic=True, stream=None,
                                fine_cells=None):
        """partition_device of a SoA payload: ``flats`` (uint8 device tensors
        of n * row_bytes[f] bytes each, e.g. positions, velocities, masses,
        ids) partitioned by ONE binning of ``pos_tensor`` (wrapped in place;
        it may itself be one of the fields' arrays) and one mgr_pack_fields
        launch.  Returns ([out_flat per field], bin_counts) device tensors, or
        with ``fine_cells`` ([out_flat ...], fine_ids_out, bin_counts)."""
        n = int(pos_tensor.shape[0])
        nf = len(flats)
        hint = _tile_hint(list(row_bytes))
        key = ("fields", n, tuple(int(b) for b in row_bytes))
        if key not in self._cache:
            tile_rows, ws, dest = _scratch(n, self.nbins, hint, self._dev)
            outs = [torch.empty(max(n * int(b), 1), dtype=torch.uint8, device=self._dev)
                    for b in row_bytes]
            counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
            self._cache = {key: (tile_rows, ws, dest, outs, counts)}
        tile_rows, ws, dest, outs, counts = self._cache[key]
        self._last_part = key
        self.last_counts = counts
        code = pos_code(pos_tensor.dtype)
        s = _lib.stream_handle(stream)
        fid = fid_out = None
        if fine_cells is None:
            _lib.call("mgr_bin_count", self._plan.h, _lib.ptr(pos_tensor), code, n,
                      pos_tensor.stride(0), int(bool(periodic)), _lib.ptr(dest), tile_rows,
                      _lib.ptr(ws), s)
        else:
            fplan = self._fine_plan(fine_cells)
            fid, fid_out = self.fine_buffers(n)
            _lib.call("mgr_bin_count_fine", self._plan.h, fplan.h, _lib.ptr(pos_tensor), code, n,
                      pos_tensor.stride(0), int(bool(periodic)), _lib.ptr(dest), _lib.ptr(fid),
                      tile_rows, _lib.ptr(ws), s)
        _lib.call("mgr_scan", n, self.nbins, tile_rows, _lib.ptr(ws), _lib.ptr(counts), s)
        _lib.call("mgr_pack_fields", nf, _ptrs([f.data_ptr() for f in flats]), _i64s(row_bytes),
                  n, _lib.ptr(dest), self.nbins, -1, tile_rows, _lib.ptr(ws),
                  _ptrs([o.data_ptr() for o in outs]), -1, None, _lib.ptr(fid),
                  _lib.ptr(fid_out), None, 0, -1, s)
        if fine_cells is None:
            return outs, counts
        return outs, fid_out.view(torch.int16)[:n], counts

    def unpartition_device(self, packed_flat, row_bytes, stream=None):
        """The return path of ``partition_device`` / ``partition_fields_device``
        (mgr_unpack): ``packed_flat`` (uint8 device tensor of n * row_bytes, any
        row size) holds one row per row of the last partition's OUTPUT order;
        returns out_flat, the same rows in the partition's INPUT order
        (out[r] = packed[slot(r)]).  Uses the destination bytes and workspace
        that partition call left in its cache: valid until the next partition
        call, RuntimeError before any.  The returned buffer is reused by the
        next call of the same shape."""
        return self.unpartition_fields_device([packed_flat], [row_bytes], stream)[0]

    def unpartition_fields_device(self, flats, row_bytes, stream=None):
        """``unpartition_device`` of a SoA set: one mgr_unpack_fields launch."""
        key = getattr(self, "_last_part", None)
        ent = self._cache.get(key) if key is not None else None
        if ent is None:
            raise RuntimeError("unpartition: no partition_device / partition_fields_device call "
                               "whose destination bytes and workspace are still cached")
        n = key[1] if key[0] == "fields" else key[0]
        tile_rows, ws, dest = ent[0], ent[1], ent[2]
        rbs = [int(b) for b in row_bytes]
        for t, rb in zip(flats, rbs):
            if t.numel() != n * rb:
                raise ValueError(f"a field of {t.numel()} bytes for {n} rows of {rb}")
        okey = (n, tuple(rbs))
        if getattr(self, "_unpart", (None,))[0] != okey:
            self._unpart = (okey, [torch.empty(max(n * rb, 1), dtype=torch.uint8,
                                               device=self._dev) for rb in rbs])
        outs = self._unpart[1]
        _lib.call("mgr_unpack_fields", len(rbs), _ptrs([t.data_ptr() for t in flats]), _i64s(rbs),
                  n, _lib.ptr(dest), self.nbins, -1, tile_rows, _lib.ptr(ws),
                  _ptrs([o.data_ptr() for o in outs]), -1, None, 0, -1, _lib.stream_handle(stream))
        return outs

    def _onepass_state(self, n, cap_rows, fine_cells, out_row_bytes, key_of):
        """What both one-pass entry points keep for the next call of the same
        shape: (cap, workspace, one output per entry of ``out_row_bytes``,
        fine ids or None, counts, fine plan or None).  ``cap_rows`` defaults
        to 1.25 x the mean + 4096 rows per bin region; ``key_of(cap)`` is the
        shape's key in the single-entry cache.  The counts become
        ``last_counts``."""
        cap = int(cap_rows) if cap_rows is not None else (5 * n) // (4 * self.nbins) + 4096
        key = key_of(cap)
        if key not in self._cache:
            wsb = _lib.load().mgr_onepass_workspace_bytes(n, self.nbins)
            ws = torch.empty(max(int(wsb), 8), dtype=torch.uint8, device=self._dev)
            outs = [torch.empty(max(self.nbins * cap * b, 1), dtype=torch.uint8, device=self._dev)
                    for b in out_row_bytes]
            fo = (torch.empty(max(self.nbins * cap, 1), dtype=torch.int16, device=self._dev)
                  if fine_cells is not None else None)
            counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
            self._cache = {key: (ws, outs, fo, counts)}
        ws, outs, fo, counts = self._cache[key]
        self.last_counts = counts
        fplan = self._fine_plan(fine_cells) if fine_cells is not None else None
        return cap, ws, outs, fo, counts, fplan

    def partition_onepass_device(self, data_flat, row_bytes, pos_tensor, periodic=True,
                                 stream=None, fine_cells=None, cap_rows=None):
        """The local stage in ONE read of the records (mgr_partition_onepass):
        ``pos_tensor`` is the (n, >= 3) float32 / float64 position view INSIDE
        the records of ``data_flat`` (uint8 device tensor of n * row_bytes, e.g.
        config 5's 36-byte records and their f32 positions, S9), wrapped in
        place.  The output is the reference's send_buff list (redist.py:195-
        198): bin b's rows, in order, from row b * cap of ``out`` (its fine
        cells from fine_out[b * cap]).  Returns (out, fine_out or None, counts,
        cap) device tensors without a host sync; a count above cap means the
        bin did not fit (the caller redoes the partition: partition_lists
        does), -1 counts a failed look-back.  ``cap_rows``: rows per bin region
        (default 1.25 x the mean + 4096).  MgrError (MGR_EUNSUPPORTED) for
        shapes the one-pass kernel does not take."""
        n = int(pos_tensor.shape[0])
        esz = pos_tensor.element_size()
        off = pos_tensor.data_ptr() - data_flat.data_ptr() if n else 0
        if n and (pos_tensor.stride(0) * esz != row_bytes or pos_tensor.stride(1) != 1
                  or off < 0 or off + 3 * esz > row_bytes):
            raise ValueError("pos_tensor must be the position view inside the records")
        cap, ws, (out,), fo, counts, fplan = self._onepass_state(
            n, cap_rows, fine_cells, [int(row_bytes)],
            lambda cap: ("onepass", n, int(row_bytes), cap, fine_cells is not None))
        _lib.call("mgr_partition_onepass", self._plan.h, fplan.h if fplan else None,
                  _lib.ptr(data_flat), int(row_bytes), int(off), pos_code(pos_tensor.dtype), n,
                  int(bool(periodic)), _lib.ptr(out), _lib.ptr(fo), cap, _lib.ptr(counts),
                  _lib.ptr(ws), _lib.stream_handle(stream))
        return out, fo, counts, cap

    def partition_onepass_fields_device(self, flats, row_bytes, pos_tensor, periodic=True,
                                        stream=None, fine_cells=None, cap_rows=None):
        """partition_onepass_device of a SoA payload
        (mgr_partition_onepass_fields): ``flats`` (uint8 device tensors of
        n * row_bytes[f] bytes each) are read ONCE, binned by ``pos_tensor`` --
        a device float32 / float64 (n, >= 3) tensor with unit column stride,
        wrapped in place -- and scattered into the send_buff list of every
        field: bin b's rows of field f, in order, from row b * cap of
        ``outs[f]`` (their fine cells from fine_out[b * cap]).  If
        ``pos_tensor`` lies inside one of ``flats`` with that field's row bytes
        as its row stride (the field itself, or a strided view inside a wider
        field), that field is the position field; otherwise the positions ride
        as an extra staged field without an output.  Returns (outs, fine_out
        or None, counts, cap) device tensors without a host sync; a count
        above cap means the bin did not fit (partition_lists redoes the
        partition), -1 counts a failed look-back (every count is then -1).
        ``cap_rows``: rows per bin region (default 1.25 x the mean + 4096).
        The outputs, counts and workspace are cached per (n, row bytes, cap,
        fine, position field) and REUSED by the next call of the same shape:
        a caller that keeps results across calls copies them.  MgrError
        (MGR_EUNSUPPORTED) for shapes the kernel does not take -- among them
        positions outside the fields whose n rows of stride(0) elements do not
        fit their tensor's storage (a column-offset view of a wider tensor)."""
        n = int(pos_tensor.shape[0])
        nf = len(flats)
        rbs = [int(b) for b in row_bytes]
        esz = pos_tensor.element_size()
        if pos_tensor.dim() != 2 or pos_tensor.shape[1] < 3 or (n and pos_tensor.stride(1) != 1):
            raise ValueError("pos_tensor must be (n, >= 3) with unit column stride")
        if nf < 1 or nf > MAX_FIELDS:
            raise ValueError(f"1..{MAX_FIELDS} fields (got {nf})")
        srcs = [t.data_ptr() for t in flats]
        pf, off = (_pos_field(srcs, rbs, pos_tensor.data_ptr(), pos_tensor.stride(0) * esz, esz)
                   if n else (-1, 0))
        extra = pf < 0
        if extra:   # the positions as one more staged field, not scattered
            if nf + 1 > MAX_FIELDS:
                raise ValueError(f"one-pass partition: at most {MAX_FIELDS - 1} fields when the "
                                 f"positions are staged as an extra field (got {nf})")
            prb = int(pos_tensor.stride(0)) * esz if n else 3 * esz
            # the kernel stages (and, wrapping, writes back) n whole rows of
            # stride(0) elements from the view's first element: they must lie
            # inside the tensor's storage -- a column-offset view of a wider
            # tensor (X[:, 4:7]) would run past X's end in its last row
            st = pos_tensor.untyped_storage()
            if n and pos_tensor.data_ptr() - st.data_ptr() + n * prb > st.nbytes():
                raise _lib.MgrError(
                    "mgr_partition_onepass_fields failed (-4): pos_tensor: a view whose last "
                    "row of stride(0) elements ends beyond its storage cannot be staged as a field")
            pf = nf
            srcs.append(pos_tensor.data_ptr())
            rbs.append(prb)
        cap, ws, outs, fo, counts, fplan = self._onepass_state(
            n, cap_rows, fine_cells, rbs[:nf],
            lambda cap: ("onepass_fields", n, tuple(rbs), cap, fine_cells is not None, pf, extra))
        _lib.call("mgr_partition_onepass_fields", self._plan.h, fplan.h if fplan else None,
                  len(srcs), _ptrs(srcs), _i64s(rbs), pf, int(off), pos_code(pos_tensor.dtype), n,
                  int(bool(periodic)), _ptrs([o.data_ptr() for o in outs] + [0] * extra),
                  _lib.ptr(fo), cap, _lib.ptr(counts), _lib.ptr(ws), _lib.stream_handle(stream))
        return outs, fo, counts, cap

    # partition_lists of a SoA payload: the one-pass kernel where it takes the
    # shape (True), or the two-pass bin + scan + pack for every shape (False).
    # Decided by the A/B of the two source sides on 64M config-5 rows
    # (tools/onepass_fields_ab.py, profiles/round7/onepass_fields_ab.json,
    # DESIGN.md §3.7): two-pass 1.51 ms, one-pass 1.64 ms -- the two-pass is
    # the default; the one-pass runs with this set on the partitioner, and
    # through partition_onepass_fields_device.
    soa_onepass = False

    def _two_pass_lists(self, fields, pos, periodic, fine_cells):
        """The send_buff lists by bin + scan + mgr_pack_fields over all fields
        (any shape): ([field][bin] flat byte slices of per-call buffers, the
        bins' fine-cell slices or None, host counts)."""
        n, nf, nb = fields[0].n, len(fields), self.nbins
        rbs = [f.row_bytes for f in fields]
        tile_rows, ws, dest = _scratch(n, nb, _tile_hint(rbs), self._dev)
        stream = _lib.stream_handle()
        cnt_d = torch.empty(nb, dtype=torch.int64, device=self._dev)
        fid = fido = None
        if fine_cells is None:
            _lib.call("mgr_bin_count", self._plan.h, ctypes.c_void_p(pos.addr), pos.code, n,
                      pos.stride, int(bool(periodic)), _lib.ptr(dest), tile_rows,
                      _lib.ptr(ws), stream)
        else:
            fid = torch.empty(max(n, 1), dtype=torch.int16, device=self._dev)
            fido = torch.empty(max(n, 1), dtype=torch.int16, device=self._dev)
            _lib.call("mgr_bin_count_fine", self._plan.h, self._fine_plan(fine_cells).h,
                      ctypes.c_void_p(pos.addr), pos.code, n, pos.stride, int(bool(periodic)),
                      _lib.ptr(dest), _lib.ptr(fid), tile_rows, _lib.ptr(ws), stream)
        pos.finish()
        _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(ws), _lib.ptr(cnt_d), stream)
        outs = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=self._dev) for rb in rbs]
        _lib.call("mgr_pack_fields", nf, _ptrs([f.flat.data_ptr() for f in fields]),
                  _i64s(rbs), n, _lib.ptr(dest), nb, -1, tile_rows, _lib.ptr(ws),
                  _ptrs([o.data_ptr() for o in outs]), -1, None, _lib.ptr(fid),
                  _lib.ptr(fido), None, 0, -1, stream)
        counts = cnt_d.cpu().numpy()
        check_counts(counts, [])
        st = np.concatenate([[0], np.cumsum(counts)])
        parts = [[outs[i][int(st[b]) * rbs[i]:int(st[b + 1]) * rbs[i]] for b in range(nb)]
                 for i in range(nf)]
        fparts = ([fido[int(st[b]):int(st[b + 1])] for b in range(nb)]
                  if fine_cells is not None else None)
        return parts, fparts, counts

    # "onepass" / "twopass": how the last SoA partition_lists call made its lists
    last_lists_path = None

    def _partition_lists_fields(self, data, position, periodic, fine_cells):
        """partition_lists of a tuple / list payload: per field the list of
        per-bin arrays (freshly allocated, never views of a cached buffer)."""
        fields, _ = _payload(data, self._dev)
        pos = Positions(position, self.dim, self._dev, data_rows=_alias_rows(position, fields))
        n, nf, nb = fields[0].n, len(fields), self.nbins
        if pos.n != n:
            raise ValueError("data and position row counts differ")
        rbs = [f.row_bytes for f in fields]
        esz = _lib.POS_ITEMSIZE[pos.code]
        cuda_out = fields[0].kind == "torch" and fields[0].out_device.type == "cuda"
        counts = None
        if (self.soa_onepass and n and self.dim == 3
                and pos.code in (_lib.MGR_F32, _lib.MGR_F64)):
            if pos.t is not None:
                pos_t = pos.t
            else:   # a numpy view of a field: the same view of the field's device bytes
                base = pos._alias_rows.flat.view(_TORCH_POS[pos.code])
                pos_t = torch.as_strided(
                    base, (n, 3), (pos.stride, 1),
                    (pos.addr - base.untyped_storage().data_ptr()) // esz)
            try:
                outs, fo, cnt_d, cap = self.partition_onepass_fields_device(
                    [f.flat for f in fields], rbs, pos_t, periodic, fine_cells=fine_cells)
                counts = cnt_d.cpu().numpy()
                pos.finish()
                check_counts(counts, [])
                if (counts > cap).any():
                    counts = None          # a bin outgrew its region: the two-pass path
                    periodic = False       # the positions are wrapped already (S2)
                else:
                    fresh = (lambda t: t.clone()) if cuda_out else (lambda t: t)
                    parts = [[fresh(outs[i][b * cap * rbs[i]:(b * cap + int(counts[b])) * rbs[i]])
                              for b in range(nb)] for i in range(nf)]
                    fparts = ([fresh(fo[b * cap:b * cap + int(counts[b])]) for b in range(nb)]
                              if fo is not None else None)
            except _lib.MgrError as e:
                if "(-4)" not in str(e):      # MGR_EUNSUPPORTED: the two-pass path
                    raise
        self.last_lists_path = "onepass"
        if counts is None:
            self.last_lists_path = "twopass"
            parts, fparts, counts = self._two_pass_lists(fields, pos, periodic, fine_cells)
        res = tuple([f.wrap(p, int(c)) for p, c in zip(parts[i], counts)]
                    for i, f in enumerate(fields))
        if fine_cells is None:
            return res
        if cuda_out:
            return res, fparts            # int16 tensors holding the uint16 cells
        return res, [f.cpu().numpy().view(np.uint16) for f in fparts]

    def partition_lists(self, data, position, periodic=True, fine_cells=None):
        """The reference's send_buff list (redist.py:195-198: send_buff[i] =
        data[rank_to_send == i], original order kept): one array per bin, in
        the container type of ``data``; ``position`` wrapped in place (S1).
        With ``fine_cells`` also every row's fine cell inside its bin's cell,
        as a second list (uint16).  Records holding their own float32 /
        float64 positions go through the one-pass kernel
        (partition_onepass_device: every record read once); any other shape,
        or a bin that outgrows its region, through the classic bin + scan +
        pack (a redo re-bins the stored, already wrapped positions with
        periodic = 0 -- identical bins, S2 -- so nothing is wrapped twice).
        ``data`` may be a tuple / list of arrays sharing axis 0 (SoA, at most
        MAX_FIELDS; with ``soa_onepass`` set one fewer when ``position`` is
        not one of them, as the one-pass kernel then stages it as a field): the
        result is then a tuple, in field order, of per-bin lists (with
        ``fine_cells``: (that tuple, fine list)), every array freshly
        allocated; the fields go through the multi-field one-pass kernel
        (partition_onepass_fields_device) where it takes the shape, else --
        or when a bin outgrows its region -- through bin + scan +
        mgr_pack_fields over all fields."""
        if isinstance(data, (tuple, list)):
            return self._partition_lists_fields(data, position, periodic, fine_cells)
        rows = Rows(data, self._dev)
        pos = Positions(position, self.dim, self._dev, data_rows=rows)
        n, rb = rows.n, rows.row_bytes
        if pos.n != n:
            raise ValueError("data and position row counts differ")
        counts = None
        onepass_pos = None
        if n and pos.code in (_lib.MGR_F32, _lib.MGR_F64) and self.dim == 3:
            esz = _lib.POS_ITEMSIZE[pos.code]
            off = pos.addr - rows.flat.data_ptr()
            if pos.stride * esz == rb and 0 <= off and off + 3 * esz <= rb and off % esz == 0:
                # the positions as a view of the records' device bytes
                base = rows.flat.view(_TORCH_POS[pos.code])
                onepass_pos = torch.as_strided(
                    base, (n, 3), (pos.stride, 1),
                    (pos.addr - base.untyped_storage().data_ptr()) // esz)
        if onepass_pos is not None:
            try:
                out, fo, cnt_d, cap = self.partition_onepass_device(
                    rows.flat, rb, onepass_pos, periodic, fine_cells=fine_cells)
                counts = cnt_d.cpu().numpy()
                pos.finish()
                check_counts(counts, [])
                if (counts > cap).any():
                    counts = None          # a bin outgrew its region: the classic path
                    periodic = False       # the positions are wrapped already (S2)
                else:
                    parts = [out[b * cap * rb:(b * cap + int(counts[b])) * rb]
                             for b in range(self.nbins)]
                    fparts = ([fo[b * cap:b * cap + int(counts[b])] for b in range(self.nbins)]
                              if fo is not None else None)
            except _lib.MgrError as e:
                if "(-4)" not in str(e):      # MGR_EUNSUPPORTED: the classic path
                    raise
        if counts is None:
            parts, fparts, counts = self._two_pass_lists([rows], pos, periodic, fine_cells)
            parts = parts[0]
        res = [rows.wrap(p, int(c)) for p, c in zip(parts, counts)]
        if fine_cells is None:
            return res
        if isinstance(data, torch.Tensor) and data.is_cuda:
            return res, fparts            # int16 tensors holding the uint16 cells
        return res, [f.cpu().numpy().view(np.uint16) for f in fparts]

    def _fine_plan(self, fine_cells):
        key = tuple(int(x) for x in fine_cells)
        if key not in self._fine_plans:
            self._fine_plans[key] = _Plan(self.grid_topology, self.box_length, 0,
                                          fine=np.array(key))
        return self._fine_plans[key]

    def partition_by_position(self, data, position, periodic=True):
        """Arrays in, (partitioned data, offsets[nbins+1]) out; position
        wrapped in place (S1).  Same container types as the inputs.  ``data``:
        one array, or a tuple / list of arrays sharing axis 0 (SoA: every
        field partitioned by the same destinations in one pack; the result is
        then a tuple in the same order)."""
        fields, multi = _payload(data, self._dev)
        pos = Positions(position, self.dim, self._dev, data_rows=_alias_rows(position, fields))
        n = fields[0].n
        if pos.n != n:
            raise ValueError("data and position row counts differ")
        rbs = [f.row_bytes for f in fields]
        tile_rows, ws, dest = _scratch(n, self.nbins, _tile_hint(rbs), self._dev)
        stream = _lib.stream_handle()
        counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
        _lib.call("mgr_bin_count", self._plan.h, ctypes.c_void_p(pos.addr), pos.code, n,
                  pos.stride, int(bool(periodic)), _lib.ptr(dest), tile_rows, _lib.ptr(ws), stream)
        pos.finish()
        _lib.call("mgr_scan", n, self.nbins, tile_rows, _lib.ptr(ws), _lib.ptr(counts), stream)
        outs = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=self._dev) for rb in rbs]
        _lib.call("mgr_pack_fields", len(fields), _ptrs([f.flat.data_ptr() for f in fields]),
                  _i64s(rbs), n, _lib.ptr(dest), self.nbins, -1, tile_rows, _lib.ptr(ws),
                  _ptrs([o.data_ptr() for o in outs]), -1, None, None, None, None, 0, -1, stream)
        offsets = torch.zeros(self.nbins + 1, dtype=torch.int64, device=self._dev)
        offsets[1:] = torch.cumsum(counts, 0)
        first = fields[0].obj
        if isinstance(first, torch.Tensor) and first.is_cuda:
            # device results stay asynchronous: a failed scan shows as -1 counts
            return _results(fields, outs, n, multi), offsets
        check_counts(counts.cpu().numpy(), [])   # a failed scan reports -1 counts
        res = _results(fields, outs, n, multi)
        if isinstance(first, torch.Tensor):
            return res, offsets.cpu()
        return res, offsets.cpu().numpy()


def mpi_grid_redistribute(data, pos, grid_topology, box_lengths, comm, overload_lengths=None,
                          periodic=True):
    """redist.py:11-13 with its intended behaviour (the reference calls a
    misspelled method and always raises AttributeError, S13)."""
    redist = MPIGridRedistributor(comm, grid_topology, box_lengths)
    return redist.redistribute_by_position(data, pos, overload_lengths=overload_lengths,
                                           periodic=periodic)


__all__ = ["MPIGridRedistributor", "GridPartitioner", "Route", "mpi_grid_redistribute",
           "SelfComm"]
