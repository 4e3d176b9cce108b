"""The stable sort by 16-bit cell ids (fine cells, ghost cells): rank or count
-> scan -> pack; the two-digit sort by 32-bit cell ids built on it (grids beyond
1024 cells); the SortRoute that brings per-row results back out of sorted
order; and the extended fine grid with ghost layers (ghost_grid)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._arrays import Positions, Rows
from ._stage import (_TORCH_POS, _alias_rows, _i64s, _offsets_like, _payload, _ptrs, _results,
                     _scratch, bin_count, scan, unpack_fields)


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


class WideSortRoute(SortRoute):
    """The SortRoute of the two-digit sort by 32-bit cell ids
    (``ghost_cell_sort(..., max_cells=, return_route=True)`` on a grid beyond
    1024 cells): it owns the routes of both passes, and ``unsort`` /
    ``return_to_source(..., sort_route=)`` undo pass 2, then pass 1, through
    one intermediate buffer per field (two launches; the buffers, n * row
    bytes each, live for the call only).  Memory per live route: the two
    passes' routes -- ranked passes about 8 B/row (a digit and a rank per row
    and pass) + 2 * T * (nb0 + nb1) + both workspaces; counted passes 2-4
    B/row + the workspaces -- until ``release()``."""

    def __init__(self, n, ncells, low, high):
        self.n, self.nbins, self.tile_rows = int(n), int(ncells), low.tile_rows
        self.ranked = low.ranked and high.ranked
        self._passes = (low, high)

    @property
    def released(self):
        return self._passes is None

    def release(self):
        """Free the route's device memory; it cannot be used afterwards."""
        if self._passes is not None:
            for r in self._passes:
                r.release()
        self._passes = None


def _unsort_into(sroute, srcs, rbs, outs):
    """outs[f][r] = srcs[f][slot(r)] for the sort that made ``sroute``: flat
    device tensors of sroute.n rows of rbs[f] bytes; one launch (a
    WideSortRoute: one per pass, the high digit's first)."""
    n, s = sroute.n, _lib.stream_handle()
    if n == 0:
        return
    if isinstance(sroute, WideSortRoute):
        low, high = sroute._passes
        mids = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=o.device)
                for rb, o in zip(rbs, outs)]
        _unsort_into(high, srcs, rbs, mids)
        _unsort_into(low, mids, rbs, outs)
        return
    src_a, out_a = [t.data_ptr() for t in srcs], [t.data_ptr() for t in outs]
    if sroute.ranked:
        _lib.call("mgr_unpack_ranked_fields", len(rbs), _ptrs(src_a), _i64s(rbs), n,
                  _lib.ptr(sroute._ids), _lib.ptr(sroute._ranks), _lib.ptr(sroute._tstarts),
                  sroute.nbins, sroute.tile_rows, _lib.ptr(sroute._ws), _ptrs(out_a), s)
    else:
        unpack_fields(src_a, rbs, n, sroute._dest, sroute.nbins, -1, sroute.tile_rows,
                      sroute._ws, out_a, s)


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

        def pack(f, o):
            _lib.call("mgr_pack_ranked", _lib.ptr(f.flat), f.row_bytes, n, _lib.ptr(ids),
                      _lib.ptr(ranks), _lib.ptr(tstarts), nb, tile_rows, _lib.ptr(ws),
                      _lib.ptr(o), s)
    else:
        ranks = tstarts = None
        _lib.call("mgr_count_ids", _lib.ptr(ids), n, nb, tile_rows, _lib.ptr(dest),
                  _lib.ptr(bad), _lib.ptr(ws), s)

        def pack(f, o):
            _lib.call("mgr_pack", _lib.ptr(f.flat), f.row_bytes, n, _lib.ptr(dest), nb, -1,
                      tile_rows, _lib.ptr(ws), _lib.ptr(o), -1, None, s)
    scan(n, nb, tile_rows, ws, counts, s)
    outs = []
    for f in fields:
        outs.append(torch.empty(max(n * f.row_bytes, 1), dtype=torch.uint8, device=dev))
        pack(f, outs[-1])
    if bad is not None:
        counts.masked_fill_(bad.ne(0), -1)
    if not route:
        return outs, counts
    if scratch is not None:   # the route owns them: the next sort allocates anew
        for name in ("ws_fine", "dest_fine", "ranks_fine", "tstarts_fine"):
            scratch.take(name)
    return outs, counts, SortRoute(n, nb, tile_rows, ws, ids if ranked else None, ranks,
                                   tstarts, dest)


GHOST_MAX_CELLS = 1024   # the ranked sort's bound (mgr_rank_ids + mgr_pack_ranked)
CELLS_MAX = 1 << 20      # the two-digit sort's bound (mgr.h MGR_MAX_WIDE_CELLS)

# How the two-digit sort cuts a cell id of ``bits`` bits: "balanced" -- a low
# digit of ceil(bits / 2) bits: the fewest bins per pass, so the longest runs in
# the ranked pack and the smallest tile tables -- or "low10" -- 10 low bits and
# the rest.  Both measured once; the product uses this one.
WIDE_SPLIT = "balanced"


def _digit_split(ncells, split=None):
    """(b0, b1, nb0, nb1): the low and high digits' bits, each <= 10, and the
    bins of the two passes, for ids < ncells <= CELLS_MAX."""
    if not 1 <= ncells <= CELLS_MAX:
        raise ValueError(f"{ncells} cells: 1..{CELLS_MAX}")
    bits = max(2, (int(ncells) - 1).bit_length())
    split = split or WIDE_SPLIT
    if split == "balanced":
        b0 = (bits + 1) // 2
    elif split == "low10":
        b0 = min(10, bits - 1)
    else:
        raise ValueError(f"digit split {split!r}: 'balanced' or 'low10'")
    b1 = bits - b0
    return b0, b1, 1 << b0, (int(ncells) + (1 << b0) - 1) >> b0


def _sort_by_wide_ids(fields, ids, n, ncells, dev, route=False, split=None):
    """Stable sort of every field by 32-bit cell ids < ncells <= CELLS_MAX
    (``ids``: an int32 device tensor of >= n entries, bits as uint32): a
    least-significant-digit sort in two passes of _sort_by_ids over digits of
    at most 10 bits (_digit_split).

      1. low digit of the ids (mgr_id_digit); every field, and the ids as one
         more 4-byte field, sorted by it at nb0 = 2^b0 bins;
      2. high digit of the permuted ids (mgr_id_digit); pass 1's outputs and
         the ids sorted by it at nb1 = ceil(ncells / 2^b0) bins;
      3. offsets[c] = rows with id < c from the sorted ids (mgr_cell_offsets),
         whose ``bad`` word -- an id >= ncells, or ids the two passes left out
         of order -- turns every offset to -1 on the device, without a sync.

    Each pass is _sort_by_ids unchanged: rows of 4-byte multiples <= 64 B take
    the ranked kernels, others count + scan + the generic pack.  Pass 1's
    outputs are dropped as soon as pass 2 is enqueued.  Peak device memory
    beside the inputs: about twice the payload + 8 B/row (both passes' outputs
    with their riding ids) + 4 B/row of digits + the passes' workspaces.
    Returns ([sorted flat fields], offsets[ncells + 1] (int64, device)), and
    with ``route`` a WideSortRoute."""
    b0, b1, nb0, nb1 = _digit_split(ncells, split)
    s = _lib.stream_handle()

    def digit(src, shift, bits):
        d = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        _lib.call("mgr_id_digit", _lib.ptr(src), n, shift, bits, _lib.ptr(d), s)
        return d[:n]

    idf = _IdField(ids.view(torch.uint8).reshape(-1), 4)
    outs1, _, *r1 = _sort_by_ids(list(fields) + [idf], digit(ids, 0, b0), n, nb0, dev,
                                 check_ids=False, route=route)
    mid = [_IdField(o, f.row_bytes) for o, f in zip(outs1, list(fields) + [idf])]
    outs2, _, *r2 = _sort_by_ids(mid, digit(outs1[-1], b0, b1), n, nb1, dev, check_ids=False,
                                 route=route)
    del outs1, mid   # stream-ordered: pass 2 has consumed them
    offsets = torch.empty(ncells + 1, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("mgr_cell_offsets", _lib.ptr(outs2[-1]), n, ncells, _lib.ptr(offsets),
              _lib.ptr(bad), s)
    offsets.masked_fill_(bad.ne(0), -1)
    if not route:
        return outs2[:-1], offsets
    return outs2[:-1], offsets, WideSortRoute(n, ncells, r1[0], r2[0])


def _wide_offsets_like(data, offsets):
    """The wide sort's offsets in the container of ``data``; host results are
    checked at the copy (-1: the failure convention), device results stay
    asynchronous."""
    if isinstance(data, torch.Tensor) and data.is_cuda:
        return offsets
    host = offsets.cpu()
    if bool((host < 0).any()):
        raise _lib.MgrError("the sorted cell ids are out of range or out of order (the device "
                            "check of mgr_cell_offsets)")
    return host if isinstance(data, torch.Tensor) else host.numpy()


def ghost_grid(cell_length, cell_limits, fine_cells, overload_lengths, max_cells=GHOST_MAX_CELLS):
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
    ``max_cells``: the bound on prod(extents) and on the ghost layers of a
    dimension -- 1024 (GHOST_MAX_CELLS, the ranked sort) by default, up to
    CELLS_MAX = 2^20 for the two-digit sort of ``ghost_cell_sort(...,
    max_cells=)``.  ValueError: prod(extents) beyond ``max_cells``, a fine
    cell count < 1, a negative or non-finite overload length, ``max_cells``
    outside 1..CELLS_MAX."""
    max_cells = int(max_cells)
    if not 1 <= max_cells <= CELLS_MAX:
        raise ValueError(f"max_cells {max_cells}: 1..{CELLS_MAX}")
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
    if (ghost > max_cells).any():
        raise ValueError(f"ghost layers of {ghost.tolist()} cells: beyond {max_cells}")
    ghost = ghost.astype(np.int64)
    extents = fine + 2 * ghost
    cells = 1
    for e in extents:
        cells *= int(e)
    if cells > max_cells:
        why = ("the ranked sort's bound" if max_cells == GHOST_MAX_CELLS else "max_cells")
        raise ValueError(f"extended grid {extents.tolist()} has {cells} cells: at "
                         f"most {max_cells} ({why}); use fewer fine cells")
    origin = np.ascontiguousarray(np.asarray(cell_limits, dtype=np.float64)[:, 0])
    return ghost, extents, origin, width


def _sort_by_cells(data, position, dim, dev, nb, cell_ids, return_positions, return_route,
                   floats=None, failed=None):
    """What fine_cell_sort and ghost_cell_sort share: the payload's fields
    (and the position rows with ``return_positions``) stably sorted by the ids
    of ``cell_ids(pos, n, fields)`` -> (ids, check_ids, after); ``after(counts)``
    (or None) runs before the counts become offsets.  int32 ids are 32-bit cell
    ids (nb > 1024 cells): the two-digit sort (_sort_by_wide_ids), where
    ``after`` gets the offsets.  Returns (data, [positions,]
    offsets[nb + 1], [SortRoute]).  ``floats``: the caller's name, if it takes
    float32 / float64 positions only; ``failed``: what -1 counts mean there."""
    rows, multi = _payload(data, dev)
    pos = Positions(position, dim, dev, data_rows=_alias_rows(position, rows))
    if floats and pos.code not in _TORCH_POS:
        raise TypeError(f"{floats}: float32 or float64 positions")
    n = rows[0].n
    if pos.n != n:
        raise ValueError(f"data has {n} rows, position has {pos.n}")
    prow = Rows(position, dev) if return_positions else None
    fields = rows + ([prow] if prow else [])
    ids, check, after = cell_ids(pos, n, fields)
    wide = ids.dtype == torch.int32
    if wide:
        outs, counts, *sroute = _sort_by_wide_ids(fields, ids, n, nb, dev, route=return_route)
    else:
        outs, counts, *sroute = _sort_by_ids(fields, ids, n, nb, dev, check_ids=check,
                                             route=return_route)
    if after is not None:
        after(counts)
    nd = len(rows)
    res = [_results(rows, outs[:nd], n, multi)]
    if prow:
        res.append(prow.wrap(outs[nd], n))
    try:
        res.append(_wide_offsets_like(rows[0].obj, counts) if wide
                   else _offsets_like(rows[0].obj, counts, dev))
    except _lib.MgrError as e:
        if failed is None:
            raise
        raise _lib.MgrError(f"{failed}, or: {e}") from None
    return tuple(res) + tuple(sroute)


def _fine_sort(plan, coarse, dim, dev, data, position, return_positions, fine_ids=None,
               return_route=False):
    """The fine cells of the rows -- ``fine_ids`` as given (computed at the
    source), else one read of the positions (mgr_bin_count_fine against the
    coarse plan, periodic=0: no wrap, no write-back; the fine cell is the fine
    plan's binning by construction, mgr_device.h bin_coord) -- then the
    stable sort by them (_sort_by_ids).  ``return_route``: the SortRoute of
    the sort is appended to the result."""
    def cell_ids(pos, n, fields):
        if fine_ids is None:
            ids = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
            hint = max(f.row_bytes for f in fields)
            tile_rows, ws, dest = _scratch(n, coarse.nbins, hint, dev)
            bin_count(coarse, pos, False, dest, tile_rows, ws, _lib.stream_handle(),
                      fine=(plan, ids))
            return ids[:n], False, None
        ids = _as_ids(fine_ids, n, dev, plan.nbins)
        if (return_route and isinstance(fine_ids, torch.Tensor) and n
                and ids.untyped_storage().data_ptr() == fine_ids.untyped_storage().data_ptr()):
            ids = ids.clone()   # the caller's tensor: the route keeps its own copy
        return ids, True, None

    return _sort_by_cells(data, position, dim, dev, plan.nbins, cell_ids, return_positions,
                          return_route)


class _IdField:
    """A flat device field; by default the 2-byte fine cells or halo flags."""

    def __init__(self, flat, row_bytes=2):
        self.flat, self.row_bytes = flat, row_bytes
