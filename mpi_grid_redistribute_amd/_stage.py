"""What MPIGridRedistributor, GridPartitioner and the fine-cell sort share:
the native plan, scratch buffers, payload adapters, and ONE function per
native stage -- ``bin_count`` (mgr_bin_count / _fine / _halo), ``scan``,
``pack_fields``, ``unpack_fields`` -- through which every caller in the package
launches them (halo.py keeps a mgr_scan call for its selection workspaces)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._arrays import Positions, Rows, box_dtype_code
from .exchange import check_counts

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


class _FinePlans:
    """Base of the two classes that bin into fine cells (``grid_topology``,
    ``box_length``, ``dim`` and the dict ``_fine_plans`` are theirs)."""

    def _fine_plan(self, fine_cells):
        """Made once per shape; ``dim`` entries, as the native side reads."""
        fine = np.array(fine_cells).astype(np.int64)
        if fine.ndim != 1 or len(fine) != self.dim:
            raise ValueError(f"fine_cells must have {self.dim} entries")
        key = tuple(int(x) for x in fine)
        plan = self._fine_plans.get(key)
        if plan is None:
            plan = self._fine_plans[key] = _Plan(self.grid_topology, self.box_length, 0,
                                                 fine=fine)
        return plan


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


# ------------------------------------------------------------ native stages
def bin_count(plan, pos, periodic, dest, tile_rows, ws, stream, fine=None, halo=None):
    """The binning launch: every row's destination byte into ``dest``, tile
    histograms into ``ws``, positions wrapped in place when ``periodic``.
    ``pos``: a Positions, or (device tensor (n, >= dim), its mgr_dtype code).
    ``fine`` = (fine plan, int16 id buffer): the fine cells too (mgr_bin_count_
    fine); ``halo`` = (flag buffer, cell_length, overload_lengths as float64
    numpy): the halo face flags too (mgr_bin_count_halo); else mgr_bin_count."""
    if isinstance(pos, Positions):
        rows = (ctypes.c_void_p(pos.addr), pos.code, pos.n, pos.stride)
    else:
        t, code = pos
        rows = (_lib.ptr(t), code, int(t.shape[0]), t.stride(0))
    rows += (int(bool(periodic)), _lib.ptr(dest))
    tiles = (tile_rows, _lib.ptr(ws), stream)
    if fine is not None:
        _lib.call("mgr_bin_count_fine", plan.h, fine[0].h, *rows, _lib.ptr(fine[1]), *tiles)
    elif halo is not None:
        flags, cl, ol = halo
        _lib.call("mgr_bin_count_halo", plan.h, *rows, _lib.ptr(flags),
                  cl.ctypes.data_as(ctypes.c_void_p), ol.ctypes.data_as(ctypes.c_void_p), *tiles)
    else:
        _lib.call("mgr_bin_count", plan.h, *rows, *tiles)


def scan(n, nbins, tile_rows, ws, counts, stream):
    """Tile histograms in ``ws`` -> segment starts; bin row counts -> ``counts``."""
    _lib.call("mgr_scan", n, nbins, tile_rows, _lib.ptr(ws), _lib.ptr(counts), stream)


def pack_fields(srcs, row_bytes, n, dest, nbins, drop_bin, tile_rows, ws, outs, stream,
                redirect_bin=-1, redirect=None, side=(None, None, None), t0=0, t1=-1):
    """Every field in ONE mgr_pack_fields call (one ranking for all).  ``srcs``
    / ``outs`` / ``redirect``: device addresses per field; the rows of
    ``redirect_bin`` (>= 0) go to ``redirect``.  ``side``: (source, output,
    redirect) addresses of the 2-byte side field, None where absent; tiles t0..t1."""
    vp = [ctypes.c_void_p(a) if a else None for a in side]
    _lib.call("mgr_pack_fields", len(srcs), _ptrs(srcs), _i64s(row_bytes), n, _lib.ptr(dest),
              nbins, drop_bin, tile_rows, _lib.ptr(ws), _ptrs(outs), redirect_bin,
              _ptrs(redirect) if redirect_bin >= 0 else None, *vp, t0, t1, stream)


def unpack_fields(srcs, row_bytes, n, dest, nbins, drop_bin, tile_rows, ws, outs, stream,
                  redirect_bin=-1, redirect=None):
    """The inverse of pack_fields in one mgr_unpack_fields call:
    outs[f][r] = srcs[f][slot(r)] (addresses per field); the rows of
    ``redirect_bin`` (>= 0) are read from ``redirect``, dropped rows are zero."""
    _lib.call("mgr_unpack_fields", len(row_bytes), _ptrs(srcs), _i64s(row_bytes), n,
              _lib.ptr(dest), nbins, drop_bin, tile_rows, _lib.ptr(ws), _ptrs(outs),
              redirect_bin, _ptrs(redirect) if redirect_bin >= 0 else None, 0, -1, stream)
