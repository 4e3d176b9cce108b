"""GridPartitioner -- the 1-GPU local stage (bin + scan + stable pack, or
the one-pass partition) without an exchange."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._arrays import Positions, device, pos_code
from ._stage import (_TORCH_POS, MAX_FIELDS, _alias_rows, _FinePlans, _i64s, _offsets_like,
                     _payload, _Plan, _ptrs, _results, _scratch, _tile_hint, bin_count,
                     pack_fields, scan, unpack_fields)
from .exchange import check_counts


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


class GridPartitioner(_FinePlans):
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

    def _two_pass(self, pos, periodic, srcs, rbs, bufs, stream, fine=None, outs=None):
        """bin -> scan -> mgr_pack_fields of the fields at the addresses
        ``srcs`` by one binning of ``pos``, a Positions (finished after the
        binning) or (device tensor, code).  ``bufs``: (tile_rows, workspace,
        dest, counts); ``fine``: (fine plan, ids, partitioned ids), the fine
        cells riding along; ``outs``: given, or allocated behind the scan."""
        tile_rows, ws, dest, counts = bufs
        host = isinstance(pos, Positions)
        n = pos.n if host else int(pos[0].shape[0])
        bin_count(self._plan, pos, periodic, dest, tile_rows, ws, stream,
                  fine=fine[:2] if fine else None)
        if host:
            pos.finish()
        scan(n, self.nbins, tile_rows, ws, counts, stream)
        if outs is None:
            outs = [torch.empty(max(n * rb, 1), dtype=torch.uint8, device=self._dev)
                    for rb in rbs]
        side = (fine[1].data_ptr(), fine[2].data_ptr(), None) if fine else (None, None, None)
        pack_fields(srcs, rbs, n, dest, self.nbins, -1, tile_rows, ws,
                    [o.data_ptr() for o in outs], stream, side=side)
        return outs

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
        bin_count(self._plan, (pos_tensor, code), periodic, dest, tile_rows, ws, s,
                  fine=(fplan, fid))
        scan(n, self.nbins, tile_rows, ws, counts, s)
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
        key = ("fields", n, tuple(int(b) for b in row_bytes))
        if key not in self._cache:
            tile_rows, ws, dest = _scratch(n, self.nbins, _tile_hint(list(row_bytes)), self._dev)
            outs = [torch.empty(max(n * int(b), 1), dtype=torch.uint8, device=self._dev)
                    for b in row_bytes]
            counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
            self._cache = {key: (tile_rows, ws, dest, outs, counts)}
        tile_rows, ws, dest, outs, counts = self._cache[key]
        self._last_part = key
        self.last_counts = counts
        fine = ((self._fine_plan(fine_cells),) + self.fine_buffers(n)
                if fine_cells is not None else None)
        self._two_pass((pos_tensor, pos_code(pos_tensor.dtype)), periodic,
                       [f.data_ptr() for f in flats], row_bytes, (tile_rows, ws, dest, counts),
                       _lib.stream_handle(stream), fine=fine, outs=outs)
        if fine is None:
            return outs, counts
        return outs, fine[2].view(torch.int16)[:n], counts

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
        unpack_fields([t.data_ptr() for t in flats], rbs, n, dest, self.nbins, -1, tile_rows, ws,
                      [o.data_ptr() for o in outs], _lib.stream_handle(stream))
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
        cnt_d = torch.empty(nb, dtype=torch.int64, device=self._dev)
        fine = fido = None
        if fine_cells is not None:
            fid = torch.empty(max(n, 1), dtype=torch.int16, device=self._dev)
            fido = torch.empty(max(n, 1), dtype=torch.int16, device=self._dev)
            fine = (self._fine_plan(fine_cells), fid, fido)
        outs = self._two_pass(pos, periodic, [f.flat.data_ptr() for f in fields], rbs,
                              (tile_rows, ws, dest, cnt_d), _lib.stream_handle(), fine=fine)
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

    def _onepass_view(self, fields, pos, multi):
        """The positions as the one-pass kernels take them (3-D, f32 / f64), else
        None: one array: a view inside the records; SoA (``soa_onepass``): the
        tensor, or for a numpy view of a field that view of its device bytes."""
        n, esz = fields[0].n, _lib.POS_ITEMSIZE[pos.code]
        if not (n and self.dim == 3 and pos.code in _TORCH_POS and (self.soa_onepass
                                                                    or not multi)):
            return None
        if multi and pos.t is not None:
            return pos.t
        rows = pos._alias_rows if multi else fields[0]
        off, rb = pos.addr - rows.flat.data_ptr(), rows.row_bytes
        if not multi and not (pos.stride * esz == rb and 0 <= off and off + 3 * esz <= rb
                              and off % esz == 0):
            return None
        base = rows.flat.view(_TORCH_POS[pos.code])
        return torch.as_strided(base, (n, 3), (pos.stride, 1),
                                (pos.addr - base.untyped_storage().data_ptr()) // esz)

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
        mgr_pack_fields over all fields.  (One array comes back as slices of the
        cached one-pass output.)"""
        fields, multi = _payload(data, self._dev)
        pos = Positions(position, self.dim, self._dev, data_rows=_alias_rows(position, fields))
        n, nf, nb = fields[0].n, len(fields), self.nbins
        if pos.n != n:
            raise ValueError("data and position row counts differ")
        rbs = [f.row_bytes for f in fields]
        cuda_out = fields[0].kind == "torch" and fields[0].out_device.type == "cuda"
        pos_t = self._onepass_view(fields, pos, multi)
        parts = None
        if pos_t is not None:
            try:
                if multi:
                    outs, fo, cnt_d, cap = self.partition_onepass_fields_device(
                        [f.flat for f in fields], rbs, pos_t, periodic, fine_cells=fine_cells)
                else:
                    out, fo, cnt_d, cap = self.partition_onepass_device(
                        fields[0].flat, rbs[0], pos_t, periodic, fine_cells=fine_cells)
                    outs = [out]
                counts = cnt_d.cpu().numpy()
                pos.finish()
                check_counts(counts, [])
                if (counts > cap).any():   # a bin outgrew its region: the two-pass path
                    periodic = False       # the positions are wrapped already (S2)
                else:
                    fresh = (lambda t: t.clone()) if multi and cuda_out else (lambda t: t)
                    parts = [[fresh(outs[i][b * cap * rbs[i]:(b * cap + int(counts[b])) * rbs[i]])
                              for b in range(nb)] for i in range(nf)]
                    fparts = ([fresh(fo[b * cap:b * cap + int(counts[b])]) for b in range(nb)]
                              if fo is not None else None)
            except _lib.MgrError as e:
                if "(-4)" not in str(e):      # MGR_EUNSUPPORTED: the two-pass path
                    raise
        if multi:
            self.last_lists_path = "twopass" if parts is None else "onepass"
        if parts is None:
            parts, fparts, counts = self._two_pass_lists(fields, pos, periodic, fine_cells)
        res = tuple([f.wrap(p, int(c)) for p, c in zip(parts[i], counts)]
                    for i, f in enumerate(fields))
        res = res if multi else res[0]
        if fine_cells is None:
            return res
        if cuda_out:
            return res, fparts            # int16 tensors holding the uint16 cells
        return res, [f.cpu().numpy().view(np.uint16) for f in fparts]

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
        counts = torch.empty(self.nbins, dtype=torch.int64, device=self._dev)
        outs = self._two_pass(pos, periodic, [f.flat.data_ptr() for f in fields], rbs,
                              (tile_rows, ws, dest, counts), _lib.stream_handle())
        # device results stay asynchronous: a failed scan shows as -1 counts
        offsets = _offsets_like(fields[0].obj, counts, self._dev)
        return _results(fields, outs, n, multi), offsets
