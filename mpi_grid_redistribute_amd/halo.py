"""Overload (halo) exchange -- ``exchange_overload_by_position`` (redist.py:202-309).

After the main redistribution every rank holds the rows of its own cell.  The
halo exchange adds, dimension by dimension, copies of the neighbours' rows
that lie within ``overload_lengths[d]`` of the shared face:

  for d in 0..dim-1 (redist.py:246):
      a / b = right / left neighbour cell (periodic wrap, :248-255)
      to_a  = rows with pos[:, d] > limits[d,1] - ol[d]   (local, then buffer)
      to_b  = rows with pos[:, d] < limits[d,0] + ol[d]
      step 1: send to_a -> a, receive from_b <- b         (:289-295)
      step 2: send to_b -> b, receive from_a <- a         (:298-303)
      buffer = concat(buffer, from_a, from_b)             (:305-306)

Data and positions travel with the same selections (the reference sends
them as two passes, :264); rows received in earlier dimensions are forwarded
in later ones, which fills the edge/corner regions.  Kept reference quirks:
positions are not shifted across the periodic boundary (``unwrap=True``
shifts them: exchange_overload, mgr_shift_regions); with
``periodic=False`` the left send uses the right neighbour's flag (:287);
``redistribute_by_position`` never forwards ``periodic`` (:165).

On the GPU every row carries 16 face-flag bits (bit 2d: coordinate d beyond
the right threshold, bit 2d+1: below the left one).  Through
``redistribute_by_position`` the binning kernel computes them against the
limits of the cell the row lands in (mgr_bin_count_halo) and they travel
with the row; called directly, one pass over the local positions computes
them (mgr_halo_flags).  They stay valid on every rank a row is forwarded to:
a neighbour's cell differs from the sender's only in the dimension of the
exchange, whose bits are not read again.

  1. the local rows' 2*dim selections counted in ONE pass (mgr_msel_count,
     mgr_scan); one group exchanges the counts with the neighbours; one host
     sync reads them;
  2. the local sends of every dimension whose neighbours are other ranks
     (and of dimension 0) are packed in one pass (mgr_msel_pack_fields:
     data, positions when carried, flags), each set straight to its place;
  3. per dimension d: the received rows so far (the buffer) are selected the
     same way (2 sets) -- a small set; from d = 1 their counts travel as an
     8-byte message and one host sync reads them; then ONE group moves, in
     the reference's order (step 1, then step 2), the local piece and the
     buffer piece of every field to each neighbour, the receives landing
     appended to the buffer in place.  A dimension whose neighbours are this
     rank itself (a grid extent of 1) sends nothing: its pieces are packed
     straight into the buffer where the receives would land.
Host syncs: 1 + (dim - 1) per exchange.  The buffer is an append-only store:
redistribute_by_position hands over the spare rows of its output, so the
final concatenate(data, overload) (:166) costs nothing while the halo fits;
when the positions are not returned they are not carried at all (the flags
already hold everything the selections read).

A SoA payload (a list of fields, at most _lib.MAX_FIELDS) moves the same way:
the fields of a pack, a staging buffer or a message group are then the
payload's fields, the positions when carried, and the flags -- up to
_lib.MSEL_MAX_FIELDS = MAX_FIELDS + 2, which mgr_msel_pack_fields takes in one
call (the wide kernel from 4 fields on, mgr.h).
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .exchange import check_counts, host_read_start, host_read_wait


def _p2p(transport, ops):
    """One batch of point-to-point messages, its off-rank bytes counted in
    the transport's traffic."""
    transport.note_p2p(ops)
    transport.p2p(ops)


# The multi-rank halo's count messages carry a failure bit beside the size: a
# selection scan that gave up (-1 counts) is announced as size 0 with the bit
# set, so every message of the exchange keeps consistent sizes on both sides
# (nobody waits for a message that will not come), and the ranks agree on the
# failure ONCE, after the last message, instead of after every count exchange.
_FAIL = 1 << 62


def _encode_counts(c):
    """Device int64 counts -> message words: size (>= 0), plus _FAIL on every
    word when any count is negative (a failed scan poisons all of them)."""
    bad = (c < 0).any()
    return torch.where(bad, torch.full_like(c, _FAIL), c.clamp(min=0))


def _decode(words):
    w = np.asarray(words, dtype=np.int64)
    return w & (_FAIL - 1), bool((w >> 62).any())


def _agree_counts(transport, sent, received):
    """check_counts on every rank at once: a -1 count (a selection scan that
    gave up) reaches only the neighbours of the failed rank, so the ranks
    agree on the flag first and all raise, none left waiting in a message."""
    failed = (np.asarray(sent) < 0).any() or (np.asarray(received) < 0).any()
    if transport.any_failed(failed):
        check_counts(sent, received)
        check_counts([-1], [])     # a peer failed: raise here too


def _swap_counts(transport, sel, dev, counts, nbs, failed):
    """One count swap with the neighbours ``nbs`` (neighbour tuples, one per
    dimension concerned): ``counts`` = device int64, per dimension the rows to
    a and to b (None: nothing selected, zeros).  One group of 8-byte messages,
    one host read.  Returns the sizes sent, the sizes received ([from_b,
    from_a] per dimension) and the new ``failed``: a failed selection scan
    (here, or at a neighbour through its messages) travels as the failure bit
    and is announced on from then on, so the neighbours' neighbours learn too;
    sizes stay as announced (the neighbours post receives of them) and the
    ranks agree at the end of the exchange.  A side that does not send: 0."""
    k = 2 * len(nbs)
    send = torch.zeros(k, dtype=torch.int64, device=dev)
    recv = torch.zeros(k, dtype=torch.int64, device=dev)
    if counts is not None:
        send.copy_(_encode_counts(counts))
    if failed:
        send.fill_(_FAIL)
    ops = []
    for i, (a, b, keep_a, keep_b) in enumerate(nbs):
        if not keep_a:
            send[2 * i].zero_()
        if not keep_b:
            send[2 * i + 1].zero_()
        ops += [("send", a, send[2 * i:2 * i + 1].view(torch.uint8)),
                ("recv", b, recv[2 * i:2 * i + 1].view(torch.uint8)),
                ("send", b, send[2 * i + 1:2 * i + 2].view(torch.uint8)),
                ("recv", a, recv[2 * i + 1:2 * i + 2].view(torch.uint8))]
    _p2p(transport, ops)
    sent, received = sel.to_host([send, recv])
    sent, f1 = _decode(sent)
    received, f2 = _decode(received)
    return sent, received, failed or f1 or f2


def self_halo_pieces(dim):
    """The overload rows of a rank that is its own neighbour in every
    dimension (one rank; periodic), as pieces in store order: piece = the
    local rows whose flags hold every bit of its mask, in row order.  The
    reference's loop (redist.py:246-306) on sets of local rows: per dimension
    to_a = local rows beyond the right face, then the buffer's; to_b the same
    at the left face; the rank receives its own to_a as from_b and its own
    to_b as from_a, and buffer = concat(buffer, from_a, from_b) (:305-306).
    3^dim - 1 pieces: the faces, edges and corners of the halo."""
    buf = []
    for d in range(dim):
        a, b = 1 << (2 * d), 1 << (2 * d + 1)
        to_a = [a] + [m | a for m in buf]
        to_b = [b] + [m | b for m in buf]
        buf = buf + to_b + to_a
    return buf


class Step(namedtuple("Step", "nla nlb nga ngb rla rga rlb rgb ia ib m gh")):
    """One dimension's step of the general path, as the host knows it once
    the counts are read: ``nla, nlb, nga, ngb`` rows sent (local / buffer
    piece, to a / b), ``rla, rga, rlb, rgb`` rows received (the senders' local
    / buffer pieces, from a / b), ``ia, ib`` where the received pieces are
    appended -- concat(buffer, from_a, from_b), redist.py:305 --, ``m`` the
    buffer rows before the dimension and ``gh`` the buffer's selection handle
    (None: nothing was selected)."""
    __slots__ = ()
    to_a = property(lambda s: s.nla + s.nga)
    to_b = property(lambda s: s.nlb + s.ngb)
    from_a = property(lambda s: s.rla + s.rga)
    from_b = property(lambda s: s.rlb + s.rgb)
    end = property(lambda s: s.m + s.from_a + s.from_b)    # buffer rows after the dimension


def _forward_group(s, d, a, b, store, local, gbuf):
    """Dimension d's message group towards other ranks, in the reference's
    order: step 1 (send to a, receive from b) then step 2, and inside a step
    per field: local send, buffer send, local receive, buffer receive (RCCL
    matches a pair's messages in posting order).  ``local``: the _LocalSends
    holding the packed local pieces; ``gbuf[f]``: field f's packed buffer
    pieces, to a then to b; the receives land appended in ``store``."""
    ops = []
    for side, (to, frm, nl, ng, go, rl, rg, at) in enumerate(
            ((a, b, s.nla, s.nga, 0, s.rlb, s.rgb, s.ib),
             (b, a, s.nlb, s.ngb, s.nga, s.rla, s.rga, s.ia))):
        for f, rb in enumerate(store.rbs):
            if nl:
                ops.append(("send", to, local.staged(d, f, side)))
            if ng:
                ops.append(("send", to, gbuf[f][go * rb:(go + ng) * rb]))
            if rl:
                ops.append(("recv", frm, store.rows(f, at, rl)))
            if rg:
                ops.append(("recv", frm, store.rows(f, at + rl, rg)))
    return ops


def _backward_group(s, a, b, S, stage, ebs):
    """_forward_group with sender and receiver swapped (reduce_overload): the
    rows received from b / a go back from the value stores ``S`` -- they are
    contiguous there, nothing is packed -- and the values for this rank's own
    sends arrive in ``stage``, to_a's then to_b's.  Towards a pair of ranks
    the sends and the receives match in posting order (a == b on a grid
    extent of 2)."""
    ops = []
    for f, eb in enumerate(ebs):
        if s.from_b:
            ops.append(("send", b, S[f][s.ib * eb:(s.ib + s.from_b) * eb]))
        if s.to_a:
            ops.append(("recv", a, stage[f][: s.to_a * eb]))
        if s.from_a:
            ops.append(("send", a, S[f][s.ia * eb:(s.ia + s.from_a) * eb]))
        if s.to_b:
            ops.append(("recv", b, stage[f][s.to_a * eb:(s.to_a + s.to_b) * eb]))
    return ops


class HaloRoute:
    """What ``reduce_overload`` needs to sum per-row results on overload rows
    back onto the rows they are copies of (``exchange_overload(...,
    return_route=True)``): everything the forward exchange left on the device
    and read on the host, so the way back bins, scans and counts nothing.

      * the local rows' face flags (2 B/row) and their selection handle (masks
        and the msel workspace as mgr_scan left it);
      * per dimension: the neighbours and the ``Step`` -- the host-side sizes
        and places, and the buffer's selection handle (its own workspace, the
        flags of the rows received so far);
      * on the one-rank path the one selection handle over the 3^dim - 1
        pieces and the piece sizes.

    Buffers that came from a Scratch are TAKEN OUT of it (the next exchange
    allocates anew), so a route stays valid across later calls and may be
    used any number of times.  Memory per live route: about 2 * (n_local +
    n_halo) bytes of flags plus the msel workspaces (12 bytes per (set, tile
    of 4096 rows), + 32 KiB each).  Freed by ``release()``."""

    def __init__(self, owner, n_local, n_halo, flags, lh=None, nb=None, selfd=None, steps=None,
                 self_handle=None, self_counts=None):
        self._owner = owner
        self.n_local, self.n_halo = int(n_local), int(n_halo)
        self._flags, self._lh = flags, lh
        self._nb, self._selfd, self._steps = nb, selfd, steps
        self._self, self._self_counts = self_handle, self_counts
        self._live = True

    @property
    def released(self):
        return not self._live

    def release(self):
        """Free the route's device memory; it cannot be used afterwards."""
        self._flags = self._lh = self._steps = self._self = None
        self._live = False


def shift_regions(pos_flat, code, ncols, dim, ends, shifts):
    """mgr_shift_regions on the rows at the start of ``pos_flat`` (a flat uint8
    view of (rows, ncols) positions of dtype ``code``): region r = rows
    [ends[r-1], ends[r]) gets += shifts[r] (dim values), in chunks of 64
    regions (the call's limit)."""
    ends = [int(e) for e in ends]
    for k0 in range(0, len(ends), 64):
        k1 = min(len(ends), k0 + 64)
        r0 = ends[k0 - 1] if k0 else 0
        n = ends[k1 - 1] - r0
        if n <= 0 or not any(any(s) for s in shifts[k0:k1]):
            continue
        e = (ctypes.c_int64 * (k1 - k0))(*[x - r0 for x in ends[k0:k1]])
        s = (ctypes.c_double * ((k1 - k0) * dim))(*[float(v) for row in shifts[k0:k1]
                                                    for v in row])
        _lib.call("mgr_shift_regions",
                  ctypes.c_void_p(pos_flat.data_ptr() + r0 * ncols * _lib.POS_ITEMSIZE[code]),
                  code, n, ncols, dim, k1 - k0, e, s, _lib.stream_handle())


def _arena_stores(arena, multi, carry_pos):
    """The arena's stores in field order: payload, then positions when carried."""
    return (list(arena[0]) if multi else [arena[0]]) + ([arena[1]] if carry_pos else [])


def _result(sel, dev, shape, out, rows, in_arena, route=None):
    """What exchange_overload returns.  ``shape``: (payload fields, whether
    the payload is a list, whether positions are carried); ``out``: the
    fields' overload rows, payload then positions (not read when there are no
    rows); ``route``: None, or (the msel workspaces the route takes out of the
    scratch, HaloRoute's arguments but n_halo)."""
    D, multi, carry_pos = shape
    if not rows:
        out = [torch.empty(0, dtype=torch.uint8, device=dev)] * (D + carry_pos)
    res = (out[:D] if multi else out[0]), (out[D] if carry_pos else None), rows, in_arena
    if route is None:
        return res
    for name in route[0]:
        sel.take(name)   # the route owns the workspaces from here on
    return res + (HaloRoute(n_halo=rows, **route[1]),)


def _self_halo(transport, sel, srcs, rbs, flags, n, dim, carry_pos, arena, dev, pending=(),
               multi=False, owner=None, unwrap=None):
    """exchange_overload when every neighbour is this rank: all pieces are
    known from the local rows' flags, so one selection pass counts them all
    and one multi-set pack writes every row straight to each of its pieces
    in the store -- the local rows are read once, not once per dimension,
    and nothing is staged or received.  ``srcs`` / ``rbs``: the payload's
    fields, then the positions when carried; ``multi``: the payload is a list
    of fields (arena[0] a list of stores, the data returned as a list).
    ``unwrap``: (position dtype code, position columns, box lengths) -- the
    carried positions of every piece are shifted to the image beside the cell
    (mask bit 2d: beyond the right face, the copy lies on the left, -L_d; bit
    2d+1: +L_d), one mgr_shift_regions call once the piece sizes are known."""
    pieces = self_halo_pieces(dim)
    h, cnt = sel.msel_masks(flags, n, pieces, "_self")
    F = len(rbs)
    D = F - 1 if carry_pos else F                         # payload fields

    def unwrapped(out, offs):
        """out: the fields' overload rows, the pieces ending at offs[1:]."""
        if unwrap is not None:
            code, ncols, box = unwrap
            shifts = [[(-box[d] if m >> (2 * d) & 1 else 0.0) + (box[d] if m >> (2 * d + 1) & 1
                                                                  else 0.0)
                       for d in range(dim)] for m in pieces]
            shift_regions(out[D], code, ncols, dim, offs[1:], shifts)
        return out

    def result(out, total, in_arena):
        route = None if owner is None else (["msel_ws_self"], dict(
            owner=owner, n_local=n, flags=flags, self_handle=h,
            self_counts=np.asarray(counts, dtype=np.int64).copy()))
        return _result(sel, dev, (D, multi, carry_pos), out, total, in_arena, route)
    placed = arena is not None and arena[3] > 0
    # the one host read is enqueued BEFORE the placed pack and waited for on
    # its own event: the host finishes this call (and launches the caller's
    # next work) while the pack runs, instead of idling the GPU after it
    read = sel.to_host_start([cnt] + list(pending))
    if placed:   # into the arena before the sizes are known: no gap at the sync
        ast = _arena_stores(arena, multi, carry_pos)
        sel.msel_pack_placed(h, srcs, rbs, [ast[f][arena[2] * rbs[f]:] for f in range(F)],
                             arena[3])
    got = sel.to_host_wait(read)                          # the one host sync
    counts = got[0]
    for c in got[1:]:   # the redistribution's deferred count check
        check_counts(c, [])
    _agree_counts(transport, counts, [])
    total = int(counts.sum())
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if placed and total <= arena[3]:
        _lib.alg_add("halo_pack", 2 * n + 2 * total * sum(rbs))
        if not total:
            return result(None, 0, True)
        b = arena[2]
        return result(unwrapped([ast[f][b * rbs[f]:(b + total) * rbs[f]] for f in range(F)],
                                offs), total, True)
    if arena is not None and total <= arena[3]:
        st, base, in_arena = _arena_stores(arena, multi, carry_pos), arena[2], True
    else:
        st = [torch.empty(max(total, 1) * rb, dtype=torch.uint8, device=dev) for rb in rbs]
        base, in_arena = 0, False
    dsts = [[st[f][(base + int(offs[k])) * rbs[f]:(base + int(offs[k + 1])) * rbs[f]]
             if counts[k] else None for k in range(len(pieces))] for f in range(F)]
    if total:
        sel.msel_pack_fields(h, srcs, rbs, dsts, total)
    if not total:
        return result(None, 0, in_arena)
    return result(unwrapped([st[f][base * rbs[f]:(base + total) * rbs[f]] for f in range(F)],
                            offs), total, in_arena)


def neighbours(R, d, periodic):
    """Right/left neighbour ranks of R's cell in dimension d and whether each
    side sends (redist.py:248-267, quirk :287 -- the left send's flag is the
    right neighbour's)."""
    ea = np.zeros(R.dim, dtype=np.int64)
    ea[d] = 1
    ia, ib = R.rank_cell_index + ea, R.rank_cell_index - ea
    a = int(R.get_cell_number_from_indexes_host(np.array([ia]))[0])
    b = int(R.get_cell_number_from_indexes_host(np.array([ib]))[0])
    if periodic:
        keep_a = keep_b = True
    else:
        keep_a = bool(R.get_cell_number_from_indexes_host(np.array([ia]), periodic=False)[0] == a)
        keep_b = keep_a
    return a, b, keep_a, keep_b


def thresholds(R, overload_lengths):
    """hi[d] = limits[d,1] - ol[d], lo[d] = limits[d,0] + ol[d], in float64
    with numpy's scalar promotion (redist.py:271-276)."""
    ol = overload_lengths
    hi = np.array([np.float64(R.rank_cell_limits[d, 1] - ol[d]) for d in range(R.dim)])
    lo = np.array([np.float64(R.rank_cell_limits[d, 0] + ol[d]) for d in range(R.dim)])
    return hi, lo


SELECT_TILE_ROWS = 4096


def halo_capacity(R, m, overload_lengths):
    """Spare rows to reserve after a rank's m redistributed rows for its halo:
    the uniform-density estimate m * (prod(1 + 2 ol/len) - 1), x1.25, + 4096,
    with ol capped at the cell length (the exchange reaches the immediate
    neighbours only, so each factor is at most 3) and the whole at
    (3^dim - 1) * m.  A halo that outgrows it still works (exchange_overload
    then moves to its own store and the caller concatenates)."""
    cl = np.asarray(R.cell_length, dtype=np.float64)
    ol = np.minimum(np.maximum(np.asarray(overload_lengths, dtype=np.float64), 0.0), cl)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = float(np.prod(1.0 + 2.0 * np.where(cl > 0, ol / cl, 1.0)) - 1.0)
    frac = min(frac, 3.0 ** len(cl) - 1.0)
    return int(m * frac * 1.25) + 4096


class _Handle(namedtuple("_Handle", "n flags masks k ws tile_rows")):
    """A counted and scanned multi-set selection (DeviceSelect.msel_masks):
    rows, their flags, the k masks (ctypes ints), the workspace as mgr_scan
    left it.  Opaque to the exchange."""
    __slots__ = ()

    @property
    def args(self):
        """The selection as every mgr_msel_* pack / unpack call takes it."""
        return (self.n, _lib.ptr(self.flags), self.k, self.masks, self.tile_rows,
                _lib.ptr(self.ws))


def _field_args(srcs, row_bytes):
    """(fields, their source pointers, their row bytes) of a multi-field pack."""
    nf = len(srcs)
    return (nf, (ctypes.c_void_p * nf)(*[_lib.ptr(t) for t in srcs]),
            (ctypes.c_int64 * nf)(*row_bytes))


class DeviceSelect:
    """Selections on the GPU: face flags (mgr_halo_flags) and multi-set
    selections (mgr_msel_count + mgr_scan + mgr_msel_pack)."""

    def __init__(self, dev, scratch=None):
        self.dev = dev
        self.scratch = scratch

    def _buf(self, name, nbytes):
        if self.scratch is not None:
            return self.scratch.get(name, nbytes)
        return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.dev)

    def take(self, name):
        """Buffer ``name`` leaves the scratch (a route owns it from here on)."""
        if self.scratch is not None:
            self.scratch.take(name)

    def msel_unpack_add(self, handle, acc_flat, elem, ncomp, srcs):
        """The inverse of msel_pack with an add (mgr_msel_unpack_add): for
        every set k with srcs[k] not None, in ascending order, the rows of
        ``acc_flat`` in the set += srcs[k]'s rows, in row order."""
        ptrs = (ctypes.c_void_p * handle.k)(*[None if t is None else t.data_ptr() for t in srcs])
        _lib.call("mgr_msel_unpack_add", _lib.ptr(acc_flat), int(elem), int(ncomp), *handle.args,
                  ptrs, _lib.stream_handle())

    def flags(self, pos_flat, n, ncols, code, dim, hi, lo):
        f = torch.empty(max(n, 1), dtype=torch.int16, device=self.dev)
        h = np.ascontiguousarray(hi, dtype=np.float64)
        l_ = np.ascontiguousarray(lo, dtype=np.float64)
        _lib.call("mgr_halo_flags", _lib.ptr(pos_flat), code, n, ncols, dim,
                  h.ctypes.data_as(ctypes.c_void_p), l_.ctypes.data_as(ctypes.c_void_p),
                  _lib.ptr(f), _lib.stream_handle())
        return f

    def msel(self, flags, n, bits, tag):
        """Counts of the sets {rows with flag bit bits[k]} -> (handle, device
        int64 counts [len(bits)])."""
        return self.msel_masks(flags, n, [1 << int(b) for b in bits], tag)

    def msel_masks(self, flags, n, masks, tag):
        """Counts of the sets {rows whose flags hold every bit of masks[k]}."""
        lib = _lib.load()
        tile_rows = SELECT_TILE_ROWS
        k = len(masks)
        ws = self._buf("msel_ws" + tag, int(lib.mgr_workspace_bytes(int(n), k, tile_rows)))
        counts = torch.empty(k, dtype=torch.int64, device=self.dev)
        cb = (ctypes.c_int * k)(*[int(m) for m in masks])
        s = _lib.stream_handle()
        _lib.call("mgr_msel_count", _lib.ptr(flags), n, k, cb, tile_rows, _lib.ptr(ws), s)
        _lib.alg_add("halo", 2 * n)                        # the flags, read once
        _lib.call("mgr_scan", n, k, tile_rows, _lib.ptr(ws), _lib.ptr(counts), s)
        return _Handle(n, flags, cb, k, ws, tile_rows), counts

    def msel_pack(self, handle, src_flat, row_bytes, dsts):
        """One field's selected rows: set k's rows, in row order, to dsts[k]
        (a flat uint8 tensor, or None: set k not written)."""
        ptrs = (ctypes.c_void_p * handle.k)(*[None if t is None else _lib.ptr(t) for t in dsts])
        _lib.call("mgr_msel_pack", _lib.ptr(src_flat), row_bytes, *handle.args, ptrs,
                  _lib.stream_handle())

    def msel_pack_fields(self, handle, srcs, row_bytes, dsts, rows_out=0):
        """Several fields (at most _lib.MSEL_MAX_FIELDS) of the same rows in
        one pass: dsts[f][k] as in msel_pack (field 0's None entries decide
        which sets are written).
        ``rows_out``: the rows the written sets hold (byte accounting)."""
        _lib.alg_add("halo_pack", 2 * handle.n + 2 * rows_out * sum(row_bytes))
        dp = (ctypes.c_void_p * (len(srcs) * handle.k))(*[None if t is None else _lib.ptr(t)
                                                          for row in dsts for t in row])
        _lib.call("mgr_msel_pack_fields", *_field_args(srcs, row_bytes), *handle.args, dp,
                  _lib.stream_handle())

    def msel_pack_placed(self, handle, srcs, row_bytes, dsts, cap_rows):
        """msel_pack_fields with the sets back to back from dsts[f] at the
        scan's set starts, rows beyond cap_rows not written: launched before
        the set sizes are known on the host."""
        dp = (ctypes.c_void_p * len(srcs))(*[_lib.ptr(t) for t in dsts])
        _lib.call("mgr_msel_pack_placed", *_field_args(srcs, row_bytes), *handle.args, dp,
                  int(cap_rows), _lib.stream_handle())

    def to_host(self, tensors):
        """One device->host read of several small int64 tensors (one sync)."""
        return self.to_host_wait(self.to_host_start(tensors))

    @staticmethod
    def to_host_start(tensors):
        return host_read_start(tensors)

    @staticmethod
    def to_host_wait(read):
        return host_read_wait(read)


class _Store:
    """The append-only overload store: per field (payload, positions when
    carried, flags) a flat tensor and the row where the overload rows start,
    the capacity in rows and the rows so far (``m``).  Built on ``arena`` (the
    flags field's store is always the exchange's own) or on nothing: the
    first ``ensure`` then allocates."""

    def __init__(self, rbs, dev, arena=None, multi=False, carry_pos=False):
        self.rbs, self.dev, self.m = rbs, dev, 0
        self.st, self.base, self.cap, self.in_arena = None, None, 0, False
        if arena is not None:
            self.cap, self.in_arena = arena[3], True
            self.st = _arena_stores(arena, multi, carry_pos) + [
                torch.empty(max(self.cap, 1) * 2, dtype=torch.uint8, device=dev)]
            self.base = [arena[2]] * (len(rbs) - 1) + [0]

    def rows(self, f, row0=0, rows=None):
        """Field f's store from overload row ``row0`` on (``rows`` rows of it)."""
        o = (self.base[f] + row0) * self.rbs[f]
        return self.st[f][o:] if rows is None else self.st[f][o:o + rows * self.rbs[f]]

    def ensure(self, new_m):
        """Room for new_m rows: outgrown, the rows so far move once to a store
        of the exchange's own with headroom."""
        if self.st is not None and new_m <= self.cap:
            return
        ncap = max(2 * new_m, 1024)
        nst = [torch.empty(ncap * rb, dtype=torch.uint8, device=self.dev) for rb in self.rbs]
        for f, rb in enumerate(self.rbs):
            if self.m:
                nst[f][: self.m * rb].copy_(self.rows(f, 0, self.m))
        self.st, self.base, self.cap, self.in_arena = nst, [0] * len(nst), ncap, False


class _LocalSends:
    """Where the local rows' sends are packed.  ``pieces[d]``: the rows this
    rank sends in dimension d to a (step 1) and to b (step 2), 0 for a side
    that does not send.  The sets of every dimension whose neighbours are
    other ranks are staged back to back in one buffer per field
    (``halo_local<f>``), so one pass packs them all; the sets of a self
    dimension go straight into the store, where the receives would land --
    dimension 0's in that first pass (its place is known), a later one's when
    that dimension comes (its place depends on the earlier receives)."""

    def __init__(self, sel, lh, srcs, rbs, nb, selfd, sent):
        self.sel, self.lh, self.srcs, self.rbs, self.selfd = sel, lh, srcs, rbs, selfd
        self.pieces = [(int(sent[2 * d]) if keep_a else 0, int(sent[2 * d + 1]) if keep_b else 0)
                       for d, (_, _, keep_a, keep_b) in enumerate(nb)]
        self.off, off = {}, 0
        for d, p in enumerate(self.pieces):
            if not selfd[d]:
                self.off[d] = off
                off += sum(p)
        self.buf = [sel._buf(f"halo_local{f}", off * rb) for f, rb in enumerate(rbs)]

    def staged(self, d, f, side):
        """Field f's staged rows of dimension d to a (side 0) or b (side 1)."""
        o = self.off[d] + (self.pieces[d][0] if side else 0)
        return self.buf[f][o * self.rbs[f]:(o + self.pieces[d][side]) * self.rbs[f]]

    def pack(self, dims, store=None, ia=0, ib=0):
        """One pass packing the sets of ``dims``; a self dimension among them
        lands in ``store``: step 1 (to a = me) at ib, step 2 (to b = me) at ia."""
        dsts = [[None] * (2 * len(self.pieces)) for _ in self.rbs]
        for d in dims:
            for f in range(len(self.rbs)):
                for side, at in enumerate((ib, ia)):
                    if self.pieces[d][side]:
                        dsts[f][2 * d + side] = store.rows(f, at, self.pieces[d][side]) \
                            if self.selfd[d] else self.staged(d, f, side)
        if any(t is not None for t in dsts[0]):
            self.sel.msel_pack_fields(self.lh, self.srcs, self.rbs, dsts,
                                      sum(sum(self.pieces[d]) for d in dims))


def _unwrap_step(R, d, box, store, f, pos_code, ncols, s):
    """The rows dimension d appended (field f: the positions), shifted to the
    image beside this cell: [ia, ib) came from a (+L on the last cell),
    [ib, ib + from_b) from b (-L on the first)."""
    rows = s.from_a + s.from_b
    up = box[d] if int(R.rank_cell_index[d]) == int(R.grid_topology[d]) - 1 else 0.0
    down = -box[d] if int(R.rank_cell_index[d]) == 0 else 0.0
    if rows and (up or down):
        e = [0.0] * R.dim
        shift_regions(store.rows(f, s.ia, rows), pos_code, ncols, R.dim, [s.from_a, rows],
                      [e[:d] + [up] + e[d + 1:], e[:d] + [down] + e[d + 1:]])


def exchange_overload(R, transport, data_flat, rbd, pos_flat, ncols, pos_code, n,
                      overload_lengths, periodic=True, sel=None, arena=None, flags=None,
                      pending=(), return_route=False, unwrap=False):
    """Overload rows of rank R (redist.py:202-309).  ``data_flat``: flat uint8
    tensor of this rank's n payload rows of ``rbd`` bytes; ``pos_flat``: their
    positions (n, ncols) rows of any position dtype (ncols >= dim), or None when the
    positions are not wanted back and ``flags`` is given.  ``flags``: the
    rows' face flags (int16 [n]) when the binning computed them, else one pass
    computes them from the positions here.  The overload buffer only grows at
    its end (concat(buffer, from_a, from_b), :305), so its rows live in an
    append-only store: ``arena`` = (data store, position store or None, first
    row, spare rows), e.g. the free tail of the redistribution's output, is
    used while the rows fit; beyond it the rows move once to a store of their
    own with headroom.  Returns (overload data flat, overload positions flat
    or None, rows, whether they stayed in the arena).  ``pending``: device
    count tensors of the caller whose check (check_counts) rides on this
    exchange's first host read.

    SoA payloads: ``data_flat`` and ``rbd`` may be lists, one entry per
    payload field (at most MAX_FIELDS); every field moves with the same
    selections -- one count and one pack launch per step for all of them,
    one message group per dimension.  ``arena[0]`` is then a list of stores
    and the returned overload data a list in the same order.

    ``return_route``: a HaloRoute for ``reduce_overload`` is appended to the
    result; every dimension's buffer selection then keeps a workspace of its
    own.  Without it the call allocates, copies and launches nothing more.

    ``unwrap``: the carried positions of the overload rows come back as the
    periodic image beside this rank's cell instead of the owner's coordinates
    (which image a copy is, is known only here: a grid extent of 1, or of 2
    with 2 * ol > cell, delivers the same row as a left and a right copy with
    identical position and flags).  General path: once dimension d's receives
    are posted, one mgr_shift_regions call on the rows just appended -- the
    rows from a get + box_length[d] on the last cell of the dimension, the
    rows from b get - box_length[d] on the first, a self dimension both --
    and later dimensions forward the shifted positions (their selections read
    the stored flags only).  One-rank path: one call over the pieces
    (_self_halo).  With ``periodic=False`` nothing is shifted.  Needs carried
    positions (ValueError) of float32 or float64 (TypeError); data rows,
    counts, order and the route are what ``unwrap=False`` gives, which
    launches nothing new."""
    dim = R.dim
    if unwrap:
        if pos_flat is None:
            raise ValueError("unwrap=True needs the positions carried (return_positions=True)")
        if pos_code not in (_lib.MGR_F32, _lib.MGR_F64):
            raise TypeError("unwrap=True: float32 or float64 positions (a shifted float16, "
                            "integer or bool position is not the row's image)")
    box = [float(x) for x in R.box_length] if unwrap else None
    assert len(overload_lengths) == dim, \
        "Overload lengths must be the same length as the dimensions"  # redist.py:245
    multi = isinstance(data_flat, (list, tuple))
    datas, rbds = (list(data_flat), list(rbd)) if multi else ([data_flat], [rbd])
    D = len(datas)                                        # payload fields
    if not 1 <= D == len(rbds) <= _lib.MAX_FIELDS:
        raise ValueError(f"1..{_lib.MAX_FIELDS} payload fields with their row bytes "
                         f"(got {D} and {len(rbds)})")
    dev = datas[0].device
    sel = sel or DeviceSelect(dev)
    carry_pos = pos_flat is not None
    if flags is None:
        hi, lo = thresholds(R, overload_lengths)
        flags = sel.flags(pos_flat, n, ncols, pos_code, dim, hi, lo)
    flags_flat = flags.reshape(-1).view(torch.uint8)[: 2 * n]
    isz = _lib.POS_ITEMSIZE[pos_code]
    srcs = datas + ([pos_flat] if carry_pos else []) + [flags_flat]
    rbs = rbds + ([ncols * isz] if carry_pos else []) + [2]
    F, FL = len(rbs), len(rbs) - 1                        # fields; the flags field

    me = transport.rank
    nb = [neighbours(R, d, periodic) for d in range(dim)]
    selfd = [a == me and b == me for a, b, _, _ in nb]
    if dim <= 3 and all(selfd) and all(ka and kb for _, _, ka, kb in nb):
        return _self_halo(transport, sel, srcs[:F - 1], rbs[:F - 1], flags, n, dim, carry_pos,
                          arena, dev, pending, multi, R if return_route else None,
                          (pos_code, ncols, box) if unwrap else None)
    for c in pending:   # (the general path reads them here)
        check_counts(c.cpu().numpy(), [])

    # 1. the local rows' counts of every dimension's two selections, one pass,
    # swapped with the neighbours of every dimension                (host sync 1)
    lh, lcount = sel.msel(flags, n, list(range(2 * dim)), "_local")
    sent, rl, failed = _swap_counts(transport, sel, dev, lcount, nb, False)
    # 2. the store, and the first pack of the local sends
    store = _Store(rbs, dev, arena, multi, carry_pos)
    local = _LocalSends(sel, lh, srcs, rbs, nb, selfd, sent)
    if selfd[0]:
        store.ensure(sum(local.pieces[0]))
    local.pack([d for d in range(dim) if not selfd[d] or d == 0], store, 0, local.pieces[0][1])

    steps = []                                            # per dimension, for the route
    for d, (a, b, _, _) in enumerate(nb):
        # 3. the buffer's selections for this dimension (rows received so far),
        # their counts swapped from d = 1 on              (host sync per dimension)
        m, gh, gcount = store.m, None, None
        gc = rg = (0, 0)
        if d > 0:
            if m:
                gh, gcount = sel.msel(store.rows(FL, 0, m).view(torch.int16), m, [2 * d, 2 * d + 1],
                                      f"_ghost{d}" if return_route else "_ghost")
            gc, rg, failed = _swap_counts(transport, sel, dev, gcount, [nb[d]], failed)
        # what it receives: from_b (step 1) and from_a (step 2), each a local
        # piece and a buffer piece of the sender, appended in place
        rlb, rla, rgb, rga = int(rl[2 * d]), int(rl[2 * d + 1]), int(rg[0]), int(rg[1])
        s = Step(*local.pieces[d], int(gc[0]), int(gc[1]), rla, rga, rlb, rgb,
                 ia=m, ib=m + rla + rga, m=m, gh=gh)
        store.ensure(s.end)
        if return_route:
            steps.append(s)
        if selfd[d] and d > 0:
            local.pack([d], store, s.ia, s.ib)
        gbuf, ng = None, s.nga + s.ngb
        if ng:   # the buffer's pieces: staged, or on a self dimension after the local ones
            if selfd[d]:
                gd = [[store.rows(f, s.ib + s.nla, s.nga) if s.nga else None,
                       store.rows(f, s.ia + s.nlb, s.ngb) if s.ngb else None] for f in range(F)]
            else:
                gbuf = [sel._buf(f"halo_ghost{f}", ng * rbs[f]) for f in range(F)]
                gd = [[gbuf[f][: s.nga * rbs[f]] if s.nga else None,
                       gbuf[f][s.nga * rbs[f]:ng * rbs[f]] if s.ngb else None] for f in range(F)]
            sel.msel_pack_fields(gh, [store.rows(f, 0, m) for f in range(F)], rbs, gd, ng)
        if not selfd[d]:
            _p2p(transport, _forward_group(s, d, a, b, store, local, gbuf))
        if unwrap and periodic:
            _unwrap_step(R, d, box, store, D, pos_code, ncols, s)
        store.m = s.end
    # one agreement per call: every rank raises together if any scan failed
    if transport.any_failed(failed):
        check_counts([-1], [])
    route = (["msel_ws_local"] + [f"msel_ws_ghost{d}" for d in range(dim)],
             dict(owner=R, n_local=n, flags=flags, lh=lh, nb=nb, selfd=selfd, steps=steps))
    return _result(sel, dev, (D, multi, carry_pos), [store.rows(f, 0, store.m) for f in range(FL)],
                   store.m, store.in_arena, route if return_route else None)


ELEM_BYTES = {_lib.MGR_ELEM_F32: 4, _lib.MGR_ELEM_F64: 8, _lib.MGR_ELEM_I32: 4,
              _lib.MGR_ELEM_I64: 8}


def reduce_overload(R, transport, route, local_acc, halo_vals, elem, ncomp, sel=None):
    """The halo exchange that made ``route``, backwards, with a sum: every
    value on an overload row is added onto the row it is a copy of, on the
    rank that owns it.  ``local_acc``: flat uint8 device tensor of
    route.n_local rows of ``ncomp`` elements of type ``elem`` (_lib.MGR_ELEM_*)
    -- the output, holding the owner's own values (or zeros) on entry;
    ``halo_vals``: the same for the route.n_halo overload rows, never written.
    All three may be lists, one entry per field: the fields then share every
    message group (one mgr_msel_unpack_add call per field and step).

    The dimensions go backwards, d = dim-1 .. 0, each step mirroring the
    forward one.  The halo values are copied once into a scratch store S; the
    rows S[ia : ia + rla + rga] a sent go back to a and S[ib : ...] to b --
    contiguous, nothing is packed -- while the values for this rank's own
    to_a sends (nla local + nga buffer rows) come back from a and for its to_b
    sends from b: the forward sizes with sender and receiver swapped, so no
    count message and no host sync.  Then two adds: onto ``local_acc`` with the
    local selection (sets 2d, 2d+1), onto S[0 : m_d] with the dimension's
    buffer selection.  The rows appended in dimension d - 1 have then absorbed
    what came through dimension d: corner and edge contributions reach the
    owner through the same chain of neighbours they were copied along.  A
    dimension whose neighbours are this rank sends nothing: the sources are
    the regions of S themselves.  A side that did not send (a non-periodic
    boundary) gets no source.  The one-rank path is one launch: piece k of
    ``halo_vals`` onto the rows of piece k's mask.

    Every row's adds come in a fixed order (dimension by dimension, within a
    launch by ascending set), so a result is bit-identical from run to run."""
    multi = isinstance(local_acc, (list, tuple))
    accs, vals = (list(local_acc), list(halo_vals)) if multi else ([local_acc], [halo_vals])
    elems = list(elem) if multi else [elem]
    ncomps = list(ncomp) if multi else [ncomp]
    ebs = [int(c) * ELEM_BYTES[e] for c, e in zip(ncomps, elems)]
    nf = len(accs)
    dev = accs[0].device
    sel = sel or DeviceSelect(dev)
    if route._self is not None:
        counts = route._self_counts
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if not counts.any():
            return
        for f in range(nf):
            srcs = [vals[f][int(offs[k]) * ebs[f]:] if counts[k] else None
                    for k in range(len(counts))]
            sel.msel_unpack_add(route._self, accs[f], elems[f], ncomps[f], srcs)
        return
    steps, dim = route._steps, len(route._steps)
    if not route.n_halo and not any(s.nla + s.nlb for s in steps):
        return
    nst = max([s.to_a + s.to_b for s in steps] + [1])
    S, stage = [], []
    for f in range(nf):
        S.append(sel._buf(f"halo_red_store{f}", route.n_halo * ebs[f]))
        S[f][: route.n_halo * ebs[f]].copy_(vals[f][: route.n_halo * ebs[f]])
        stage.append(sel._buf(f"halo_red_stage{f}", nst * ebs[f]))
    for d in range(dim - 1, -1, -1):
        s = steps[d]
        if not route._selfd[d]:
            _p2p(transport, _backward_group(s, route._nb[d][0], route._nb[d][1], S, stage, ebs))
        for f in range(nf):
            eb = ebs[f]
            if route._selfd[d]:   # step 1 (to a = me) landed at ib, step 2 at ia
                la, ga = S[f][s.ib * eb:], S[f][(s.ib + s.nla) * eb:]
                lb, gb = S[f][s.ia * eb:], S[f][(s.ia + s.nlb) * eb:]
            else:
                la, ga = stage[f], stage[f][s.nla * eb:]
                lb, gb = stage[f][s.to_a * eb:], stage[f][(s.to_a + s.nlb) * eb:]
            if s.nla or s.nlb:
                srcs = [None] * (2 * dim)
                srcs[2 * d], srcs[2 * d + 1] = (la if s.nla else None), (lb if s.nlb else None)
                sel.msel_unpack_add(route._lh, accs[f], elems[f], ncomps[f], srcs)
            if s.nga or s.ngb:
                sel.msel_unpack_add(s.gh, S[f][: s.m * eb], elems[f], ncomps[f],
                                    [ga if s.nga else None, gb if s.ngb else None])
