"""Plain numpy model of the stable pack (mgr_pack / mgr_pack_ids / mgr_pack_tiles /
mgr_pack_fields) and of mgr_tile_offsets: what every output buffer must hold,
byte for byte, for a given set of options.  No GPU, no library: the reference
the kernel tests compare against (tests/test_gpu_pack_matrix.py), itself
checked against the C oracle in tests/test_pack_model_cpu.py.

Everything is computed in int64 with np.argsort(kind="stable") and np.bincount.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def _as_rows(a, n):
    """A field as an (n, row_bytes) uint8 array."""
    a = np.ascontiguousarray(a)
    if a.shape[0] != n:
        raise ValueError(f"field of {a.shape[0]} rows for {n} destinations")
    row_bytes = a.itemsize * int(np.prod(a.shape[1:], dtype=np.int64))
    return np.frombuffer(a.tobytes(), dtype=np.uint8).reshape(n, row_bytes)


def bin_layout(dest, nbins):
    """(counts, bin_start, rank): per-bin row counts, their exclusive prefix
    (nbins + 1 entries) and, per row, the number of rows of its bin before it."""
    dest = np.asarray(dest, dtype=np.int64).reshape(-1)
    n = dest.size
    if n and (dest.min() < 0 or dest.max() >= nbins):
        raise ValueError("dest outside [0, nbins)")
    counts = np.bincount(dest, minlength=nbins).astype(np.int64)
    bin_start = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)])
    order = np.argsort(dest, kind="stable")
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n, dtype=np.int64) - bin_start[dest[order]]
    return counts, bin_start, rank


@dataclass
class PackResult:
    """Whole buffers after one pack call, as (rows, row_bytes) uint8 arrays
    pre-filled with the sentinel: ``dst[f]`` has n rows, ``red[f]`` as many rows
    as the redirect bin holds (none without a redirect); ``ids_dst`` /
    ``ids_red`` likewise with 2-byte rows (None without side ids).
    ``dst_written`` / ``red_written``: the rows (slots) this call wrote."""
    dst: list
    red: list
    ids_dst: np.ndarray | None
    ids_red: np.ndarray | None
    dst_written: np.ndarray
    red_written: np.ndarray
    counts: np.ndarray = field(repr=False, default=None)
    bin_start: np.ndarray = field(repr=False, default=None)

    def buffers(self):
        """[(name, array)] of every buffer, ids included."""
        out = [(f"dst{f}", a) for f, a in enumerate(self.dst)]
        out += [(f"red{f}", a) for f, a in enumerate(self.red)]
        if self.ids_dst is not None:
            out += [("ids_dst", self.ids_dst), ("ids_red", self.ids_red)]
        return out

    def over(self, prev):
        """The buffers after this call ran on buffers holding ``prev`` (an
        earlier call's state, or None: sentinel): this call's rows replace
        what was there, everything else stays."""
        if prev is None:
            return self
        m = lambda new, old, w: np.where(w[:, None], new, old)  # noqa: E731
        ids = self.ids_dst is not None
        return PackResult(
            dst=[m(a, b, self.dst_written) for a, b in zip(self.dst, prev.dst)],
            red=[m(a, b, self.red_written) for a, b in zip(self.red, prev.red)],
            ids_dst=m(self.ids_dst, prev.ids_dst, self.dst_written) if ids else None,
            ids_red=m(self.ids_red, prev.ids_red, self.red_written) if ids else None,
            dst_written=self.dst_written | prev.dst_written,
            red_written=self.red_written | prev.red_written,
            counts=self.counts, bin_start=self.bin_start)


def pack_model(fields, dest, nbins, drop_bin=-1, redirect_bin=-1, tile_rows=64, tile_begin=0,
               tile_end=-1, ids=None, sentinel=0xAB):
    """The buffers after packing the rows of the tiles [tile_begin, tile_end)
    (tile_end < 0: every tile) into sentinel-filled buffers.

    Row r of bin b goes to slot bin_start[b] + (rows of bin b before r); for
    b > redirect_bin the redirect bin's count is subtracted (the gap closes);
    for b == redirect_bin the slot is in the redirect buffer, minus
    bin_start[b]; rows of drop_bin are not written.  Only the rows
    [tile_begin * tile_rows, min(n, tile_end * tile_rows)) are written.
    ``fields``: arrays sharing axis 0 (any dtype, moved as opaque bytes);
    ``ids``: the optional 2-byte side field."""
    dest = np.asarray(dest, dtype=np.int64).reshape(-1)
    n = int(dest.size)
    counts, bin_start, rank = bin_layout(dest, nbins)
    T = (n + tile_rows - 1) // tile_rows
    if tile_end is None or tile_end < 0:
        tile_begin, tile_end = 0, T
    lo = np.int64(tile_begin) * tile_rows
    hi = min(np.int64(n), np.int64(tile_end) * tile_rows)
    r = np.arange(n, dtype=np.int64)
    live = (r >= lo) & (r < hi) & (dest != drop_bin)
    slot = bin_start[dest] + rank
    nred = 0
    to_red = np.zeros(n, dtype=bool)
    if redirect_bin >= 0:
        nred = int(counts[redirect_bin])
        to_red = dest == redirect_bin
        slot = np.where(dest > redirect_bin, slot - nred, slot)
        slot = np.where(to_red, slot - bin_start[redirect_bin], slot)
    d_rows, d_slots = r[live & ~to_red], slot[live & ~to_red]
    r_rows, r_slots = r[live & to_red], slot[live & to_red]
    dst_written = np.zeros(n, dtype=bool)
    red_written = np.zeros(nred, dtype=bool)
    dst_written[d_slots] = True
    red_written[r_slots] = True

    def place(a):
        rows = _as_rows(a, n)
        rb = rows.shape[1]
        d = np.full((n, rb), sentinel, dtype=np.uint8)
        q = np.full((nred, rb), sentinel, dtype=np.uint8)
        d[d_slots] = rows[d_rows]
        q[r_slots] = rows[r_rows]
        return d, q

    placed = [place(f) for f in fields]
    idd = idr = None
    if ids is not None:
        idd, idr = place(np.ascontiguousarray(np.asarray(ids).reshape(n)).view(np.uint16))
    return PackResult(dst=[p[0] for p in placed], red=[p[1] for p in placed], ids_dst=idd,
                      ids_red=idr, dst_written=dst_written, red_written=red_written,
                      counts=counts, bin_start=bin_start)


def tile_offsets_model(dest, nbins, tile_rows, tiles):
    """out[i][b] = bin_start[b] + the rows of bin b among the rows before tile
    tiles[i] -- absolute slots, no redirect gap (tile_offsets_kernel)."""
    dest = np.asarray(dest, dtype=np.int64).reshape(-1)
    n = int(dest.size)
    _, bin_start, _ = bin_layout(dest, nbins)
    out = np.empty((len(tiles), nbins), dtype=np.int64)
    for i, t in enumerate(tiles):
        upto = min(np.int64(n), np.int64(t) * tile_rows)
        out[i] = bin_start[:nbins] + np.bincount(dest[:upto], minlength=nbins)
    return out
