#!/usr/bin/env python3
"""Ghost-cell list measurements (GPU, one process, one rank): the two new
kernels and the whole ``ghost_cell_sort`` beside the ``bin_fine`` kernel and
``fine_cell_sort`` of the same row count and box.

Config 3's halo density: 16,777,216 owned rows uniform in the unit box, ol =
0.05 (about 5.5M overload rows through the 26-piece one-rank halo), float32 x 3
and float64 x 3 positions, which are also the payload; 8 x 8 x 8 fine cells, so
the extended grid is 10 x 10 x 10.

  * mgr_shift_regions : the halo's own call, 26 regions with the pieces'
    shifts, on the overload rows' positions.  Bytes: every shifted coordinate
    read and written (zero-shift coordinates are neither).
  * mgr_ghost_cells   : owned + overload rows.  Bytes: the positions read plus
    2 B/row written.
  * ghost_cell_sort   : the whole call on device tensors (ids, ranked sort,
    offsets); beside it fine_cell_sort on as many rows inside the box, and the
    bin_fine kernel of that call from the library's profiler.

Kernel figures: the median over REPS blocks of ITERS launches (HIP events
around a block, after a warm-up); whole calls the same with fewer launches per
block.  Writes one JSON file (default profiles/ghost_cells/ghost_ab.json) and
prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpi_grid_redistribute_amd as mgr  # noqa: E402
from mpi_grid_redistribute_amd import _lib  # noqa: E402
from mpi_grid_redistribute_amd.halo import self_halo_pieces, shift_regions  # noqa: E402

PEAK_GBS = 8000.0


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure(fn, reps, iters, nbytes=None):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = [block_ms(fn, iters) for _ in range(reps)]
    m = statistics.median(t)
    out = {"median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    if nbytes is not None:
        out.update(bytes_per_launch=int(nbytes), gb_per_s=round(nbytes / m / 1e6, 1),
                   fraction_of_8TBs=round(nbytes / m / 1e6 / PEAK_GBS, 4))
    return out


def run(dt, n, reps, iters, whole_iters):
    g = torch.Generator(device="cuda").manual_seed(5)
    pos = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64).to(dt)
    isz = pos.element_size()
    code = _lib.MGR_F32 if dt == torch.float32 else _lib.MGR_F64
    R = mgr.MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    ol, fine = [0.05] * 3, [8, 8, 8]
    h, p = R.exchange_overload_by_position(pos, pos, ol, return_positions=True, unwrap=True)
    nh = int(p.shape[0])
    res = {"owned_rows": n, "overload_rows": nh, "position_bytes": 3 * isz}

    # the halo's shift call: 26 regions, the pieces' shifts
    pieces = self_halo_pieces(3)
    ends = [nh * (k + 1) // len(pieces) for k in range(len(pieces))]
    shifts = [[(-1.0 if m >> (2 * d) & 1 else 0.0) + (1.0 if m >> (2 * d + 1) & 1 else 0.0)
               for d in range(3)] for m in pieces]
    moved, b = 0, 0
    for e, s in zip(ends, shifts):
        moved += (e - b) * sum(1 for v in s if v)
        b = e
    scratch = p.clone()
    sflat = scratch.view(-1).view(torch.uint8)
    res["shift_regions"] = measure(lambda: shift_regions(sflat, code, 3, 3, ends, shifts), reps,
                                   iters, 2 * moved * isz)
    res["shift_regions"]["all_position_bytes_rw"] = 2 * nh * 3 * isz
    del scratch, sflat

    # the binning over owned + overload rows
    both = torch.cat([pos, p])
    nt = int(both.shape[0])
    ghost, ext, origin, width = R.ghost_grid(fine, ol)
    ids = torch.empty(nt, dtype=torch.int16, device="cuda")
    outside = torch.zeros(1, dtype=torch.int32, device="cuda")
    fi = (ctypes.c_int * 3)(*fine)
    gi = (ctypes.c_int * 3)(*[int(x) for x in ghost])

    def cells():
        _lib.call("mgr_ghost_cells", _lib.ptr(both), code, nt, n, 3, 3,
                  origin.ctypes.data_as(ctypes.c_void_p), width.ctypes.data_as(ctypes.c_void_p),
                  fi, gi, _lib.ptr(ids), _lib.ptr(outside), _lib.stream_handle())

    res["ghost_cells"] = measure(cells, reps, iters, nt * (3 * isz + 2))
    assert int(outside.item()) == 0
    res["rows_sorted"] = nt
    res["extents"] = [int(x) for x in ext]
    del ids

    res["ghost_cell_sort"] = measure(lambda: R.ghost_cell_sort(both, both, n, fine, ol), reps,
                                     whole_iters)
    # the yardsticks: the parent's fine sort on as many rows inside the box
    inbox = torch.rand((nt, 3), generator=g, device="cuda", dtype=torch.float64).to(dt)
    del both, p, h
    res["fine_cell_sort"] = measure(lambda: R.fine_cell_sort(inbox, inbox, fine), reps,
                                    whole_iters)
    _lib.profile_enable(True)
    _lib.profile_select(["bin_fine"])
    _lib.profile_reset()
    for _ in range(reps * whole_iters):
        R.fine_cell_sort(inbox, inbox, fine)
    torch.cuda.synchronize()
    ms, cnt = _lib.profile_read("bin_fine")
    _lib.profile_enable(False)
    _lib.profile_select(None)
    nb = nt * (3 * isz + 2)
    res["bin_fine"] = {"mean_ms": round(ms / max(cnt, 1), 4), "launches": int(cnt),
                       "bytes_per_launch": nb,
                       "gb_per_s": round(nb / (ms / max(cnt, 1)) / 1e6, 1),
                       "fraction_of_8TBs": round(nb / (ms / max(cnt, 1)) / 1e6 / PEAK_GBS, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--whole-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "ghost_cells", "ghost_ab.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "iters": a.iters,
           "whole_iters": a.whole_iters}
    for name, dt in (("float32", torch.float32), ("float64", torch.float64)):
        res[name] = run(dt, a.rows, a.reps, a.iters, a.whole_iters)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
