#!/usr/bin/env python3
"""Cell lists beyond 1024 cells, measured (GPU, one process, one rank).

16,777,216 rows uniform in the unit box: float32 x 3 positions and a 36-byte
record per row, no halo (n_local = n, overload 0), so every variant sorts the
same two arrays.

  (a) ghost_cell_sort at 10^3 cells: the 16-bit path (one ranked sort).
  (b) the wide sort at 24^3 and 66^3 cells, with both digit splits
      (sort.WIDE_SPLIT = "balanced" / "low10").
  (c) what a caller does without it: torch.argsort(ids, stable=True), one
      index_select per field, torch.searchsorted for the offsets (the ids
      taken as given: mgr_ghost_cells_wide's, not timed).
  (d) the three new kernels alone, with their bytes per row against 8 TB/s.

Whole calls: the median over REPS blocks of WHOLE_ITERS calls (HIP events
around a block, after a warm-up), the variants' blocks alternating inside a
repetition; kernels: blocks of ITERS launches.  Writes one JSON file (default
profiles/wide_cells/wide_cells_ab.json) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpi_grid_redistribute_amd as mgr  # noqa: E402
from mpi_grid_redistribute_amd import _lib, sort  # noqa: E402

PEAK_GBS = 8000.0


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(t, nbytes=None):
    m = statistics.median(t)
    out = {"median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    if nbytes is not None:
        out.update(bytes_per_launch=int(nbytes), gb_per_s=round(nbytes / m / 1e6, 1),
                   fraction_of_8TBs=round(nbytes / m / 1e6 / PEAK_GBS, 4))
    return out


def alternate(fns, reps, iters):
    """{name: summary}: every repetition runs one block of each variant, in
    turn, after a warm-up of each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(block_ms(fn, iters))
    return {k: summary(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--whole-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "wide_cells", "wide_cells_ab.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    n = a.rows
    rec, _ = mgr.synth_wide(n, seed=5)
    pos = rec.view(torch.float32)[:, :3].contiguous()
    R = mgr.MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    zero = [0.0] * 3
    res = {"device": torch.cuda.get_device_name(0), "rows": n, "reps": a.reps, "iters": a.iters,
           "whole_iters": a.whole_iters, "payload_bytes_per_row": 36 + 12}

    def wide(fine, split):
        def fn():
            sort.WIDE_SPLIT = split
            R.ghost_cell_sort((rec, pos), pos, n, [fine] * 3, zero, max_cells=mgr.CELLS_MAX)
        return fn

    def ids_of(fine):
        ids = torch.empty(n, dtype=torch.int32, device="cuda")
        ghost, ext, origin, width = R.ghost_grid([fine] * 3, zero, max_cells=mgr.CELLS_MAX)
        args = (origin.ctypes.data_as(ctypes.c_void_p), width.ctypes.data_as(ctypes.c_void_p),
                (ctypes.c_int * 3)(fine, fine, fine), (ctypes.c_int * 3)(0, 0, 0))

        def cells():
            _lib.call("mgr_ghost_cells_wide", _lib.ptr(pos), _lib.MGR_F32, n, n, 3, 3, *args,
                      _lib.ptr(ids), None, _lib.stream_handle())
        cells()
        return ids, cells

    def torch_way(ids, ncells):
        cells = torch.arange(ncells + 1, device="cuda", dtype=torch.int32)

        def fn():
            order = torch.argsort(ids, stable=True)
            a_ = rec.index_select(0, order)
            b_ = pos.index_select(0, order)
            offs = torch.searchsorted(ids.index_select(0, order), cells)
            return a_, b_, offs
        return fn

    default_split = sort.WIDE_SPLIT
    for fine in (24, 66):
        ids, cells = ids_of(fine)
        fns = {"small_10^3": lambda: R.ghost_cell_sort((rec, pos), pos, n, [10] * 3, zero),
               "wide_balanced": wide(fine, "balanced"), "wide_low10": wide(fine, "low10"),
               "torch_argsort_gather_searchsorted": torch_way(ids, fine ** 3)}
        r = alternate(fns, a.reps, a.whole_iters)
        r["digit_split_balanced"] = sort._digit_split(fine ** 3, "balanced")
        r["digit_split_low10"] = sort._digit_split(fine ** 3, "low10")
        sort.WIDE_SPLIT = default_split
        # (d) the kernels alone
        dig = torch.empty(n, dtype=torch.int16, device="cuda")
        sids = torch.sort(ids)[0]
        offs = torch.empty(fine ** 3 + 1, dtype=torch.int64, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        s = _lib.stream_handle()
        kern = {
            "ghost_cells_wide": (cells, n * (12 + 4)),
            "id_digit": (lambda: _lib.call("mgr_id_digit", _lib.ptr(ids), n, 0, 10, _lib.ptr(dig), s),
                         n * (4 + 2)),
            "cell_offsets": (lambda: _lib.call("mgr_cell_offsets", _lib.ptr(sids), n, fine ** 3,
                                               _lib.ptr(offs), _lib.ptr(bad), s),
                             n * 4 + (fine ** 3 + 1) * 8),
        }
        for k, (fn, nbytes) in kern.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            r[k] = summary([block_ms(fn, a.iters) for _ in range(a.reps)], nbytes)
            r[k]["bytes_per_row"] = round(nbytes / n, 2)
        assert int(bad.item()) == 0
        res[f"{fine}^3"] = r
        del ids, dig, sids, offs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
