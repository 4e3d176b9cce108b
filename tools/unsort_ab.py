#!/usr/bin/env python3
"""A/B of the way back through the fine-cell sort (GPU, one process):
mgr_unpack_ranked_fields -- config 5's four value widths (12, 12, 4, 8 B) in
one launch, 2^26 rows, 512 uniform fine ids -- against two yardsticks of the
same run, on the same buffers, the three alternating:

  (a) the four mgr_pack_ranked launches that sorted the fields (the forward
      cost the unpack mirrors);
  (b) mgr_unpack_fields with the u16 ids as ``dest`` (nbins 512, the same tile
      rows and workspace): the only inverse there was before.

Each figure is the median over REPS blocks of ITERS launches (HIP events
around a block, after a warm-up); the spread is the blocks' min and max.
Algorithmic bytes per launch: rows * (2 * 36 + 4) (every row read and written
once, its id and rank read once).

Also one whole-call figure on one rank: redistribute_by_position +
fine_cell_sort + return_to_source(sort_route=) against the same three calls
with the values returned in arrival order (no sort route).

Writes one JSON file (default profiles/round8/unsort_ab.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpi_grid_redistribute_amd as mgr  # noqa: E402
from mpi_grid_redistribute_amd import _lib  # noqa: E402
from mpi_grid_redistribute_amd.redistributor import _i64s, _ptrs  # noqa: E402

RBS = [12, 12, 4, 8]
NBINS = 512


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def stat(t, nbytes):
    m = statistics.median(t)
    return {"median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_rel": round((max(t) - min(t)) / m, 4), "gb_per_s": round(nbytes / m / 1e6, 1)}


def kernels(n, reps, iters):
    lib = _lib.load()
    s = _lib.stream_handle()
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, NBINS, (n,), device="cuda", generator=g, dtype=torch.int16)
    srcs = [torch.randint(0, 256, (n * rb,), device="cuda", generator=g, dtype=torch.uint8)
            for rb in RBS]
    tr = int(lib.mgr_ranked_tile_rows(max(RBS), NBINS))
    T = (n + tr - 1) // tr
    ws = torch.empty(int(lib.mgr_workspace_bytes(n, NBINS, tr)), dtype=torch.uint8, device="cuda")
    ranks = torch.empty(2 * n + 16, dtype=torch.uint8, device="cuda")
    tstarts = torch.empty(8 * T * NBINS, dtype=torch.uint8, device="cuda")
    counts = torch.empty(NBINS, dtype=torch.int64, device="cuda")
    _lib.call("mgr_rank_ids", _lib.ptr(ids), n, NBINS, tr, _lib.ptr(ranks), _lib.ptr(tstarts),
              None, _lib.ptr(ws), s)
    _lib.call("mgr_scan", n, NBINS, tr, _lib.ptr(ws), _lib.ptr(counts), s)
    sorted_ = [torch.empty_like(t) for t in srcs]
    backs = [torch.empty_like(t) for t in srcs]
    backs_b = [torch.empty_like(t) for t in srcs]
    rb = _i64s(RBS)
    sp, bp, bbp = (_ptrs([t.data_ptr() for t in x]) for x in (sorted_, backs, backs_b))

    def pack4():
        for f, r in enumerate(RBS):
            _lib.call("mgr_pack_ranked", _lib.ptr(srcs[f]), r, n, _lib.ptr(ids), _lib.ptr(ranks),
                      _lib.ptr(tstarts), NBINS, tr, _lib.ptr(ws), _lib.ptr(sorted_[f]), s)

    def unpack_ranked():
        _lib.call("mgr_unpack_ranked_fields", 4, sp, rb, n, _lib.ptr(ids), _lib.ptr(ranks),
                  _lib.ptr(tstarts), NBINS, tr, _lib.ptr(ws), bp, s)

    def unpack_dest():
        _lib.call("mgr_unpack_fields", 4, sp, rb, n, _lib.ptr(ids), NBINS, -1, tr, _lib.ptr(ws),
                  bbp, -1, None, 0, -1, s)

    pack4()
    cands = [("pack_ranked_x4", pack4), ("unpack_ranked_fields", unpack_ranked)]
    try:
        unpack_dest()
        torch.cuda.synchronize()
        cands.append(("unpack_fields_u16_dest", unpack_dest))
        b_note = None
    except _lib.MgrError as e:
        b_note = f"mgr_unpack_fields refused these arguments: {e}"
    for _, fn in cands:                                # warm-up: code objects, caches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(reps):                              # alternating blocks
        for name, fn in cands:
            times[name].append(block_ms(fn, iters))
    for b, f in zip(backs, srcs):
        assert torch.equal(b, f), "unpack_ranked(pack_ranked(x)) != x"
    if b_note is None:
        for b, f in zip(backs_b, srcs):
            assert torch.equal(b, f), "unpack_fields(pack_ranked(x)) != x"
    nbytes = n * (2 * sum(RBS) + 4)
    res = {name: stat(t, nbytes) for name, t in times.items()}
    new = res["unpack_ranked_fields"]["median_ms"]
    res["unpack_ranked_over_pack_x4"] = round(new / res["pack_ranked_x4"]["median_ms"], 4)
    if b_note is None:
        res["unpack_ranked_over_unpack_fields"] = round(
            new / res["unpack_fields_u16_dest"]["median_ms"], 4)
    else:
        res["unpack_fields_u16_dest"] = b_note
    res.update(rows=n, row_bytes=RBS, nbins=NBINS, tile_rows=tr, reps=reps, iters=iters,
               bytes_per_launch=int(nbytes))
    return res


def whole_call(n, reps):
    """One rank: redistribute + fine_cell_sort + return, with the values coming
    back in sorted order (sort_route) against arrival order (host clock around
    work that ends in a device synchronise)."""
    soa = mgr.synth_wide_soa(n, seed=2)
    R = mgr.MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    fine = [8, 8, 8]

    def with_sort_route():
        loc, route = R.redistribute_by_position(soa, soa[0], return_route=True)
        srt, off, sroute = R.fine_cell_sort(loc, loc[0], fine, return_route=True)
        back = R.return_to_source(srt, route, sort_route=sroute)
        route.release()
        sroute.release()
        return back

    def without():
        loc, route = R.redistribute_by_position(soa, soa[0], return_route=True)
        R.fine_cell_sort(loc, loc[0], fine)
        back = R.return_to_source(loc, route)
        route.release()
        return back

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in (without, with_sort_route):
        fn()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(without))
        b.append(timed(with_sort_route))
    for x, y in zip(with_sort_route(), soa):
        assert torch.equal(x, y), "return_to_source(sort_route) != identity"
    ma, mb = statistics.median(a), statistics.median(b)
    return {"rows": n, "row_bytes": RBS, "fine_cells": fine, "reps": reps,
            "without_sort_route_ms": {"median": round(ma, 3), "min": round(min(a), 3),
                                      "max": round(max(a), 3)},
            "with_sort_route_ms": {"median": round(mb, 3), "min": round(min(b), 3),
                                   "max": round(max(b), 3)},
            "ratio": round(mb / ma, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--whole-rows", type=int, default=1 << 25)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "round8", "unsort_ab.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels(a.rows, a.reps, a.iters)}
    torch.cuda.empty_cache()
    if a.whole_rows > 0:
        res["whole_call_one_rank"] = whole_call(a.whole_rows, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
