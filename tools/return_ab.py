#!/usr/bin/env python3
"""Return-path A/B (GPU, one process): mgr_unpack next to mgr_pack on the same
buffers, alternating, the pack of the same run being the yardstick.

  * config 2's shape: 2^26 rows x 32 B, 2x2x2, f64 positions -- mgr_pack
    (records -> packed) against mgr_unpack (packed -> records' order);
  * config 5's four arrays (pos f32 x3, vel f32 x3, mass f32, id i64) --
    mgr_pack_fields against mgr_unpack_fields;
  * one whole-call figure on one rank: redistribute_by_position(return_route)
    + return_to_source against two forward calls, 125M rows x 32 B.

Each kernel figure is the median over REPS blocks of ITERS launches (HIP
events around a block, after a warm-up), the blocks of the two kernels
alternating; the spread is the blocks' min and max.  Both kernels move the
same bytes per row: row_bytes read + row_bytes written + the destination byte.
Writes one JSON file (default profiles/round7/return_ab.json) and prints it."""
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


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def ab(pack, unpack, reps, iters, bytes_per_launch):
    for fn in (pack, unpack):                      # warm-up: code objects, caches
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tp, tu = [], []
    for _ in range(reps):                          # alternating blocks
        tp.append(block_ms(pack, iters))
        tu.append(block_ms(unpack, iters))

    def stat(t):
        m = statistics.median(t)
        return {"median_ms": round(m, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                "gb_per_s": round(bytes_per_launch / m / 1e6, 1)}

    p, u = stat(tp), stat(tu)
    return {"pack": p, "unpack": u, "unpack_over_pack": round(u["median_ms"] / p["median_ms"], 4),
            "spread_rel": round(max((p["max_ms"] - p["min_ms"]) / p["median_ms"],
                                    (u["max_ms"] - u["min_ms"]) / u["median_ms"]), 4),
            "reps": reps, "iters": iters, "bytes_per_launch": int(bytes_per_launch)}


def kernels_cfg2(n, reps, iters):
    pos, rec = mgr.synth_uniform(n, seed=1)
    P = mgr.GridPartitioner([2, 2, 2], [1.0] * 3)
    data = rec.reshape(-1)
    out, _ = P.partition_device(data, 32, pos)
    tile_rows, ws, dest = P._cache[P._last_part][:3]
    back = torch.empty_like(data)
    s = _lib.stream_handle()
    args = (32, n, _lib.ptr(dest), 8, -1, tile_rows, _lib.ptr(ws))
    pack = lambda: _lib.call("mgr_pack", _lib.ptr(data), *args, _lib.ptr(out), -1, None, s)  # noqa: E731
    unpack = lambda: _lib.call("mgr_unpack", _lib.ptr(out), *args, _lib.ptr(back), -1, None, s)  # noqa: E731
    r = ab(pack, unpack, reps, iters, n * 65)
    assert torch.equal(back, data), "unpack(pack(x)) != x"
    r.update(rows=n, row_bytes=32, tile_rows=int(tile_rows), bins=8)
    return r


def kernels_cfg5(n, reps, iters):
    soa = mgr.synth_wide_soa(n, seed=1)
    rbs = [12, 12, 4, 8]
    flats = [t.reshape(-1).view(torch.uint8) for t in soa]
    P = mgr.GridPartitioner([2, 2, 2], [1.0] * 3)
    outs, _ = P.partition_fields_device(flats, rbs, soa[0])
    tile_rows, ws, dest = P._cache[P._last_part][:3]
    backs = [torch.empty_like(f) for f in flats]
    s = _lib.stream_handle()
    fp, op, bp = (_ptrs([t.data_ptr() for t in x]) for x in (flats, outs, backs))
    rb = _i64s(rbs)
    args = (n, _lib.ptr(dest), 8, -1, tile_rows, _lib.ptr(ws))
    pack = lambda: _lib.call("mgr_pack_fields", 4, fp, rb, *args, op, -1, None, None, None, None,  # noqa: E731
                             0, -1, s)
    unpack = lambda: _lib.call("mgr_unpack_fields", 4, op, rb, *args, bp, -1, None, 0, -1, s)  # noqa: E731
    r = ab(pack, unpack, reps, iters, n * (2 * sum(rbs) + 1))
    for b, f in zip(backs, flats):
        assert torch.equal(b, f), "unpack_fields(pack_fields(x)) != x"
    r.update(rows=n, row_bytes=rbs, tile_rows=int(tile_rows), bins=8)
    return r


def whole_call(n, reps):
    """One rank: forward + return against two forward calls (host clock around
    work that ends in a device synchronise)."""
    pos, rec = mgr.synth_uniform(n, seed=2)
    R = mgr.MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)

    def two_forward():
        R.redistribute_by_position(rec, pos)
        R.redistribute_by_position(rec, pos)

    def forward_back():
        loc, route = R.redistribute_by_position(rec, pos, return_route=True)
        R.return_to_source(loc, route)
        route.release()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in (two_forward, forward_back):
        fn()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(two_forward))
        b.append(timed(forward_back))
    loc, route = R.redistribute_by_position(rec, pos, return_route=True)
    assert torch.equal(R.return_to_source(loc, route), rec), "return_to_source != identity"
    ma, mb = statistics.median(a), statistics.median(b)
    return {"rows": n, "row_bytes": 32, "reps": reps,
            "two_forward_ms": {"median": round(ma, 3), "min": round(min(a), 3), "max": round(max(a), 3)},
            "forward_plus_return_ms": {"median": round(mb, 3), "min": round(min(b), 3),
                                       "max": round(max(b), 3)},
            "ratio": round(mb / ma, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--whole-rows", type=int, default=125_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "round7", "return_ab.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0),
           "config2_32B": kernels_cfg2(a.rows, a.reps, a.iters)}
    torch.cuda.empty_cache()
    res["config5_soa"] = kernels_cfg5(a.rows, a.reps, a.iters)
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
