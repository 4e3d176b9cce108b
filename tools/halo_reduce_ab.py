#!/usr/bin/env python3
"""Halo return-path A/B (GPU, one process): mgr_msel_unpack_add next to
mgr_msel_pack over the same flags and workspace, alternating, the forward
selection pack of the same run being the yardstick (it moves the same selected
rows and is not the code under test).

  * config 3's halo density: the 6 face sets at about 10 % each, 16M rows,
    float32 with ncomp = 3 -- against mgr_msel_pack of a 12-byte field;
  * one whole-call figure on one rank: exchange_overload_by_position(
    return_route=True) + reduce_overload against the forward call alone.

Each kernel figure is the median over REPS blocks of ITERS launches (HIP
events around a block, after a warm-up), the blocks of the two kernels
alternating; the spread is the blocks' min and max.  Algorithmic bytes of the
add: 2 n flag bytes + per selected row (read acc + write acc + read src), a
row in several sets counting its accumulator once; of the pack: 2 n + per
selected row (read + write).  Writes one JSON file (default
profiles/halo_reduce/halo_reduce_ab.json) and prints it."""
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
from mpi_grid_redistribute_amd.halo import DeviceSelect  # noqa: E402


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
            "gb_per_s": round(nbytes / m / 1e6, 1), "bytes_per_launch": int(nbytes)}


def kernels(n, reps, iters):
    g = torch.Generator(device="cuda").manual_seed(3)
    flags = torch.zeros(n, dtype=torch.int16, device="cuda")
    for d in range(3):   # each face about 10 %, the two faces of a dimension exclusive
        u = torch.rand(n, generator=g, device="cuda")
        flags |= (u >= 0.9).to(torch.int16) << (2 * d)
        flags |= (u < 0.1).to(torch.int16) << (2 * d + 1)
    sel = DeviceSelect(torch.device("cuda", 0))
    masks = [1 << b for b in range(6)]
    handle, counts = sel.msel_masks(flags, n, masks, "")
    cnt = counts.cpu().numpy()
    selected = int(cnt.sum())
    touched = int((flags != 0).sum())
    src = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float32)
    packed = [torch.empty(max(int(c), 1) * 12, dtype=torch.uint8, device="cuda") for c in cnt]
    acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    srcf, accf = src.view(-1).view(torch.uint8), acc.view(-1).view(torch.uint8)
    pack = lambda: sel.msel_pack(handle, srcf, 12, packed)  # noqa: E731
    add = lambda: sel.msel_unpack_add(handle, accf, _lib.MGR_ELEM_F32, 3, packed)  # noqa: E731
    pack()
    add()
    torch.cuda.synchronize()
    # the inverse with an add: every row comes back once per set that holds it
    times = sum(((flags >> b) & 1) for b in range(6)).to(torch.float32)
    assert torch.equal(acc, src * times[:, None]), "unpack_add(pack(x)) != x * sets"
    for fn in (pack, add):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    tp, ta = [], []
    for _ in range(reps):
        tp.append(block_ms(pack, iters))
        ta.append(block_ms(add, iters))
    p = stat(tp, 2 * n + selected * 24)
    a = stat(ta, 2 * n + touched * 24 + selected * 12)
    return {"rows": n, "sets": 6, "selected_rows": selected, "touched_rows": touched,
            "set_fraction": [round(float(c) / n, 4) for c in cnt], "elem": "float32", "ncomp": 3,
            "msel_pack_12B": p, "msel_unpack_add": a,
            "add_over_pack": round(a["median_ms"] / p["median_ms"], 4),
            "spread_rel": round(max((p["max_ms"] - p["min_ms"]) / p["median_ms"],
                                    (a["max_ms"] - a["min_ms"]) / a["median_ms"]), 4),
            "reps": reps, "iters": iters}


def whole_call(n, reps, calls):
    """One rank (the 26-piece self path): forward + reduce against the forward
    call alone.  A sample is ``calls`` calls back to back under a host clock,
    ending in a device synchronise (one call is well under a millisecond: a
    single call per sample would mostly measure host and launch jitter); the
    figure is the sample's time per call."""
    g = torch.Generator(device="cuda").manual_seed(4)
    pos = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64)
    data = torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float32)
    R = mgr.MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    ol = [0.05] * 3

    def forward():
        return R.exchange_overload_by_position(data, pos, ol)

    def forward_reduce():
        h, route = R.exchange_overload_by_position(data, pos, ol, return_route=True)
        out = R.reduce_overload(h, route)
        route.release()
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    for fn in (forward, forward_reduce):
        fn()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(forward))
        b.append(timed(forward_reduce))
    ma, mb = statistics.median(a), statistics.median(b)
    return {"rows": n, "halo_rows": int(len(forward())), "overload": ol, "reps": reps,
            "calls_per_sample": calls,
            "forward_ms": {"median": round(ma, 3), "min": round(min(a), 3), "max": round(max(a), 3)},
            "forward_plus_reduce_ms": {"median": round(mb, 3), "min": round(min(b), 3),
                                       "max": round(max(b), 3)},
            "ratio": round(mb / ma, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--whole-rows", type=int, default=1 << 24)
    ap.add_argument("--whole-calls", type=int, default=20, help="calls per whole-call sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out",
                    default=os.path.join("profiles", "halo_reduce", "halo_reduce_ab.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"device": torch.cuda.get_device_name(0), "kernels": kernels(a.rows, a.reps, a.iters)}
    torch.cuda.empty_cache()
    if a.whole_rows > 0:
        res["whole_call_one_rank"] = whole_call(a.whole_rows, a.reps, a.whole_calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
