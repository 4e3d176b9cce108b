#!/usr/bin/env python3
"""SoA source-side A/B (GPU): config 5's four arrays (2^26 rows of
synth_wide_soa: pos f32 x3, vel f32 x3, mass f32, id i64), 2x2x2 destinations,
fine cells 8x8x8, write-back "all", partitioned by
  (a) twopass -- mgr_bin_count_fine + mgr_scan + mgr_pack_fields
                 (GridPartitioner.partition_fields_device, the bench's SoA
                 config-5 source step), and
  (b) onepass -- mgr_partition_onepass_fields
                 (GridPartitioner.partition_onepass_fields_device),
in ONE process: first every bin region and the fine ids of (b) are compared,
byte for byte, with (a)'s output; then AB_ROUNDS alternating rounds, each side
timed with HIP events over AB_ITERS calls after a warm-up.  Prints one JSON
line (medians and ranges over the rounds, the one-pass kernel's bytes per row
and its fraction of 8 TB/s) and, with AB_OUT, writes it to that file.
AB_ONLY=twopass|onepass runs just that side AB_ITERS times, untimed (for a
hardware-counter pass of its own)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpi_grid_redistribute_amd as mgr  # noqa: E402

N = int(os.environ.get("AB_N", 1 << 26))
ITERS = int(os.environ.get("AB_ITERS", 10))
ROUNDS = int(os.environ.get("AB_ROUNDS", 3))
RBS = [12, 12, 4, 8]
FINE = [8, 8, 8]
HBM_BPS = 8e12


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / ITERS


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
            "max_ms": round(max(xs), 4), "range_ms": round(max(xs) - min(xs), 4),
            "rounds_ms": [round(x, 4) for x in xs]}


def main():
    soa = mgr.synth_wide_soa(N, seed=1)
    flats = [t.reshape(-1).view(torch.uint8) for t in soa]
    A = mgr.GridPartitioner([2, 2, 2], [1.0] * 3)   # one partitioner per side: each keeps
    B = mgr.GridPartitioner([2, 2, 2], [1.0] * 3)   # its own cached buffers
    A.set_write_back("all")
    B.set_write_back("all")

    def twopass():
        return A.partition_fields_device(flats, RBS, soa[0], fine_cells=FINE)

    def onepass():
        return B.partition_onepass_fields_device(flats, RBS, soa[0], fine_cells=FINE)

    only = os.environ.get("AB_ONLY")
    if only:
        fn = {"twopass": twopass, "onepass": onepass}[only]
        for _ in range(ITERS):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"only": only, "n": N, "calls": ITERS}), flush=True)
        return

    # the new path's regions == the two-pass output, byte for byte
    outs_a, fid_a, cnt_a = twopass()
    outs_b, fid_b, cnt_b, cap = onepass()
    torch.cuda.synchronize()
    ca, cb = cnt_a.cpu().tolist(), cnt_b.cpu().tolist()
    equal = ca == cb and min(cb) >= 0 and max(cb) <= cap
    st = 0
    for b in range(8):
        if not equal:
            break
        c = ca[b]
        for f, rb in enumerate(RBS):
            equal = equal and torch.equal(outs_a[f][st * rb:(st + c) * rb],
                                          outs_b[f][b * cap * rb:(b * cap + c) * rb])
        equal = equal and torch.equal(fid_a[st:st + c], fid_b[b * cap:b * cap + c])
        st += c
    res = {"n": N, "iters": ITERS, "rounds": ROUNDS, "cap_rows": cap, "counts": cb,
           "onepass_equals_twopass": bool(equal)}
    if not equal:
        print(json.dumps(res), flush=True)
        sys.exit(1)

    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(twopass))
        tb.append(timed(onepass))
    res["twopass"] = summary(ta)
    res["onepass"] = summary(tb)
    # one-pass bytes per row: 36 read + 36 scattered + 2 fine id, + the 12-byte
    # position rows written back (write-back "all")
    bpr = sum(RBS) * 2 + 2 + RBS[0]
    res["onepass_bytes_per_row"] = bpr
    res["onepass_tb_per_s"] = round(bpr * N / (res["onepass"]["median_ms"] * 1e-3) / 1e12, 3)
    res["onepass_fraction_of_8tbps"] = round(
        bpr * N / (res["onepass"]["median_ms"] * 1e-3) / HBM_BPS, 3)
    gain = res["twopass"]["median_ms"] - res["onepass"]["median_ms"]
    res["onepass_faster_by_ms"] = round(gain, 4)
    res["onepass_is_default"] = bool(
        gain > max(res["twopass"]["range_ms"], res["onepass"]["range_ms"]))
    line = json.dumps(res)
    print(line, flush=True)
    if os.environ.get("AB_OUT"):
        os.makedirs(os.path.dirname(os.path.abspath(os.environ["AB_OUT"])), exist_ok=True)
        with open(os.environ["AB_OUT"], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
