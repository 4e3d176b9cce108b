#!/usr/bin/env python3
"""SoA halo pack A/B (GPU): the wide multi-selection pack against separate
launches of the three-field kernel, on one rank's local sends.

Rows: config 5's four arrays (pos f32 x3, vel f32 x3, mass f32, id i64), the
carried positions (f32 x3) and the 2-byte face flags -- 6 fields, 50 bytes a
row.  Sets: the 6 faces at config 3's halo density (overload 0.05 of a box
whose cells are 0.5 wide: each face holds 10 % of the rows), each set packed
to its own place in a staging buffer per field, as halo.exchange_overload
packs a rank's local sends.

  a  one launch of the wide kernel, all 6 fields
  b  two launches of the three-field kernel, 3 fields each (the baseline: what
     moving the same fields costs without the wide kernel)
  c  the single-array halo's three fields (36-byte records, positions, flags)
     through the three-field kernel (c3) and, by test hook msel_wide, through
     the wide kernel (cw)

The variants alternate inside every round of one process; device events
around each; medians, minima and the spread over the rounds.  Outputs of a and
b are compared byte for byte before timing.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_grid_redistribute_amd import _lib  # noqa: E402
from mpi_grid_redistribute_amd.halo import DeviceSelect  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--density", type=float, default=0.1)
    args = ap.parse_args()
    n, dev = args.rows, torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5)
    flags = torch.zeros(n, dtype=torch.int16, device=dev)
    for b in range(6):
        flags |= (torch.rand(n, generator=g, device=dev) < args.density).to(torch.int16) << b
    sel = DeviceSelect(dev)
    h, cnt = sel.msel(flags, n, list(range(6)), "_ab")
    counts = cnt.cpu().numpy()
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(starts[-1])

    def field(rb):
        return torch.randint(0, 256, (n * rb,), generator=g, device=dev, dtype=torch.uint8)

    def places(rbs):
        bufs = [torch.zeros(total * rb, dtype=torch.uint8, device=dev) for rb in rbs]
        return bufs, [[b[int(starts[k]) * rb:int(starts[k + 1]) * rb] for k in range(6)]
                      for b, rb in zip(bufs, rbs)]

    flag_bytes = flags.view(torch.uint8)
    rbs6 = [12, 12, 4, 8, 12, 2]
    src6 = [field(rb) for rb in rbs6[:5]] + [flag_bytes]
    out_a, dst_a = places(rbs6)
    out_b, dst_b = places(rbs6)
    rbs3 = [36, 12, 2]
    src3 = [field(36), src6[4], flag_bytes]
    out_c, dst_c = places(rbs3)
    out_w, dst_w = places(rbs3)

    def wide_on(on):
        _lib.test_hook("msel_wide", int(on))

    def run_a():
        sel.msel_pack_fields(h, src6, rbs6, dst_a)

    def run_b():
        sel.msel_pack_fields(h, src6[:3], rbs6[:3], dst_b[:3])
        sel.msel_pack_fields(h, src6[3:], rbs6[3:], dst_b[3:])

    def run_c3():
        sel.msel_pack_fields(h, src3, rbs3, dst_c)

    def run_cw():
        wide_on(True)
        try:
            sel.msel_pack_fields(h, src3, rbs3, dst_w)
        finally:
            wide_on(False)

    variants = {"a_wide_6": run_a, "b_three_field_x2": run_b, "c3_three_field": run_c3,
                "cw_wide_3": run_cw}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(out_a, out_b)) and \
        all(torch.equal(x, y) for x, y in zip(out_c, out_w))
    if not same:
        raise SystemExit("the variants' outputs differ")
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"rows": n, "rows_out": total, "density": args.density, "rounds": args.rounds,
           "bytes_6_fields": 2 * n + 2 * total * sum(rbs6),
           "bytes_3_fields": 2 * n + 2 * total * sum(rbs3), "outputs_equal": same}
    for k, t in times.items():
        t = np.asarray(t)
        res[k] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                  "max_ms": round(float(t.max()), 4),
                  "p10_ms": round(float(np.percentile(t, 10)), 4),
                  "p90_ms": round(float(np.percentile(t, 90)), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
