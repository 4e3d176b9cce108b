#!/usr/bin/env python3
"""Generate tests/golden/soa_halo_*.npz by running the REFERENCE itself, on the
CPU, the way make_golden.py does (whose helpers this imports):
    python tests/golden/make_golden_soa_halo.py

The overload (halo) rows of a SoA payload -- several arrays sharing axis 0 --
are what the reference's ``exchange_overload_by_position`` (redist.py:202-309)
returns called ONCE PER FIELD with the same positions: the selections read
the positions only, so every field gets the same rows in the same order.
Ranks run as threads; every rank's 40-300 local rows lie inside its cell (the
call's precondition, as in make_golden.make_halo's direct cases).

Each fixture: topology, box, size, overload, periodic, nfields and per rank
``r{r}_pos``, ``r{r}_f{i}_in`` (the local rows of field i) and ``r{r}_f{i}_out``
(the reference's overload rows of field i).  A field of kind "pos" is the
position array itself.
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

OUT_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT_DIR)
from make_golden import load_reference, run_ranks, soa_field  # noqa: E402

CASES = [
    # name, topology, box, pos dtype, periodic, overload_lengths, fields
    ("p8", [2, 2, 2], [1.0, 1.0, 1.0], np.float32, True, [0.1, 0.15, 0.2],
     ["pos", "vel_f32x3", "mass_f32", "id_i64"]),
    # periodic=False: the :287 flag quirk; the z extent of 1 is a self dimension
    ("p6_321", [3, 2, 1], [3.0, 2.0, 1.5], np.float64, False, [0.4, 0.3, 0.2],
     ["pos", "flag_u8", "ten_f64x2x2", "id_i32", "tri_i16x3"]),
    ("p1_self", [1, 1, 1], [1.0, 1.0, 1.0], np.float64, True, [0.2, 0.1, 0.3],
     ["id_i64", "vel_f32x3", "rec32"]),
    ("p4_2d", [4, 1], [4.0, 1.0], np.float64, True, [0.3, 0.2],
     ["mat_f64x3", "id_i32"]),
]


def field(kind, pos, rng, gid0):
    if kind == "ten_f64x2x2":
        return rng.normal(size=(len(pos), 2, 2))
    if kind == "rec32" and pos.shape[1] < 3:
        raise ValueError("rec32 needs 3-D positions")
    return soa_field(kind, pos, rng, gid0)


def make_soa_halo(ref, rng):
    for name, topo, box, pdt, periodic, ol, kinds in CASES:
        size = int(np.prod(topo))

        def fn0(comm, r):
            return ref.MPIGridRedistributor(comm, topo, box).rank_cell_limits.copy()

        lims = run_ranks(size, fn0)
        pos_l, fields_l = [], []
        gid = 0
        for r in range(size):
            n = int(rng.integers(40, 300))
            lo, hi = lims[r][:, 0], lims[r][:, 1]
            p = (lo + rng.random((n, len(topo))) * (hi - lo)).astype(pdt)
            pos_l.append(p)
            fields_l.append([field(k, p, rng, gid) for k in kinds])
            gid += n

        def fn(comm, r):
            R = ref.MPIGridRedistributor(comm, topo, box)
            return [R.exchange_overload_by_position(x, pos_l[r], ol, periodic=periodic)
                    for x in fields_l[r]]

        res = run_ranks(size, fn)
        f = {"topology": np.asarray(topo, dtype=np.int64), "box": np.asarray(box),
             "size": np.int64(size), "overload": np.asarray(ol, dtype=np.float64),
             "periodic": np.bool_(periodic), "nfields": np.int64(len(kinds))}
        for r in range(size):
            f[f"r{r}_pos"] = pos_l[r]
            for i in range(len(kinds)):
                f[f"r{r}_f{i}_in"] = fields_l[r][i]
                f[f"r{r}_f{i}_out"] = res[r][i]
        np.savez_compressed(os.path.join(OUT_DIR, f"soa_halo_{name}.npz"), **f)
    return len(CASES)


if __name__ == "__main__":
    print("SoA halo fixtures:", make_soa_halo(load_reference(), np.random.default_rng(20261021)))
