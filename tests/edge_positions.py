"""Edge-value position rows for the binning kernels (plain module: the CPU
tests pin it against both oracles, the GPU tests feed it to every kernel that
bins).

A uniform draw lands on a cell face, a halo threshold or nextafter(L, 0) with
probability zero; these rows land there on purpose.  ``edge_rows`` builds the
rows of one configuration, ``embed`` scatters them into in-box filler with a
fixed slab layout, ``describe`` names the rows of a failure, ``variant_hooks``
sets and restores the library's test hooks around a call.
"""
from __future__ import annotations

import contextlib

import numpy as np

SLAB = 64                      # rows of one staged slab of the bin kernel
N_BIG, N_SMALL = 4096 + 77, 64 + 13
FILLER, NEG_ZERO = -1, -2      # row-map entries that are not an index into the edge rows


# The configurations the GPU tests run (test_gpu_edge_positions.py) and the CPU
# self-checks inspect (test_edge_positions_cpu.py).  "exact": every halo
# threshold is a dyadic number that float32 holds and the periodic wrap maps
# to itself, so rows with x == hi and x == lo exist in every dtype pair, wrapped
# or not.
CASES = [
    {"id": "g3-pow2", "box": [1.0, 1.0, 1.0], "topo": [2, 2, 2], "seed": 1},
    {"id": "g3-pow2-mixed", "box": [1.0, 2.0, 4.0], "topo": [3, 5, 2], "seed": 2},
    {"id": "g3-any", "box": [0.3, 62.5, 7.0], "topo": [3, 2, 3], "seed": 3},
    {"id": "g3-any-64", "box": [1000.0, 1e-3, 10.0], "topo": [4, 4, 4], "seed": 4},
    {"id": "g3-512", "box": [1.0, 1.0, 1.0], "topo": [8, 8, 8], "seed": 5},
    {"id": "g1", "box": [0.3], "topo": [3], "seed": 6},
    {"id": "g2", "box": [1.0, 62.5], "topo": [3, 2], "seed": 7},
    {"id": "g4", "box": [1.0, 0.3, 2.0, 7.0], "topo": [2, 3, 2, 2], "seed": 8},
    {"id": "halo-222", "box": [1.0, 1.0, 1.0], "topo": [2, 2, 2],
     "overload": [0.0625, 0.125, 0.03125], "exact": True, "seed": 9},
    {"id": "halo-321", "box": [0.3, 62.5, 7.0], "topo": [3, 2, 1],
     "overload": [0.02, 3.0, 0.5], "seed": 10},
    {"id": "halo-111", "box": [1.0, 2.0, 4.0], "topo": [1, 1, 1],
     "overload": [0.125, 0.25, 0.5], "exact": True, "seed": 11},
    {"id": "fine-pow2", "box": [1.0, 1.0, 1.0], "topo": [2, 2, 2], "fine": [4, 2, 3], "seed": 12},
    {"id": "fine-any", "box": [0.3, 62.5, 7.0], "topo": [2, 2, 2], "fine": [4, 2, 3], "seed": 13},
    # n = 5, f = 5 and n = 6, f = 3: in-box float64 values just below a coarse face
    # whose fine index needs the fallback kf % f (m = kf - f * k comes out as f or -1)
    {"id": "fine-fallback", "box": [1.0, 0.3, 7.0], "topo": [5, 6, 1], "fine": [5, 3, 2],
     "seed": 14},
]


def case(case_id):
    return next(c for c in CASES if c["id"] == case_id)


def case_rows(c, dtype, box_dtype):
    """(box in its dtype, edge rows) of one configuration."""
    box = np.array(c["box"], dtype=box_dtype)
    return box, edge_rows(dtype, box, c["topo"], overload=c.get("overload"), fine=c.get("fine"),
                          seed=c["seed"])


def fixed_values(L):
    """The fixed list of tests/golden/make_golden.py edge_values(L, rng), as
    float64 (the golden fixtures' own hard values; the random tail left out)."""
    L = float(L)
    tiny = np.nextafter(0.0, 1.0)
    return np.array([0.0, -0.0, L, 2 * L, -L, -2 * L, np.nextafter(L, 0), np.nextafter(L, 2 * L),
                     tiny, -tiny, 1e-300, -1e-300, 1e-10, -1e-10,
                     0.49999999999999994 * L, 0.5 * L, 0.25 * L, -0.25 * L, -0.75 * L, 2.6 * L,
                     L / 3, 2 * L / 3, 1e20, -1e20, 1e300, -1e300, np.nan, np.inf, -np.inf,
                     6 * L - 1e-9], dtype=np.float64)


def _cast(v, dtype):
    with np.errstate(all="ignore"):
        return np.asarray(v, dtype=np.float64).astype(dtype)


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _unique_bits(a):
    """Drop repeated bit patterns, first occurrence kept (-0.0 and 0.0 differ)."""
    _, first = np.unique(_bits(a), return_index=True)
    return a[np.sort(first)]


def cell_length(box, topo):
    """box[d] / topo[d] as the reference computes it (redist.py:49-51): float64."""
    box = np.asarray(box)
    topo = np.array(topo).astype(np.int64)
    cl = np.zeros(len(topo))
    for d in range(len(topo)):
        cl[d] = box[d] / topo[d]
    return cl


def dim_values(dtype, L, n, cl, ol=None, f=None):
    """The value set of one dimension in the position dtype: the fixed list,
    and every cell face k * cl (k = 0..n) -- with the halo thresholds
    k * cl +- ol and the fine faces j * cl / f (j = 0..n * f) when asked --
    each with its two nextafter neighbours in that dtype."""
    dtype = np.dtype(dtype)
    k = np.arange(n + 1, dtype=np.int64)
    faces = [k * cl]                       # int64 * float64, as redist.py:110-111
    if ol is not None:
        faces += [k * cl + ol, k * cl - ol]
    if f is not None:
        faces.append(np.arange(n * f + 1, dtype=np.int64) * (cl / f))
    faces = _cast(np.concatenate(faces), dtype)
    lo = np.nextafter(faces, dtype.type(-np.inf))
    hi = np.nextafter(faces, dtype.type(np.inf))
    near = np.stack([lo, faces, hi], axis=1).reshape(-1)
    return _unique_bits(np.concatenate([_cast(fixed_values(L), dtype), near]))


def _inbox(rng, dtype, L, m):
    """m values strictly inside (0, L), away from every face by chance only."""
    return _cast(rng.uniform(0.05, 0.95, m) * float(L), dtype)


def edge_rows(dtype, box, topo, overload=None, fine=None, seed=0):
    """(m, dim) rows of ``dtype``.  Every value of every dimension's value set
    (dim_values) appears in three rows: (a) the other coordinates strictly
    in-box, (b) one other coordinate itself an edge value, (c) the other
    coordinates uniform in [-2L, 3L).  One dimension: one row per value."""
    dtype = np.dtype(dtype)
    box = np.asarray(box)
    dim = len(topo)
    rng = np.random.default_rng(seed)
    cl = cell_length(box, topo)
    vals = [dim_values(dtype, box[d], int(topo[d]), cl[d],
                       None if overload is None else float(overload[d]),
                       None if fine is None else int(fine[d])) for d in range(dim)]
    out = []
    for d in range(dim):
        v = vals[d]
        m = len(v)
        a = np.stack([_inbox(rng, dtype, box[e], m) for e in range(dim)], axis=1)
        a[:, d] = v
        out.append(a)
        if dim == 1:
            continue
        b = np.stack([_inbox(rng, dtype, box[e], m) for e in range(dim)], axis=1)
        b[:, d] = v
        others = [e for e in range(dim) if e != d]
        for j, e in enumerate(others):
            rows = np.arange(j, m, len(others))
            b[rows, e] = vals[e][rng.integers(0, len(vals[e]), len(rows))]
        out.append(b)
        c = np.stack([_cast(rng.uniform(-2.0, 3.0, m) * float(box[e]), dtype)
                      for e in range(dim)], axis=1)
        c[:, d] = v
        out.append(c)
    return np.ascontiguousarray(np.concatenate(out, axis=0))


def _wrap_columns(pos, box):
    """The reference's periodic wrap of every column (redist.py:68, :328-329),
    numpy's own promotion of the position and box dtypes."""
    for d in range(pos.shape[1]):
        pos[:, d] = ((pos[:, d] % box[d]) + box[d]) % box[d]
    return pos


def filler_rows(dtype, box, m, seed):
    """m strictly in-box rows that the periodic wrap maps to themselves bit
    for bit: one wrap of a uniform draw is a fixed point of the wrap (x + L is
    then exact), which the assertion re-checks."""
    box = np.asarray(box)
    rng = np.random.default_rng(seed)
    p = np.stack([_inbox(rng, dtype, box[d], m) for d in range(len(box))], axis=1)
    p = _wrap_columns(p, box)
    q = _wrap_columns(p.copy(), box)
    assert p.tobytes() == q.tobytes(), "filler rows must wrap to themselves"
    assert ((p > 0) & (p.astype(np.float64) < box.astype(np.float64))).all()
    return p


def _draw(rng, m, count):
    """``count`` >= 1 indexes into m rows: whole permutations of all of them,
    one after the other (fewer rows than places: rows repeat), cut to count."""
    reps = -(-count // m)
    return np.concatenate([rng.permutation(m) for _ in range(reps)])[:count].astype(np.int64)


def embed(rows, n_total, seed, box):
    """Scatter edge rows into ``n_total`` rows of filler (filler_rows).
    Returns (positions, row_map): row_map[i] is the index into ``rows`` of row
    i, FILLER, or NEG_ZERO.  Deterministic in (rows, n_total, seed).

    Five or more slabs (of SLAB = 64 rows):
      * slab 0, and every later slab whose number is a multiple of 4, holds
        filler only: clean, never written back under skip_clean;
      * slab 1 is filler but for one row that is filler with one coordinate
        -0.0: its only change is the sign flip -0.0 -> +0.0;
      * slab 2 is all edge rows;
      * the ragged last round (n_total % 64 rows) is all edge rows;
      * the other edge rows are scattered over the remaining slabs.
    Every row of ``rows`` is placed at least once (more than once only where
    there are fewer rows than the all-edge places: one dimension).  Fewer
    than five slabs (the 77-row size: one full round and a ragged one): every
    row is an edge row, a seeded draw from ``rows``."""
    rows = np.ascontiguousarray(rows)
    dim = rows.shape[1]
    rng = np.random.default_rng(seed)
    m = len(rows)
    full = n_total // SLAB
    if full < 5:
        pick = _draw(rng, m, n_total)
        return rows[pick].copy(), pick
    pos = filler_rows(rows.dtype, box, n_total, seed + 1)
    src = np.full(n_total, FILLER, dtype=np.int64)
    z = SLAB + int(rng.integers(0, SLAB))
    pos[z, int(rng.integers(0, dim))] = -0.0
    src[z] = NEG_ZERO
    ragged = np.arange(full * SLAB, n_total)
    solid = np.arange(2 * SLAB, 3 * SLAB)
    free = np.concatenate([np.arange(s * SLAB, (s + 1) * SLAB) for s in range(3, full) if s % 4])
    fixed = np.concatenate([solid, ragged])
    assert m <= len(fixed) + len(free), (m, len(fixed), len(free))
    order = _draw(rng, m, max(m, len(fixed)))
    where = np.concatenate([fixed, np.sort(rng.permutation(free)[: len(order) - len(fixed)])])
    pos[where] = rows[order]
    src[where] = order
    return pos, src


def describe(pos_in, row_map, bad, limit=6):
    """The input rows behind a mismatch: row number, what it is, its values."""
    out = []
    for r in np.asarray(bad).reshape(-1)[:limit]:
        kind = {FILLER: "filler", NEG_ZERO: "filler with -0.0"}.get(int(row_map[r]),
                                                                   f"edge row {int(row_map[r])}")
        out.append(f"row {int(r)} ({kind}): {[repr(x) for x in pos_in[r].tolist()]}")
    return "; ".join(out) if out else "no rows"


def differing_rows(a, b):
    """Rows of two same-shape 2-D arrays whose bytes differ."""
    ua = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    ub = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return np.nonzero((ua != ub).any(axis=1))[0]


@contextlib.contextmanager
def variant_hooks(lib, variant):
    """Set the library's test hooks of ``variant`` (every key but
    "write_back", which is a per-plan option) and restore the shipped
    defaults afterwards."""
    try:
        for k, v in variant.items():
            if k != "write_back":
                lib.test_hook(k, v)
        yield variant
    finally:
        for k, v in lib.HOOK_DEFAULTS.items():
            lib.test_hook(k, v)
