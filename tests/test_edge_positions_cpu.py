"""CPU pins of the edge-value position rows (tests/edge_positions.py).

1. The two oracles agree on them: c_oracle.bin_positions(want_idx=True)
   against redist_oracle's NumPy restatement -- cells, raw indexes and the
   wrapped position bytes -- in 1 to 4 dimensions, the three position / box
   dtype pairs, four boxes, both ``periodic`` values.  The GPU tests
   (test_gpu_edge_positions.py) take their expectations from the C oracle, so
   this is what ties those expectations to the reference-pinned NumPy one.
2. Generator self-checks, so that a later edit cannot hollow the matrix out:
   every configuration holds, per dimension, a NaN, both infinities, a -0.0,
   the halo thresholds of the landing cell with both neighbours, and the rows
   that bear on the two index reductions of bin_row_fast (below).  Each
   self-check prints the count of rows in each class (pytest -s shows them).

The ``k >= n`` reduction of bin_row_fast.  No in-box row can reach it, and
the self-check asserts exactly that (zero such rows in every configuration)
together with what does exist: rows on the general path whose raw index is n
(x == L unwrapped; a float32 wrap against a float64 box that rounds up to L),
and in-box rows at nextafter(L, 0) whose raw index is n - 1.  Why none
exists: for x < L in one precision the correctly rounded x / L is at most
1 - u (u = the spacing below 1: L - x is at least one ulp of L, which is more
than u / 2 relative to L), and (1 - u) * n is below n by n * u, at least half
an ulp of n with the tie (n a power of two) exact, so the product never
rounds up to n; float32 positions against a float64 box are further from L
still.  The reduction is a guard, not a reachable path.

The fine fallback ``m = kf - f * k`` outside [0, f).  It needs a quotient
whose products with n and with n * f round to different sides of a coarse
face.  With a float32 quotient both products are exact in float64, so no such
row exists; in float64 it takes particular (n, f): fine = [4, 2, 3] on
[2, 2, 2] has none in either box, and the self-check asserts that.  The case
"fine-fallback" (topology [5, 6, 1], fine [5, 3, 2]) has in-box float64 rows
just below a coarse face where m comes out as f or -1 -- unwrapped, that is
binned with periodic=False; the periodic wrap moves them off the value.
FINE_FALLBACK below records which configurations have one.
"""
import numpy as np
import pytest

from oracle import c_oracle
from oracle import redist_oracle as ro
from tests import edge_positions as E
from tests import golden_io as G

PAIRS = [(np.float64, np.float64), (np.float32, np.float64), (np.float32, np.float32)]
PAIR_IDS = ["f64-f64", "f32-f64", "f32-f32"]
BOXES = [([1, 1, 1], [2, 2, 2]), ([1, 2, 4], [3, 5, 2]), ([0.3, 62.5, 7.0], [3, 2, 3]),
         ([1000, 1e-3, 10], [4, 4, 4])]


def _dims(box, topo, dim):
    """The 3-D configuration cut to 1 or 2 dimensions, or grown to 4."""
    if dim <= 3:
        return box[:dim], topo[:dim]
    return box + [box[1]], topo + [topo[0]]


def _numpy_oracle(rows, box, topo, periodic):
    p = rows.copy()
    geo = ro.Geometry(topo, box, int(np.prod(topo)))
    with np.errstate(all="ignore"):
        idx = ro.cell_indexes_from_position(geo, p, periodic)
    return p, idx, ro.cell_number_from_indexes(geo, idx)


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("dim", [1, 2, 3, 4])
@pytest.mark.parametrize("box,topo", BOXES, ids=[f"box{i}" for i in range(len(BOXES))])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_oracles_agree_on_edge_rows(pair, box, topo, dim, periodic):
    box, topo = _dims(box, topo, dim)
    b = np.array(box, dtype=pair[1])
    rows = E.edge_rows(pair[0], b, topo, overload=[0.0625 * float(x) for x in b],
                       fine=[4, 2, 3, 2][:dim], seed=dim)
    p1 = rows.copy()
    cell, idx = c_oracle.bin_positions(p1, topo, b, periodic=periodic, want_idx=True)
    p2, idx2, cell2 = _numpy_oracle(rows, b, topo, periodic)
    bad = E.differing_rows(p1, p2)
    assert len(bad) == 0, E.describe(rows, np.arange(len(rows)), bad)
    bad = np.nonzero((idx != idx2).any(axis=1) | (cell != cell2))[0]
    assert len(bad) == 0, E.describe(rows, np.arange(len(rows)), bad)
    assert cell.min() >= 0 and cell.max() < int(np.prod(topo))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_halo_and_fine_oracles_take_every_row(pair):
    """The overload and fine-cell oracles accept rows with NaN and infinities
    and give in-range results: no value class is left out of a GPU test."""
    topo, box, ol, fine = [2, 2, 2], np.array([1.0, 1.0, 1.0], dtype=pair[1]), [0.0625] * 3, [4, 2, 3]
    rows = E.edge_rows(pair[0], box, topo, overload=ol, fine=fine, seed=5)
    parts = np.array_split(np.arange(len(rows)), 8)
    pos = [rows[i].copy() for i in parts]
    data = [i.astype(np.int64) for i in parts]
    with np.errstate(all="ignore"):
        out = ro.redistribute_by_position_overload_all_ranks(topo, box, 8, data, pos, ol)
        fid = ro.fine_cell_ids(topo, fine, box, np.concatenate(pos))
    got = np.concatenate(out)
    assert got.min() >= 0 and got.max() < len(rows)
    assert set(np.concatenate(data).tolist()) <= set(got.tolist())   # every row owned once
    assert fid.min() >= 0 and fid.max() < int(np.prod(fine))


# ------------------------------------------------------------ self-checks
def _sign_bit_only(col):
    return E._bits(col) == (1 << (8 * col.dtype.itemsize - 1))


def _threshold_classes(x, xs, k, cl, ol, sel):
    """Counts, among the rows ``sel``, of the stored coordinate xs (float64)
    against its landing cell's limits hi = (k + 1) cl - ol and lo = k cl + ol:
    equal, the first value above, and the last value not above (for lo: not
    below / the last below) -- the neighbours in the position dtype x has."""
    hi = (k + 1) * cl - ol
    lo = k * cl + ol
    dn = np.nextafter(x, x.dtype.type(-np.inf)).astype(np.float64)
    up = np.nextafter(x, x.dtype.type(np.inf)).astype(np.float64)
    return {"x==hi": int((sel & (xs == hi)).sum()),
            "first>hi": int((sel & (xs > hi) & (dn <= hi)).sum()),
            "last<=hi": int((sel & (xs <= hi) & (up > hi)).sum()),
            "x==lo": int((sel & (xs == lo)).sum()),
            "last<lo": int((sel & (xs < lo) & (up >= lo)).sum()),
            "first>=lo": int((sel & (xs >= lo) & (dn < lo)).sum())}


@pytest.mark.parametrize("case", E.CASES, ids=[c["id"] for c in E.CASES])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_generator_self_check(pair, case, capsys):
    box = np.array(case["box"], dtype=pair[1])
    topo, ol, fine = case["topo"], case.get("overload"), case.get("fine")
    dim = len(topo)
    rows = E.edge_rows(pair[0], box, topo, overload=ol, fine=fine, seed=case["seed"])
    L = box.astype(np.float64)
    r64 = rows.astype(np.float64)
    inbox = ((r64 >= 0) & (r64 < L)).all(axis=1)           # the rows bin_row_fast takes
    _, idx_raw, _ = _numpy_oracle(rows, box, topo, False)   # unwrapped: the value itself
    pw, idx_w, _ = _numpy_oracle(rows, box, topo, True)
    cl = E.cell_length(box, topo)
    report = {"rows": len(rows), "in-box rows": int(inbox.sum())}
    for d in range(dim):
        col = rows[:, d]
        n = int(topo[d])
        c = {"nan": int(np.isnan(col).sum()), "+inf": int(np.isposinf(col).sum()),
             "-inf": int(np.isneginf(col).sum()), "-0.0": int(_sign_bit_only(col).sum()),
             "-0.0 in-box": int((_sign_bit_only(col) & inbox).sum()),
             "in-box raw==n": int((inbox & (idx_raw[:, d] == n)).sum()),
             "in-box raw==n (wrapped)": int((inbox & (idx_w[:, d] == n)).sum()),
             "general raw==n": int((~inbox & (idx_raw[:, d] == n)).sum()),
             "in-box raw==n-1 at nextafter(L,0)": int(
                 (inbox & (col == np.nextafter(col.dtype.type(box[d]), col.dtype.type(0)))
                  & (idx_raw[:, d] == n - 1)).sum())}
        assert c["nan"] and c["+inf"] and c["-inf"] and c["-0.0"] and c["-0.0 in-box"], (d, c)
        # the k >= n reduction: unreachable in-box (module docstring), reached elsewhere
        assert c["in-box raw==n"] == 0 and c["in-box raw==n (wrapped)"] == 0, (d, c)
        assert c["general raw==n"] > 0, (d, c)
        if np.dtype(pair[0]) == np.dtype(pair[1]):   # nextafter(L, 0) is in-box in the box's type
            assert c["in-box raw==n-1 at nextafter(L,0)"] > 0, (d, c)
        if ol is not None:
            for name, p, idx in (("unwrapped", rows, idx_raw), ("wrapped", pw, idx_w)):
                xs = p[:, d].astype(np.float64)
                own = (xs >= 0) & (xs < L[d])
                k = np.where(own, idx[:, d], 0) % n
                fast = _threshold_classes(p[:, d], xs, k, cl[d], ol[d], inbox & own)
                gen = _threshold_classes(p[:, d], xs, k, cl[d], ol[d], ~inbox & own)
                c[f"halo {name} fast"], c[f"halo {name} general"] = fast, gen
                for t in (fast, gen):
                    # unwrapped (periodic=False binning, and the stand-alone flags
                    # kernel, which never wraps): both neighbours of each threshold;
                    # a wrap moves values onto the coarser grid of x + L, where the
                    # neighbours fall together: wrapped rows are counted, and asserted
                    # to hold the threshold itself in the exact cases
                    if name == "unwrapped":
                        assert (t["first>hi"] and t["last<=hi"] and t["last<lo"]
                                and t["first>=lo"]), (d, name, t)
                    # the threshold itself, bit for bit (a float32 row holds it only
                    # where it is representable: the exact cases)
                    if (name == "unwrapped" and pair[0] == np.float64) or case.get("exact"):
                        assert t["x==hi"] and t["x==lo"], (d, name, t)
        if fine is not None:
            f = int(fine[d])
            geo = ro.Geometry([n * f], box[d:d + 1], n * f)
            for name, p, idx in (("unwrapped", rows, idx_raw), ("wrapped", pw, idx_w)):
                with np.errstate(all="ignore"):
                    kf = ro.cell_indexes_from_position(geo, p[:, d:d + 1].copy(), False)[:, 0]
                m = ro.periodic_wrap(kf, n * f) - f * ro.periodic_wrap(idx[:, d], n)
                out = (m < 0) | (m >= f)
                c[f"fine {name} m outside [0,f) in-box"] = int((inbox & out).sum())
                c[f"fine {name} m outside [0,f) general"] = int((~inbox & out).sum())
        report[f"dim {d}"] = c
    if fine is not None:
        have = any(report[f"dim {d}"][f"fine {w} m outside [0,f) in-box"]
                   for d in range(dim) for w in ("unwrapped", "wrapped"))
        assert have == FINE_FALLBACK[(case["id"], PAIR_IDS[PAIRS.index(pair)])], report
    with capsys.disabled():
        print(f"\n[{case['id']} {PAIR_IDS[PAIRS.index(pair)]}]")
        for key, val in report.items():
            print(f"  {key}: {val}")


# in-box rows whose fine index needs the fallback kf % f exist (True) or
# provably do not (False: asserted), per fine configuration and dtype pair
FINE_FALLBACK = {
    ("fine-pow2", "f64-f64"): False, ("fine-pow2", "f32-f64"): False, ("fine-pow2", "f32-f32"): False,
    ("fine-any", "f64-f64"): False, ("fine-any", "f32-f64"): False, ("fine-any", "f32-f32"): False,
    ("fine-fallback", "f64-f64"): True, ("fine-fallback", "f32-f64"): False,
    ("fine-fallback", "f32-f32"): False,
}


@pytest.mark.parametrize("case", E.CASES, ids=[c["id"] for c in E.CASES])
@pytest.mark.parametrize("n_total", [E.N_BIG, E.N_SMALL])
def test_embed_layout(case, n_total):
    box = np.array(case["box"], dtype=np.float64)
    rows = E.edge_rows(np.float64, box, case["topo"], overload=case.get("overload"),
                       fine=case.get("fine"), seed=case["seed"])
    pos, src = E.embed(rows, n_total, 11, box)
    pos2, src2 = E.embed(rows, n_total, 11, box)
    assert G.same_bytes(pos, pos2) and np.array_equal(src, src2)      # deterministic
    assert pos.shape == (n_total, len(box)) and n_total % E.SLAB != 0
    edge = src >= 0
    assert G.same_bytes(pos[edge], rows[src[edge]])
    last = (n_total // E.SLAB) * E.SLAB
    assert edge[last:].all()                                          # the ragged round
    if n_total == E.N_SMALL:
        assert edge.all()
        return
    assert sorted(set(src[edge].tolist())) == list(range(len(rows)))  # every row is there
    slabs = src[:last].reshape(-1, E.SLAB)
    assert (slabs[0] == E.FILLER).all() and (slabs[2] >= 0).all()
    assert (slabs[1] == E.NEG_ZERO).sum() == 1 and (slabs[1] == E.FILLER).sum() == E.SLAB - 1
    z = pos[np.nonzero(src == E.NEG_ZERO)[0][0]]
    assert _sign_bit_only(z).sum() == 1
    # the filler wraps to itself: under skip_clean its slabs are not written back
    p = pos.copy()
    c_oracle.bin_positions(p, case["topo"], box)
    changed = E.differing_rows(p, pos)
    assert not (src[changed] == E.FILLER).any()
    assert np.nonzero(src == E.NEG_ZERO)[0][0] in changed
    clean = [s for s in range(len(slabs)) if (slabs[s] == E.FILLER).all()]
    assert len(clean) >= 2
