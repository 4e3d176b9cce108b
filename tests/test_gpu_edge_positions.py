"""Edge-value positions through every kernel that bins (tests/edge_positions.py).

The golden edge fixtures reach the GPU only through cell_ids_kernel with one
dimension, which compiles bin_row_fast out; every other GPU test draws
uniform positions, which land on a cell face, a halo threshold or
nextafter(L, 0) with probability zero.  Here the edge rows -- -0.0, L,
nextafter(L, 0), subnormals, 1e300, NaN, +-inf, every cell face, halo
threshold and fine face with both neighbours -- run through the in-box fast
path and the general path of every binning kernel, against the C oracle
(which test_edge_positions_cpu.py ties to the NumPy oracle on the same rows).

Each test compares the wrapped positions byte for byte (the whole backing
buffer: padding columns included), the payload arange(n) against
argsort(cell, kind="stable"), and the counts against bincount.

Kernel template instances reached (read off the launchers bin_count_w /
bin_count_dim / bin_count_t / geo_kind in mgr_bin.hip, launch_onepass* in
mgr_onepass*.hip, cell_ids_t, halo_flags_t; _instance() below restates that
selection and puts it into every two-pass test id):

bin_count_kernel<PosT, kP, DestT, NU, DIM, NT=true, DEPTH=1, SIDE, GEO>
  * PosT float / double; kP true / false; DestT uint8_t, and uint16_t at
    [8, 8, 8] (512 bins: 2-byte destinations and the xcd tile order);
  * NU = 16-byte units per row: float (n,3) and (n,4) -> 1, 36-byte records
    -> 3, 64-byte rows -> 4; double (n,3) and (n,4) -> 2, 48-byte rows -> 3,
    64-byte rows -> 4, double 1-D -> 1; NU 0 (unstaged) for rows wider than
    64 bytes, a base 8 bytes off 16-byte alignment, and the bin_unstaged hook;
  * DIM 1, 2, 3, and 0 for four dimensions;
  * GEO (periodic, staged, 3-D only): kGeoF64 for double or float positions
    with a float64 power-of-two box ([1,1,1], [1,2,4]), kGeoF32 for float
    positions with a float32 power-of-two box, kGeoAny for [0.3,62.5,7.0],
    [1000,1e-3,10], the bin_generic hook, non-periodic, unstaged, DIM != 3;
  * SIDE kSideNone (partition_by_position, partition_device), kSideFine
    (partition_device / partition_fields_device / redistribute_by_position
    with fine_cells), kSideHalo (redistribute_by_position with
    overload_lengths); the last two with kGeoF32 / kGeoF64 / kGeoAny alike;
  * PosT f16_t with NU 0, DIM 0, kSideHalo (bin_coord_ext).
onepass_partition_kernel / onepass_fields_kernel<PosT, kP, SIDE, GEO, NW>
  * float / double, kP true / false, kSideNone / kSideFine, kGeoF32 /
    kGeoF64 / kGeoAny (non-periodic and bin_generic: kGeoAny).
cell_ids_kernel<float / double, kP> with two, three and four dimensions.
halo_flags_kernel<float / double / int32_t / f16_t>.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import redist_oracle as ro
from tests import edge_positions as E
from tests import golden_io as G
from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import GridPartitioner, MPIGridRedistributor, _lib  # noqa: E402
from mpi_grid_redistribute_amd.comm import Transport  # noqa: E402

PAIRS = {"f64-f64": (np.float64, np.float64), "f32-f64": (np.float32, np.float64),
         "f32-f32": (np.float32, np.float32)}
N_BIG, N_SMALL = E.N_BIG, E.N_SMALL
# position layouts: elements per row of the backing buffer (float32, float64)
# and the byte offset of its base from 16-byte alignment
LAYOUTS = {"contig": ((3, 3), 0), "pad4": ((4, 4), 0), "rec": ((9, 6), 0), "row64": ((16, 8), 0),
           "wide": ((17, 9), 0), "off8": ((3, 3), 8)}


class SizedComm(Transport):
    """Rank 0 of a ``size``-rank world, for the binning-only API calls."""

    def __init__(self, size):
        self.size, self.rank = size, 0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------ inputs, expectations
@functools.lru_cache(maxsize=None)
def _input(case_id, pair, n_total):
    """(box, positions, row map) of a configuration: computed once, read-only."""
    c = E.case(case_id)
    box, rows = E.case_rows(c, *PAIRS[pair])
    pos, src = E.embed(rows, n_total, c["seed"] + 100, box)
    pos.setflags(write=False)
    src.setflags(write=False)
    return box, pos, src


@functools.lru_cache(maxsize=None)
def _expect(case_id, pair, n_total, periodic):
    """C oracle on a copy: (wrapped positions, cells, stable order, counts)."""
    box, pos, _ = _input(case_id, pair, n_total)
    topo = E.case(case_id)["topo"]
    p = pos.copy()
    cell = c_oracle.bin_positions(p, topo, box, periodic=periodic)
    order = np.argsort(cell, kind="stable")
    counts = np.bincount(cell, minlength=int(np.prod(topo)))
    for a in (p, cell, order, counts):
        a.setflags(write=False)
    return p, cell, order, counts


def _backing(pos, width):
    """(n, width) buffer of the position dtype: the positions in its first
    columns, a per-row sentinel in the padding columns."""
    n, dim = pos.shape
    back = np.empty((n, width), dtype=pos.dtype)
    back[:] = -(1000.0 + np.arange(n, dtype=np.float64) % 4096)[:, None]
    back[:, :dim] = pos
    return back


def _to_device(back, offset=0):
    """The backing buffer on the GPU, its base ``offset`` bytes past an
    allocation's start; returns (storage kept alive, (n, width) view)."""
    k = offset // back.dtype.itemsize
    store = torch.zeros(back.size + k + 4, dtype=torch.from_numpy(back[:1]).dtype, device="cuda")
    view = store[k:k + back.size].view(back.shape)
    view.copy_(torch.from_numpy(back))
    assert view.data_ptr() % 16 == offset % 16
    return store, view


def _same_rows(got, exp, pos_in, src, what):
    bad = E.differing_rows(got, exp)
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ: " + E.describe(pos_in, src, bad)


def _check_partition(out_ids, counts, order, exp_counts, pos_in, src, what):
    assert np.array_equal(counts, exp_counts), (what, counts, exp_counts)
    bad = np.nonzero(out_ids != order)[0]
    assert len(bad) == 0, (f"{what}: output differs from the stable order at {bad[:6]}: "
                           + E.describe(pos_in, src, order[bad]))


def _instance(case_id, pair, periodic, layout="contig", variant=None, side="kSideNone"):
    """The bin_count_kernel instance the launchers pick (module docstring)."""
    variant = variant or {}
    c = E.case(case_id)
    f32 = PAIRS[pair][0] == np.float32
    dim = len(c["topo"])
    widths, off = LAYOUTS[layout]
    rb = (widths[0] * 4 if f32 else widths[1] * 8) if dim == 3 else dim * (4 if f32 else 8)
    staged = not variant.get("bin_unstaged") and rb <= 64 and off % 16 == 0
    nu = (rb + 15) // 16 if staged else 0
    geo = "kGeoAny"
    pow2 = all(np.frexp(float(x))[0] == 0.5 for x in c["box"])
    if dim == 3 and periodic and nu > 0 and not variant.get("bin_generic") and pow2:
        geo = "kGeoF32" if pair == "f32-f32" else "kGeoF64"
    dest = "u8" if int(np.prod(c["topo"])) <= 256 else "u16"
    return (f"{'float' if f32 else 'double'},kP={int(periodic)},{dest},NU={nu},"
            f"DIM={dim if dim <= 3 else 0},{side},{geo}")


# ------------------------------------------------------------ two-pass path
def _two_pass(case_id, pair, n_total, periodic, layout="contig", variant=None):
    variant = variant or {}
    box, pos, src = _input(case_id, pair, n_total)
    exp_p, _, order, exp_counts = _expect(case_id, pair, n_total, periodic)
    topo = E.case(case_id)["topo"]
    n, dim = pos.shape
    widths, off = LAYOUTS[layout]
    width = (widths[0] if pos.dtype == np.float32 else widths[1]) if dim == 3 else dim
    back = _backing(pos, width)
    exp_back = back.copy()
    exp_back[:, :dim] = exp_p
    ids = torch.arange(n, dtype=torch.int64, device="cuda")
    with E.variant_hooks(_lib, variant):
        P = GridPartitioner(topo, box)
        P.set_write_back(variant.get("write_back", "changed"))
        store, view = _to_device(back, off)
        out, offsets = P.partition_by_position(ids, view[:, :dim], periodic=periodic)
        _same_rows(view.cpu().numpy(), exp_back, pos, src, "partition_by_position positions")
        _check_partition(out.cpu().numpy(), np.diff(offsets.cpu().numpy()), order, exp_counts,
                         pos, src, "partition_by_position")
        store, view = _to_device(back, off)
        out, counts = P.partition_device(ids.view(torch.uint8).reshape(-1), 8, view[:, :dim],
                                         periodic=periodic)
        torch.cuda.synchronize()
        _same_rows(view.cpu().numpy(), exp_back, pos, src, "partition_device positions")
        _check_partition(out[: n * 8].view(torch.int64).cpu().numpy(), counts.cpu().numpy(), order,
                         exp_counts, pos, src, "partition_device")


def _params(rows):
    return [pytest.param(*r, id="-".join(str(x) for x in r[:-1] if x != {}) + "-<"
                         + _instance(r[0], r[1], r[3], *r[4:6]) + ">") for r in rows]


GEOMETRY = [(c, p, n, per, "contig", {})
            for c in ("g3-pow2", "g3-pow2-mixed", "g3-any", "g3-any-64", "g3-512", "g1", "g2", "g4")
            for p in PAIRS for n in (N_BIG, N_SMALL) for per in (True, False)]
LAYOUT = ([(c, p, N_BIG, True, lay, {}) for c in ("g3-pow2", "g3-any") for p in ("f64-f64", "f32-f64")
           for lay in ("pad4", "rec", "row64", "wide", "off8")]
          + [("g3-pow2", "f32-f32", N_BIG, True, lay, {}) for lay in ("pad4", "rec", "off8")]
          + [(c, p, N_BIG, False, lay, {}) for c in ("g3-pow2", "g3-any") for p in ("f64-f64", "f32-f64")
             for lay in ("pad4", "wide")])
HOOKS = ([(c, p, N_BIG, True, "pad4", v) for c in ("g3-pow2", "g3-any") for p in PAIRS
          for v in ({"bin_generic": 1}, {"bin_unstaged": 1}, {"write_back": "all"}, {"tile_rounds": 1})]
         + [("g3-pow2", p, N_SMALL, True, "pad4", {"tile_rounds": 1}) for p in PAIRS]
         + [("g3-512", "f64-f64", N_BIG, True, "pad4", {"tile_rounds": 1}),
            ("g3-pow2", "f64-f64", N_BIG, True, "pad4", {"bin_generic": 1, "write_back": "all"})])


@pytest.mark.parametrize("case_id,pair,n_total,periodic,layout,variant", _params(GEOMETRY))
def test_two_pass_geometry(case_id, pair, n_total, periodic, layout, variant):
    """Every geometry class, dtype pair and dimensionality, both sizes."""
    _two_pass(case_id, pair, n_total, periodic, layout, variant)


@pytest.mark.parametrize("case_id,pair,n_total,periodic,layout,variant", _params(LAYOUT))
def test_two_pass_layouts(case_id, pair, n_total, periodic, layout, variant):
    """Every slab size NU 1..4 and the unstaged rows (wide, misaligned base)."""
    _two_pass(case_id, pair, n_total, periodic, layout, variant)


@pytest.mark.parametrize("case_id,pair,n_total,periodic,layout,variant", _params(HOOKS))
def test_two_pass_hooks(case_id, pair, n_total, periodic, layout, variant):
    """The hooks and options that pick another instance or write-back."""
    _two_pass(case_id, pair, n_total, periodic, layout, variant)


@pytest.mark.parametrize("case_id", ["g3-pow2", "g3-any"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_clean_slabs_are_not_written(case_id, pair):
    """write_back="changed": a sentinel in the padding column of the clean
    slabs (filler only) is still there afterwards, the -0.0 slab's only change
    is its sign flip, and the padding of every dirty slab is preserved -- a
    staged write-back that spilled a stale register copy would show here."""
    box, pos, src = _input(case_id, pair, N_BIG)
    exp_p, _, order, exp_counts = _expect(case_id, pair, N_BIG, True)
    n = len(pos)
    back = _backing(pos, 4)
    slab = np.arange(n) // E.SLAB
    clean = np.array([(src[slab == s] == E.FILLER).all() for s in range(slab.max() + 1)])[slab]
    assert clean.any() and not clean.all()
    back[clean, 3] = 77777.0
    P = GridPartitioner(E.case(case_id)["topo"], box)
    P.set_write_back("changed")
    store, view = _to_device(back)
    out, counts = P.partition_device(torch.arange(n, device="cuda").view(torch.uint8).reshape(-1),
                                     8, view[:, :3])
    got = view.cpu().numpy()
    assert G.same_bytes(got[clean], back[clean]), "a clean slab changed"
    assert (got[clean, 3] == 77777.0).all()
    assert G.same_bytes(got[:, 3], back[:, 3]), "padding of a dirty slab changed"
    _same_rows(got[:, :3], exp_p, pos, src, "positions")
    z = np.nonzero(src == E.NEG_ZERO)[0][0]
    changed = E.differing_rows(got[slab == slab[z]], back[slab == slab[z]])
    assert list(changed) == [z % E.SLAB], "the -0.0 slab's only change is the sign flip"
    _check_partition(out[: n * 8].view(torch.int64).cpu().numpy(), counts.cpu().numpy(), order,
                     exp_counts, pos, src, "partition_device")


# ---------------------------------------------------------------- fine side
def _fine_expect(case_id, pair, n_total, periodic):
    c = E.case(case_id)
    box, _, _ = _input(case_id, pair, n_total)
    exp_p, _, order, _ = _expect(case_id, pair, n_total, periodic)
    with np.errstate(all="ignore"):
        fid = ro.fine_cell_ids(c["topo"], c["fine"], box, exp_p)
    return fid[order]


@pytest.mark.parametrize("variant", [{}, {"bin_generic": 1}], ids=["default", "bin_generic"])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("case_id,n_total", [("fine-pow2", N_BIG), ("fine-any", N_BIG),
                                             ("fine-fallback", N_BIG), ("fine-pow2", N_SMALL)])
def test_fine_ids(case_id, n_total, pair, periodic, variant):
    """kSideFine: partition_device and partition_fields_device with
    fine_cells; the fine ids against ro.fine_cell_ids of the wrapped positions,
    permuted by the oracle's partition."""
    c = E.case(case_id)
    box, pos, src = _input(case_id, pair, n_total)
    exp_p, _, order, exp_counts = _expect(case_id, pair, n_total, periodic)
    exp_fid = _fine_expect(case_id, pair, n_total, periodic)
    n = len(pos)
    ids = torch.arange(n, dtype=torch.int64, device="cuda")
    with E.variant_hooks(_lib, variant):
        P = GridPartitioner(c["topo"], box)
        tpos = torch.from_numpy(pos.copy()).cuda()
        out, fid, counts = P.partition_device(ids.view(torch.uint8).reshape(-1), 8, tpos,
                                              periodic=periodic, fine_cells=c["fine"])
        torch.cuda.synchronize()
        _same_rows(tpos.cpu().numpy(), exp_p, pos, src, "partition_device positions")
        _check_partition(out[: n * 8].view(torch.int64).cpu().numpy(), counts.cpu().numpy(), order,
                         exp_counts, pos, src, "partition_device")
        got = fid.cpu().numpy().view(np.uint16).astype(np.int64)
        bad = np.nonzero(got != exp_fid)[0]
        assert len(bad) == 0, ("fine ids: " + E.describe(pos, src, order[bad]),
                               got[bad][:6], exp_fid[bad][:6])
        tpos = torch.from_numpy(pos.copy()).cuda()
        aux = torch.arange(n, dtype=torch.int32, device="cuda")
        outs, fid, counts = P.partition_fields_device(
            [ids.view(torch.uint8).reshape(-1), aux.view(torch.uint8).reshape(-1)], [8, 4], tpos,
            periodic=periodic, fine_cells=c["fine"])
        torch.cuda.synchronize()
        _same_rows(tpos.cpu().numpy(), exp_p, pos, src, "partition_fields_device positions")
        _check_partition(outs[0][: n * 8].view(torch.int64).cpu().numpy(), counts.cpu().numpy(),
                         order, exp_counts, pos, src, "partition_fields_device")
        assert np.array_equal(outs[1][: n * 4].view(torch.int32).cpu().numpy(), order)
        got = fid.cpu().numpy().view(np.uint16).astype(np.int64)
        bad = np.nonzero(got != exp_fid)[0]
        assert len(bad) == 0, "fields fine ids: " + E.describe(pos, src, order[bad])


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("box", [[1.0, 1.0, 1.0], [0.3, 62.5, 7.0]], ids=["pow2", "any"])
def test_fine_redistribution_two_ranks(box, pair):
    """redistribute_by_position(fine_cells=...) on two thread ranks (as
    test_fine_cells_position_dtypes) with edge rows."""
    size, topo, fine = 2, [2, 1, 1], [4, 2, 3]
    b = np.array(box, dtype=PAIRS[pair][1])
    rows = E.edge_rows(PAIRS[pair][0], b, topo, fine=fine, seed=31)
    allpos, _ = E.embed(rows, N_BIG, 32, b)
    parts = np.array_split(np.arange(len(allpos)), size)
    pos = [allpos[i].copy() for i in parts]
    data = [i.astype(np.int64) for i in parts]
    pos_o = [p.copy() for p in pos]
    with np.errstate(all="ignore"):
        plain = ro.redistribute_by_position_all_ranks(topo, b, size, data, pos_o)
        plain_pos = ro.redistribute_by_cell_number_all_ranks(
            size, pos_o, [ro.cell_number_from_position(ro.Geometry(topo, b, size), p.copy())
                          for p in pos_o])

    def fn(comm, r):
        return MPIGridRedistributor(comm, topo, b).redistribute_by_position(
            data[r], pos[r], fine_cells=fine)

    outs = run_ranks(size, fn)
    for r in range(size):
        with np.errstate(all="ignore"):
            fid = ro.fine_cell_ids(topo, fine, b, plain_pos[r])
        exp, exp_off = ro.fine_cell_sort(plain[r], fid, int(np.prod(fine)))
        assert G.same_bytes(pos[r], pos_o[r]), r
        assert np.array_equal(outs[r][1], exp_off), r
        bad = np.nonzero(outs[r][0] != exp)[0]
        assert len(bad) == 0, E.describe(allpos, np.arange(len(allpos)), exp[bad])


# ---------------------------------------------------------------- halo side
def _halo_inputs(case_id, pair):
    c = E.case(case_id)
    box, allpos, src = _input(case_id, pair, N_BIG)
    size = int(np.prod(c["topo"]))
    parts = np.array_split(np.arange(len(allpos)), size)
    return c, box, allpos, size, [allpos[i].copy() for i in parts], [i.astype(np.int64) for i in parts]


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("case_id", ["halo-222", "halo-321", "halo-111"])
def test_halo_fused_flags(case_id, pair, periodic):
    """kSideHalo: the face flags the bin kernel writes (bin_row_fast's own
    thresholds for in-box rows, coord_index's for the rest), through
    redistribute_by_position(overload_lengths=...) on one thread rank per
    cell, against the oracle's overload redistribution."""
    c, box, allpos, size, pos, data = _halo_inputs(case_id, pair)
    topo, ol = c["topo"], c["overload"]
    pos_o = [p.copy() for p in pos]
    with np.errstate(all="ignore"):
        exp = ro.redistribute_by_position_overload_all_ranks(topo, box, size, data, pos_o, ol,
                                                             periodic=periodic)
    wrapped = np.concatenate(pos_o)

    def fn(comm, r):
        return MPIGridRedistributor(comm if size > 1 else None, topo, box).redistribute_by_position(
            data[r], pos[r], periodic=periodic, overload_lengths=ol, return_positions=True)

    outs = run_ranks(size, fn)
    for r in range(size):
        got, gpos = outs[r]
        assert G.same_bytes(pos[r], pos_o[r]), r
        if not (len(got) == len(exp[r]) and (got == exp[r]).all()):
            extra = sorted(set(got.tolist()) ^ set(exp[r].tolist()))
            raise AssertionError(f"rank {r}: rows {extra[:8]} selected differently: "
                                 + E.describe(allpos, np.arange(len(allpos)), extra))
        assert G.same_bytes(gpos, wrapped[got]), r


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("case_id", ["halo-222", "halo-321", "halo-111"])
def test_halo_flags_kernel(case_id, pair, periodic):
    """halo_flags_kernel: the same rows, as they are (never wrapped), through
    exchange_overload_by_position against ro.exchange_overload_all_ranks."""
    c, box, allpos, size, pos, data = _halo_inputs(case_id, pair)
    topo, ol = c["topo"], c["overload"]
    with np.errstate(all="ignore"):
        exp = ro.exchange_overload_all_ranks(topo, box, size, data, pos, ol, periodic=periodic)

    def fn(comm, r):
        return MPIGridRedistributor(comm if size > 1 else None, topo, box) \
            .exchange_overload_by_position(data[r], pos[r].copy(), ol, periodic=periodic)

    outs = run_ranks(size, fn)
    for r in range(size):
        if not (len(outs[r]) == len(exp[r]) and (outs[r] == exp[r]).all()):
            extra = sorted(set(outs[r].tolist()) ^ set(exp[r].tolist()))
            raise AssertionError(f"rank {r}: rows {extra[:8]} selected differently: "
                                 + E.describe(allpos, np.arange(len(allpos)), extra))


def _ext_rows(dtype, box, topo, ol, seed):
    """Edge rows of an integer or float16 position dtype: every face and
    threshold with its two neighbours in that dtype (+-1 for integers), the
    box's multiples and the type's extremes, in the three row classes."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    vals = []
    for d in range(len(topo)):
        L, n = float(box[d]), int(topo[d])
        k = np.arange(n + 1) * (L / n)
        f = np.concatenate([k, k + ol[d], k - ol[d], [-L, 2 * L, -2 * L, 2.6 * L, -0.25 * L]])
        if dtype.kind == "i":
            info = np.iinfo(dtype)
            v = np.concatenate([f - 1, f, f + 1, [info.min, info.min + 1, info.max, info.max - 1]])
            vals.append(np.unique(v.astype(np.int64)).astype(dtype))
        else:
            f = E._cast(np.concatenate([f, E.fixed_values(L)]), dtype)
            v = np.concatenate([np.nextafter(f, dtype.type(-np.inf)), f,
                                np.nextafter(f, dtype.type(np.inf))])
            vals.append(E._unique_bits(v))
    out = []
    for d in range(len(topo)):
        m = len(vals[d])
        for lo, hi in ((0.05, 0.95), (-2.0, 3.0)):
            a = np.stack([E._cast(rng.uniform(lo, hi, m) * float(box[e]), dtype)
                          for e in range(len(topo))], axis=1)
            a[:, d] = vals[d]
            out.append(a)
    return np.concatenate(out)


@pytest.mark.parametrize("dtype,box,ol,fused",
                         [(np.int32, [64, 32, 48], [4, 4, 4], False),
                          (np.float16, [2.0, 1.0, 1.0], [0.125, 0.125, 0.125], True)],
                         ids=["int32", "float16"])
def test_halo_ext_positions(dtype, box, ol, fused):
    """pos_as_f64 in the halo kernels: int32 and float16 positions, box and
    thresholds exactly representable, on two thread ranks.  float16 runs the
    fused flags (bin_coord_ext + coord_index, kSideHalo) and halo_flags_kernel;
    int32 runs halo_flags_kernel only: its fused flags at integer thresholds
    are pinned by the reference's own halo_p4_i32pos / halo_p6_321_i32
    fixtures already (a ``<`` turned ``<=`` in coord_index fails them)."""
    size, topo = 2, [2, 1, 1]
    rows = _ext_rows(dtype, box, topo, ol, 41)
    parts = np.array_split(np.random.default_rng(42).permutation(len(rows)), size)
    pos = [rows[i].copy() for i in parts]
    data = [i.astype(np.int64) for i in parts]
    pos_o = [p.copy() for p in pos]
    with np.errstate(all="ignore"):
        exp = ro.redistribute_by_position_overload_all_ranks(topo, box, size, data, pos_o, ol)
        exp_x = ro.exchange_overload_all_ranks(topo, box, size, data, pos, ol)

    def fn(comm, r):
        R = MPIGridRedistributor(comm, topo, box)
        x = R.exchange_overload_by_position(data[r], pos[r].copy(), ol)
        if not fused:
            return None, x
        return R.redistribute_by_position(data[r], pos[r], overload_lengths=ol), x

    outs = run_ranks(size, fn)
    for r in range(size):
        if fused:
            assert G.same_bytes(pos[r], pos_o[r]), r
        for got, want, what in ((outs[r][0], exp[r], "fused"), (outs[r][1], exp_x[r], "flags")):
            if got is None:
                continue
            if not (len(got) == len(want) and (got == want).all()):
                extra = sorted(set(got.tolist()) ^ set(want.tolist()))
                raise AssertionError(f"{what}, rank {r}: " + E.describe(rows, np.arange(len(rows)),
                                                                        extra))


# ---------------------------------------------------------- one-pass kernels
def _segments(out, counts, cap, rb):
    return np.concatenate([out[b * cap * rb:(b * cap + int(c)) * rb] for b, c in enumerate(counts)])


@pytest.mark.parametrize("variant", [{}, {"bin_generic": 1}], ids=["default", "bin_generic"])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("case_id,n_total", [("g3-pow2", N_BIG), ("g3-pow2-mixed", N_BIG),
                                             ("g3-any", N_BIG), ("g3-any-64", N_BIG),
                                             ("g3-pow2", N_SMALL), ("fine-pow2", N_BIG),
                                             ("fine-any", N_BIG), ("fine-fallback", N_BIG)])
def test_onepass(case_id, n_total, pair, periodic, variant):
    """onepass_partition_kernel (records holding their positions) and
    onepass_fields_kernel (positions and ids as two fields): against the
    oracle, then byte for byte against the two-pass result on the same input."""
    c = E.case(case_id)
    fine = c.get("fine")
    box, pos, src = _input(case_id, pair, n_total)
    exp_p, _, order, exp_counts = _expect(case_id, pair, n_total, periodic)
    exp_fid = _fine_expect(case_id, pair, n_total, periodic) if fine else None
    n = len(pos)
    back = _backing(pos, 4)
    back[:, 3] = np.arange(n)                   # the record's payload: its row number
    rb = back.dtype.itemsize * 4
    exp_back = back.copy()
    exp_back[:, :3] = exp_p
    with E.variant_hooks(_lib, variant):
        P = GridPartitioner(c["topo"], box)
        _, rec = _to_device(back)
        out, fo, counts, cap = P.partition_onepass_device(rec.view(-1).view(torch.uint8), rb,
                                                          rec[:, :3], periodic=periodic,
                                                          fine_cells=fine)
        cnt = counts.cpu().numpy()
        assert np.array_equal(cnt, exp_counts), (cnt, exp_counts)
        _same_rows(rec.cpu().numpy(), exp_back, pos, src, "one-pass positions")
        one = _segments(out.cpu().numpy(), cnt, cap, rb)
        got = one.view(back.dtype).reshape(n, 4)
        _check_partition(got[:, 3].astype(np.int64), cnt, order, exp_counts, pos, src, "one-pass")
        assert G.same_bytes(got, exp_back[order])
        if fine:
            gf = _segments(fo.cpu().numpy().view(np.uint16), cnt, cap, 1).astype(np.int64)
            bad = np.nonzero(gf != exp_fid)[0]
            assert len(bad) == 0, "one-pass fine ids: " + E.describe(pos, src, order[bad])
        # the two-pass result on the same input, byte for byte
        _, rec2 = _to_device(back)
        res = P.partition_device(rec2.view(-1).view(torch.uint8), rb, rec2[:, :3],
                                 periodic=periodic, fine_cells=fine)
        torch.cuda.synchronize()
        assert np.array_equal(res[-1].cpu().numpy(), cnt)
        assert np.array_equal(res[0][: n * rb].cpu().numpy(), one), "one-pass vs two-pass rows"
        assert G.same_bytes(rec2.cpu().numpy(), rec.cpu().numpy()), "one-pass vs two-pass positions"
        if fine:
            assert np.array_equal(res[1].cpu().numpy().view(np.uint16).astype(np.int64), gf)
        # the SoA kernel: the positions and the ids as two fields
        tpos = torch.from_numpy(pos.copy()).cuda()
        ids = torch.arange(n, dtype=torch.int64, device="cuda")
        prb = pos.dtype.itemsize * 3
        outs, fo, counts, cap = P.partition_onepass_fields_device(
            [tpos.view(-1).view(torch.uint8), ids.view(torch.uint8).reshape(-1)], [prb, 8], tpos,
            periodic=periodic, fine_cells=fine)
        cnt = counts.cpu().numpy()
        assert np.array_equal(cnt, exp_counts), (cnt, exp_counts)
        _same_rows(tpos.cpu().numpy(), exp_p, pos, src, "one-pass fields positions")
        gi = _segments(outs[1].cpu().numpy(), cnt, cap, 8).view(np.int64)
        _check_partition(gi, cnt, order, exp_counts, pos, src, "one-pass fields")
        gp = _segments(outs[0].cpu().numpy(), cnt, cap, prb).view(pos.dtype).reshape(n, 3)
        assert G.same_bytes(gp, exp_p[order])
        if fine:
            gf = _segments(fo.cpu().numpy().view(np.uint16), cnt, cap, 1).astype(np.int64)
            bad = np.nonzero(gf != exp_fid)[0]
            assert len(bad) == 0, "one-pass fields fine ids: " + E.describe(pos, src, order[bad])


# ------------------------------------- cell_ids_kernel beyond one dimension
@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("case_id", ["g2", "g3-pow2", "g3-any", "g4"])
def test_cell_ids_more_dimensions(case_id, pair, periodic, as_torch):
    """get_cell_indexes_from_position / get_cell_number_from_position on the
    2-D, 3-D and 4-D edge rows (the goldens cover one dimension)."""
    c = E.case(case_id)
    box, rows = E.case_rows(c, *PAIRS[pair])
    exp_p = rows.copy()
    cell, idx = c_oracle.bin_positions(exp_p, c["topo"], box, periodic=periodic, want_idx=True)
    R = MPIGridRedistributor(SizedComm(int(np.prod(c["topo"]))), c["topo"], box)
    src = np.arange(len(rows))
    for want_idx in (True, False):
        p = torch.from_numpy(rows.copy()).cuda() if as_torch else rows.copy()
        got = (R.get_cell_indexes_from_position if want_idx
               else R.get_cell_number_from_position)(p, periodic=periodic)
        if as_torch:
            assert got.is_cuda
            got, p = got.cpu().numpy(), p.cpu().numpy()
        _same_rows(p, exp_p, rows, src, "positions")
        want = idx if want_idx else cell
        bad = np.nonzero((got != want).reshape(len(rows), -1).any(axis=1))[0]
        assert len(bad) == 0, E.describe(rows, src, bad)
