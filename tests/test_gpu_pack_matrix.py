"""Every pack kernel family of csrc/mgr_pack.hip (single array) and
csrc/mgr_pack_fields.hip (multi-field) against the numpy model
(tests/pack_model.py), straight on the C ABI, with the four options the
product reaches only along its own diagonal: redirect bin, drop bin, tile
ranges and the 2-byte side field.  Also mgr_tile_offsets beyond one kernarg
batch, mgr_bin_ids on edge ids, and the argument checks of the tile entry
points.  Bit-exact everywhere: whole buffers, sentinel guards included.

Which parametrisation reaches which kernel (the dispatch conditions of
launch_pack_rows, pack_w, pack_img and launch_pack_fields; nb counts the drop
bin where there is one, so a drop case has P = nb - 1 ranks):

| SHAPES entry            | condition that selects the kernel                      | kernel                    |
|-------------------------|--------------------------------------------------------|---------------------------|
| gen-3 / gen-6           | row_bytes 3 / 6: unit W = 1 / 2 (< 4: no coop)         | pack_kernel<1|2, u8>      |
| gen-100                 | 4-byte unit, row_bytes > 64                            | pack_kernel<4, u8>        |
| gen-1000                | row_bytes > 256                                        | pack_kernel<8, u8, wide>  |
| gen-8-nb1100            | nb > 1024 (above pack_many), 2-byte destinations       | pack_kernel<8, u16>       |
| coop-{4,8,16,32,64}     | nb <= 64, row_bytes <= 64, 16/8/4-byte units           | pack_coop_kernel          |
| coop-2                  | nb <= 64, row_bytes == 2                               | pack_coop_kernel<2, 1>    |
| coop-36-tr2048          | 36-B rows, 2048-row tiles: the image pack refuses      | pack_coop_kernel<4,9,2>   |
| img-36                  | 24..60 B, 4- not 16-byte multiple, nb <= 64            | pack_img_kernel<36>       |
| img-12 / img-60         | the same from 12 B with the pack_img_all hook          | pack_img_kernel<12|60>    |
| many-*                  | 64 < nb <= 1024, rows <= 64 B, tile = many_round_rows  | pack_many_kernel          |
|   nb 65, 256            |   1-byte destinations, 2048-row super-rounds           |   <.., uint8_t, 2>        |
|   nb 257, 513 / 1024    |   2-byte destinations, 2048 / 4096-row super-rounds    |   <.., uint16_t, 2 / 4>   |
| many-8-tr1024           | tile_rows != many_round_rows: pack_many refuses        | pack_kernel<8, u16>       |
| mf-cfg5-k{1,2,3}        | fields_kernel hook on (12, 12, 4, 8)                   | pack_fields_kernel / pack_fields_tile_kernel / pack_coop_fields_kernel |
| mf-24-8-k{1,2,3}        | the same on (24, 8)                                    | likewise                  |
| mf-mixed                | (12, 6, 8): two fast fields, the 6-byte one slow       | pack_fields_kernel + pack_kernel<2> |
| mf-4x128                | 4 x 128 B exceed one launch's LDS rows: two launches   | pack_fields_kernel (fields_pass_any) x 2 |
| coop-*-generic          | the pack_generic hook: pack_coop_u refuses             | pack_kernel<4|8|16|2, u8> |
| img-*-generic-tr2048    | the hook + 2048-row tiles: pack_img refuses (> 1024    | pack_kernel<4, u8>        |
|                         |   rows), then pack_coop_u refuses (the hook)           |                           |
| many-*-generic-tr1024   | the hook + 1024-row tiles: pack_many refuses (tile !=  | pack_kernel<8, u8> /      |
|                         |   many_round_rows; it does not read the hook)          |   <16, u16> / <4, u16>    |
| mf-cfg5-generic         | the hook: no field is "fast"                           | one launch_pack per field: pack_coop refuses, pack_kernel<4|8, u8> |

With nb == 2 and a drop bin (coop-*-nb2, img-36-nb2: one rank plus the drop
bin) the coop and image launchers take their selection variants (sel / SEL:
the loads of dropped rows are skipped), the halo's shape.

Side ids: the coop and image kernels and the three multi-field kernels carry
them in the launch; every other kernel leaves them to a second 2-byte pack
(SideField::used, side_done), which is the coop-2 kernel for nb <= 64 and
pack_kernel<2> otherwise.

Redirect placement.  Every launcher takes the widest unit W that divides the
row and every pointer (launch_pack_rows, coop_unit: src | dst | row_bytes |
redirect_dst; pack_img and the multi-field "fast" test want 4-byte outputs).
Sources and dst are 256-byte aligned here, so without a redirect W is U, the
widest of 16/8/4/2/1 dividing row_bytes.  A whole number of rows into its
buffer a redirect pointer keeps W = U (U divides the row), so the misaligned
placements add a byte shift that U does not divide; _run_case asserts that the
alignment word really loses bits.  One field is shifted (the only one; of a
field set the last for "half" / "quarter", the first for "two" / "one"), the
others and the 2-byte ids sit one row in:

| placement | shift        | single field                                   | field set                              |
|-----------|--------------|------------------------------------------------|----------------------------------------|
| half      | U / 2        | 16/32/64 B: W 16 -> 8, 8 B: 8 -> 4, both still | cfg5, (24, 8): the 8-B field +4, its   |
|           |              | coop / many; 4-multiples (36, 12, 60, 100 B):  | coop unit 8x1 -> 4x2: no signature,    |
|           |              | +2, pack_img / coop / many refuse ->           | pack_coop_fields falls through to      |
|           |              | pack_kernel<2>; 6 B: W 1; 2 B: W 1, not coop-2 | pack_fields_kernel; tile kernel: W 4   |
| quarter   | U / 4        | 16/32/64 B: W 4; 8 B: W 2 -> pack_kernel<2>;   | the 8-B field +2: slow (pack_kernel<2>)|
|           | (U < 4: U/2) | 4-multiples: +1 -> pack_kernel<1>              | 4x128: the last field +4, still fast   |
| two       | 2            | rows with U >= 4: W 2 -> pack_kernel<2>        | the first field slow; (24, 8) and      |
|           |              |                                                |   mixed: < 2 fast fields, all slow     |
| one       | 1            | W 1 -> pack_kernel<1>                          | the first field slow, pack_kernel<1>   |

(3-B rows have U = 1: nothing to lose; "two" leaves 6-B and 2-B rows at W 2.)
With W < 4 no kernel carries the side ids, so they take the second 2-byte pack
there.

OPTIONS is the option design every shape runs: each redirect position (none,
first, middle, last, an empty bin, a bin with ~90 % of the rows) x chunked
tiles, side ids x chunked tiles x redirect, the drop bin, every redirect
placement, the three tile patterns and the four row counts.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests.pack_model import pack_model, tile_offsets_model

pytestmark = pytest.mark.gpu

from mpi_grid_redistribute_amd import _lib  # noqa: E402

SENT = 0xAB
GUARD = 256          # sentinel bytes before and after every output
MGR_EINVAL = -1


@pytest.fixture(autouse=True)
def _gpu_and_hooks():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    try:
        yield
    finally:
        for k, v in _lib.HOOK_DEFAULTS.items():
            _lib.test_hook(k, v)


# ------------------------------------------------------------------ helpers
def _dev(a):
    """A numpy array's bytes on the device (16 spare bytes: the multi-field
    kernels stage sources in 16-byte units)."""
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    t[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t


class Guarded:
    """An output of ``rows`` rows of ``rb`` bytes, ``lead_rows`` rows and
    ``shift`` bytes into its buffer, between two sentinel guards; everything
    pre-filled with the sentinel."""

    def __init__(self, rows, rb, lead_rows=0, shift=0):
        self.off = GUARD + lead_rows * rb + shift
        self.rows, self.rb = rows, rb
        self.t = torch.full((self.off + rows * rb + GUARD,), SENT, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off

    def check(self, want, what):
        """The whole buffer, guards included, against the model's payload."""
        full = np.full(self.t.numel(), SENT, dtype=np.uint8)
        full[self.off:self.off + self.rows * self.rb] = want.reshape(-1)
        got = self.t.cpu().numpy()
        if not np.array_equal(got, full):
            bad = np.flatnonzero(got != full)
            raise AssertionError(
                f"{what}: {bad.size} bytes differ, first at byte {bad[0] - self.off} of the "
                f"payload ({self.rows} rows of {self.rb} B; row {(bad[0] - self.off) // self.rb})")


def _vp(values):
    return (ctypes.c_void_p * len(values))(*values)


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def _plan(P):
    """A [P]-topology plan of P destinations (mgr_bin_ids: the drop bin is P)."""
    topo = np.asarray([P], dtype=np.int64)
    box = np.asarray([1.0], dtype=np.float64)
    h = ctypes.c_void_p()
    _lib.call("mgr_plan_create", 1, topo.ctypes.data_as(ctypes.c_void_p),
              box.ctypes.data_as(ctypes.c_void_p), _lib.MGR_F64, int(P), ctypes.byref(h))
    return h


class Scanned:
    """Destinations made by the public producers, scanned: mgr_bin_ids on int32
    ids in [-1, P] (drop bin P, nb = P + 1) or mgr_count_ids on uint16 ids
    (nb = P); ``dest`` is the device's own destination array read back."""

    def __init__(self, ids, P, drop, tile_rows):
        self.n = n = int(ids.size)
        self.nb = nb = P + 1 if drop else P
        self.drop_bin = P if drop else -1
        self.tile_rows = tile_rows
        self.T = (n + tile_rows - 1) // tile_rows
        s = _lib.stream_handle()
        lib = _lib.load()
        width = int(lib.mgr_dest_bytes(nb))
        self.ws = torch.empty(int(lib.mgr_workspace_bytes(n, nb, tile_rows)), dtype=torch.uint8,
                              device="cuda")
        self.dest_t = torch.zeros(n * width + 64, dtype=torch.uint8, device="cuda")
        self.counts_t = torch.full((nb,), -7, dtype=torch.int64, device="cuda")
        if drop:
            self.ids_t = _dev(ids.astype(np.int32))
            plan = _plan(P)
            try:
                _lib.call("mgr_bin_ids", plan, _lib.ptr(self.ids_t), _lib.MGR_I32, n,
                          _lib.ptr(self.dest_t), tile_rows, _lib.ptr(self.ws), s)
            finally:
                lib.mgr_plan_destroy(plan)
            want = np.where((ids < 0) | (ids >= P), P, ids).astype(np.int64)
        else:
            self.ids_t = _dev(ids.astype(np.uint16))
            bad = torch.zeros(1, dtype=torch.int32, device="cuda")
            _lib.call("mgr_count_ids", _lib.ptr(self.ids_t), n, nb, tile_rows,
                      _lib.ptr(self.dest_t), _lib.ptr(bad), _lib.ptr(self.ws), s)
            want = ids.astype(np.int64)
        _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(self.ws), _lib.ptr(self.counts_t), s)
        raw = self.dest_t.cpu().numpy()[:n * width]
        self.dest = raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[width]).astype(np.int64)
        assert np.array_equal(self.dest, want)
        assert np.array_equal(self.counts_t.cpu().numpy(), np.bincount(want, minlength=nb))
        if not drop:
            assert int(bad.item()) == 0


def _tile_rows(max_row_bytes, nb):
    return int(_lib.load().mgr_tile_rows(int(max_row_bytes), int(nb)))


# -------------------------------------------------------------- the matrix
def S(name, fields, nb, **hooks):
    return {"name": name, "fields": tuple(fields), "nb": nb, "hooks": hooks}


SHAPES = [
    # generic pack_kernel
    S("gen-3", [3], 9), S("gen-6", [6], 9), S("gen-100", [100], 9), S("gen-1000", [1000], 5),
    S("gen-8-nb1100", [8], 1100),
    # cooperative pack: every row size, every nb
    S("coop-4-nb2", [4], 2), S("coop-8-nb9", [8], 9), S("coop-16-nb64", [16], 64),
    S("coop-32-nb2", [32], 2), S("coop-64-nb9", [64], 9), S("coop-2-nb64", [2], 64),
    S("coop-2-nb9", [2], 9), S("coop-8-nb64", [8], 64), S("coop-16-nb2", [16], 2),
    S("coop-36-tr2048", [36], 9, tile_rounds=32),
    # image pack
    S("img-36-nb9", [36], 9), S("img-36-nb64", [36], 64), S("img-36-nb2", [36], 2),
    S("img-12-nb9", [12], 9, pack_img_all=1), S("img-60-nb64", [60], 64, pack_img_all=1),
    # many-bin pack: both destination widths, both super-round sizes
    S("many-8-nb65", [8], 65), S("many-36-nb256", [36], 256), S("many-64-nb257", [64], 257),
    S("many-8-nb513", [8], 513), S("many-36-nb1024", [36], 1024), S("many-64-nb65", [64], 65),
    S("many-8-tr1024", [8], 300, tile_rounds=16),
    # multi-field packs
    S("mf-cfg5-k1", [12, 12, 4, 8], 9, fields_kernel=1),
    S("mf-cfg5-k2", [12, 12, 4, 8], 9, fields_kernel=2),
    S("mf-cfg5-k3", [12, 12, 4, 8], 9, fields_kernel=3),
    S("mf-24-8-k1", [24, 8], 64, fields_kernel=1),
    S("mf-24-8-k2", [24, 8], 64, fields_kernel=2),
    S("mf-24-8-k3", [24, 8], 64, fields_kernel=3),
    S("mf-mixed", [12, 6, 8], 9),
    S("mf-4x128", [128, 128, 128, 128], 9),
    # the same shapes with the cooperative kernels switched off
    S("coop-4-nb2-generic", [4], 2, pack_generic=1),
    S("coop-8-nb9-generic", [8], 9, pack_generic=1),
    S("coop-16-nb64-generic", [16], 64, pack_generic=1),
    S("coop-32-nb2-generic", [32], 2, pack_generic=1),
    S("coop-64-nb9-generic", [64], 9, pack_generic=1),
    S("coop-2-nb64-generic", [2], 64, pack_generic=1),
    # (the image and many-bin launchers do not read the hook: tiles they refuse)
    S("img-36-nb9-generic-tr2048", [36], 9, pack_generic=1, tile_rounds=32),
    S("img-12-nb9-generic-tr2048", [12], 9, pack_img_all=1, pack_generic=1, tile_rounds=32),
    S("img-60-nb64-generic-tr2048", [60], 64, pack_img_all=1, pack_generic=1, tile_rounds=32),
    S("many-8-nb65-generic-tr1024", [8], 65, pack_generic=1, tile_rounds=16),
    S("many-64-nb257-generic-tr1024", [64], 257, pack_generic=1, tile_rounds=16),
    S("many-36-nb1024-generic-tr1024", [36], 1024, pack_generic=1, tile_rounds=16),
    S("mf-cfg5-generic", [12, 12, 4, 8], 9, pack_generic=1),
]

# redirect: none / first / mid / last, "empty" = a middle bin without rows,
#   "heavy" = a middle bin with ~90 % of the rows (whole tiles are one bin)
# tiles: "pack" = all tiles by mgr_pack / mgr_pack_ids (multi-field: mgr_pack_fields),
#   "fields" = mgr_pack_fields with tile_end = -1, "chunks" = 4 chunks T * c // 4,
#   "ragged" = a split with an empty and a one-tile chunk; chunks packed in reverse
# n: "1", "63", "tile" = tile_rows, "big" = 5 * tile_rows + 37
# placement of redirect_dst: "start" = at its buffer's start, else one row in
#   plus the byte shift of the header's placement table
# (redirect, drop, tiles, side ids, redirect placement, n)
OPTIONS = [
    ("none", False, "pack", False, "start", "big"),
    ("none", True, "chunks", True, "start", "big"),
    ("first", True, "chunks", True, "half", "big"),
    ("mid", False, "chunks", True, "start", "big"),
    ("last", True, "chunks", False, "quarter", "big"),
    ("last", False, "ragged", True, "two", "big"),
    ("heavy", True, "ragged", True, "one", "big"),
    ("empty", False, "ragged", False, "start", "big"),
    ("first", False, "fields", True, "half", "tile"),
    ("last", True, "fields", False, "start", "63"),
    ("mid", True, "pack", True, "quarter", "1"),
    ("first", False, "chunks", False, "start", "63"),
]


def _unit(*words):
    """The widest of 16/8/4/2/1 dividing every pointer and size given: the
    launchers' unit choice."""
    a = 0
    for w in words:
        a |= int(w)
    return next(W for W in (16, 8, 4, 2, 1) if a % W == 0)


def _shifts(fields, place):
    """Byte shift of every field's redirect pointer for a placement."""
    sh = [0] * len(fields)
    if place == "start":
        return sh
    f = len(fields) - 1 if place in ("half", "quarter") else 0
    U = _unit(fields[f])
    sh[f] = {"half": max(U // 2, 1), "quarter": max(U // 4, 1) if U >= 4 else max(U // 2, 1),
             "two": 2, "one": 1}[place]
    return sh


def _ids_for(rng, n, P, drop, redirect_bin, kind):
    """Rank ids of n rows: uniform over the P ranks with bin 1 % P thinned, the
    redirect bin empty or heavy where asked, and with a drop bin ~10 % of the
    rows outside [0, P) (-1 and P)."""
    ids = rng.integers(0, P, size=n).astype(np.int64)
    if redirect_bin >= 0 and kind == "heavy":
        ids = np.where(rng.random(n) < 0.9, redirect_bin, ids)
    if redirect_bin >= 0 and kind == "empty" and P > 1:
        ids = np.where(ids == redirect_bin, (redirect_bin + 1) % P, ids)
    if drop:
        u = rng.random(n)
        ids = np.where(u < 0.05, -1, np.where(u < 0.10, P, ids))
    return ids


def _bounds(tiles, T):
    if tiles == "chunks":
        return [T * c // 4 for c in range(5)]
    if tiles == "ragged":
        return [0, 0, min(1, T), max(min(1, T), T - 2), T]
    return None


def _run_case(shape, opt, seed):
    redirect, drop, tiles, side, place, nkind = opt
    fields, nb = shape["fields"], shape["nb"]
    for k, v in shape["hooks"].items():
        _lib.test_hook(k, v)
    P = nb - 1 if drop else nb
    tile_rows = _tile_rows(max(fields), nb)
    n = {"1": 1, "63": 63, "tile": tile_rows, "big": 5 * tile_rows + 37}[nkind]
    redirect_bin = {"none": -1, "first": 0, "last": P - 1}.get(redirect, P // 2)
    rng = np.random.default_rng(seed)
    sc = Scanned(_ids_for(rng, n, P, drop, redirect_bin, redirect), P, drop, tile_rows)
    if redirect == "empty" and P > 1:
        assert not (sc.dest == redirect_bin).any()
    srcs = [rng.integers(0, 256, size=(n, rb), dtype=np.uint8) for rb in fields]
    side_ids = rng.integers(0, 1 << 16, size=n, dtype=np.uint16) if side else None
    src_t = [_dev(a) for a in srcs]
    side_t = _dev(side_ids) if side else None

    def model(t0=0, t1=-1):
        return pack_model(srcs, sc.dest, nb, sc.drop_bin, redirect_bin, tile_rows, t0, t1,
                          ids=side_ids, sentinel=SENT)

    whole = model()
    nred = whole.red[0].shape[0]
    lead = 0 if place == "start" else 1
    shifts = _shifts(fields, place)
    dst = [Guarded(n, rb) for rb in fields]
    red = [Guarded(nred, rb, lead, sh) for rb, sh in zip(fields, shifts)]
    idd, idr = Guarded(n, 2), Guarded(nred, 2, lead)
    r = redirect_bin >= 0
    for f, rb in enumerate(fields):
        # the placement does what the header says: without the redirect pointer
        # the unit is U, with the shifted one it is narrower
        U = _unit(rb)
        assert _unit(src_t[f].data_ptr(), dst[f].ptr, rb) == U
        want = min(U, _unit(shifts[f])) if shifts[f] else U
        assert place not in ("half", "quarter") or f != len(fields) - 1 or U == 1 or want < U
        assert _unit(src_t[f].data_ptr(), dst[f].ptr, rb, red[f].ptr) == want
    s = _lib.stream_handle()
    common = (n, _lib.ptr(sc.dest_t), nb, sc.drop_bin, tile_rows, _lib.ptr(sc.ws))
    ids3 = (_lib.ptr(side_t), idd.ptr if side else None, idr.ptr if side and r else None)

    def pack_fields(t0, t1):
        _lib.call("mgr_pack_fields", len(fields), _vp([t.data_ptr() for t in src_t]), _i64(fields),
                  *common, _vp([d.ptr for d in dst]), redirect_bin,
                  _vp([q.ptr for q in red]) if r else None, *ids3, t0, t1, s)

    def check(m, what):
        for f in range(len(fields)):
            dst[f].check(m.dst[f], f"{what}: dst of field {f}")
            red[f].check(m.red[f], f"{what}: redirect_dst of field {f}")
        # without side ids the id outputs were never passed: still sentinel
        idd.check(m.ids_dst if side else np.full((n, 2), SENT, np.uint8), f"{what}: ids_dst")
        idr.check(m.ids_red if side else np.full((nred, 2), SENT, np.uint8),
                  f"{what}: ids_redirect_dst")

    single = len(fields) == 1
    one = (_lib.ptr(src_t[0]), fields[0]) + common + (dst[0].ptr, redirect_bin,
                                                       red[0].ptr if r else None)
    bounds = _bounds(tiles, sc.T)
    if bounds is None:
        if tiles == "fields" or not single:
            pack_fields(0, -1)
        elif side:
            _lib.call("mgr_pack_ids", *one, *ids3, s)
        else:
            _lib.call("mgr_pack", *one, s)
        check(whole, "all tiles")
        return
    acc = None
    for c in reversed(range(len(bounds) - 1)):
        if single and tiles == "chunks":
            _lib.call("mgr_pack_tiles", *one, *ids3, bounds[c], bounds[c + 1], s)
        else:
            pack_fields(bounds[c], bounds[c + 1])
        acc = model(bounds[c], bounds[c + 1]).over(acc)
        check(acc, f"after chunk {c} = tiles [{bounds[c]}, {bounds[c + 1]})")
    check(whole, "after the last chunk")


def _opt_id(o):
    return "-".join([o[0], "drop" if o[1] else "keep", o[2], "ids" if o[3] else "noids",
                     o[4], "n" + o[5]])


@pytest.mark.parametrize("opt", OPTIONS, ids=_opt_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s["name"])
def test_pack_matrix(shape, opt):
    _run_case(shape, opt, seed=1 + SHAPES.index(shape) * 100 + OPTIONS.index(opt))


# --------------------------------------------------------- mgr_tile_offsets
@pytest.mark.parametrize("nb", [9, 300])
def test_tile_offsets_batches(nb):
    """Tile lists longer than one 64-entry kernarg batch, with 0, T, repeats
    and unsorted entries, on one scanned workspace of T = 132 tiles."""
    _lib.test_hook("tile_rounds", 1)
    tile_rows = _tile_rows(8, nb)
    assert tile_rows == 64
    n = 131 * 64 + 5
    rng = np.random.default_rng(nb)
    sc = Scanned(rng.integers(0, nb, size=n).astype(np.int64), nb, False, tile_rows)
    T = sc.T
    assert T == 132
    s = _lib.stream_handle()
    lists = {
        1: [T], 64: list(rng.permutation(T)[:64]),
        65: [0, T, T, 0, 7, 7] + list(rng.integers(0, T + 1, size=59)),
        130: list(rng.permutation(T + 1)[:128]) + [T, 0],
    }
    for k, tiles in lists.items():
        assert len(tiles) == k
        out = Guarded(k * nb, 8)
        _lib.call("mgr_tile_offsets", _lib.ptr(sc.ws), n, nb, tile_rows, _i64(tiles), k, out.ptr, s)
        want = tile_offsets_model(sc.dest, nb, tile_rows, tiles)
        out.check(want.view(np.uint8), f"tile offsets of {k} tiles")
    lib = _lib.load()
    out = Guarded(4097 * nb, 8)
    assert lib.mgr_tile_offsets(_lib.ptr(sc.ws), n, nb, tile_rows, _i64([0] * 4097), 4097, out.ptr,
                                s) == MGR_EINVAL
    assert lib.mgr_tile_offsets(_lib.ptr(sc.ws), n, nb, tile_rows, _i64([0, T + 1]), 2, out.ptr,
                                s) == MGR_EINVAL
    assert lib.mgr_tile_offsets(_lib.ptr(sc.ws), n, nb, tile_rows, _i64([0, -1]), 2, out.ptr,
                                s) == MGR_EINVAL
    out.check(np.full((4097 * nb, 8), SENT, np.uint8), "refused calls write nothing")


# -------------------------------------------------------- mgr_bin_ids edges
_I64_EDGES = [2**32, 2**32 + 1, -(2**63), 2**63 - 1, -1, 0, 1, 2**31, -(2**31), 2**16, 2**8, 255,
              256, 257]
_I32_EDGES = [-(2**31), 2**31 - 1, -1, 0, 1, 2**16, 2**8, 255, 256, 257, -2, 65535, 65536]
_F_EDGES = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e20, -1e20, 0.5, -0.5, 16777217.0, 2.0**32,
            2.0**32 + 1, 255.0, 256.0, 257.0, 1.0, 0.99999]


@pytest.mark.parametrize("nbins", [1, 3, 255, 256, 4095])
@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float32, np.float64])
def test_bin_ids_edge_ids(nbins, dtype):
    """dest = id when 0 <= id < nbins and id is integral, else the drop bin
    nbins; computed in int64 / float64 of the value the array stores.  nbins
    255 / 256 are the two sides of the mgr_dest_bytes step (nbins + 1 bins)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(nbins * 8 + dt.itemsize + (dt.kind == "f"))
    near = [nbins - 1, nbins, nbins + 1, nbins - 2]
    if dt.kind == "f":
        edges = _F_EDGES + [float(v) for v in near] + [nbins - 0.5, nbins - 1 + 0.25]
    else:
        edges = (_I64_EDGES if dt.itemsize == 8 else _I32_EDGES) + near
    n = 5 * 64 + 37
    vals = np.concatenate([np.asarray(edges, dtype=dt),
                           rng.integers(0, nbins, size=n).astype(dt)])[:n]
    vals = vals[rng.permutation(n)]
    # every edge again in the ragged last round
    vals[n - len(edges):] = np.asarray(edges, dtype=dt)[:n]
    wide = vals.astype(np.float64 if dt.kind == "f" else np.int64)
    with np.errstate(invalid="ignore"):
        ok = (wide >= 0) & (wide < nbins)
        if dt.kind == "f":
            ok &= wide == np.trunc(wide)
    want = np.where(ok, np.where(ok, wide, 0).astype(np.int64), nbins)
    nb = nbins + 1
    tile_rows = _tile_rows(8, nb)
    lib = _lib.load()
    width = int(lib.mgr_dest_bytes(nb))
    assert width == (1 if nb <= 256 else 2)
    s = _lib.stream_handle()
    ids_t = _dev(vals)
    ws = torch.empty(int(lib.mgr_workspace_bytes(n, nb, tile_rows)), dtype=torch.uint8, device="cuda")
    dest = Guarded(n, width)
    counts = Guarded(nb, 8)
    code = {"i4": _lib.MGR_I32, "i8": _lib.MGR_I64, "f4": _lib.MGR_F32, "f8": _lib.MGR_F64}[
        dt.kind + str(dt.itemsize)]
    plan = _plan(nbins)
    try:
        _lib.call("mgr_bin_ids", plan, _lib.ptr(ids_t), code, n, dest.ptr, tile_rows, _lib.ptr(ws), s)
    finally:
        lib.mgr_plan_destroy(plan)
    _lib.call("mgr_scan", n, nb, tile_rows, _lib.ptr(ws), counts.ptr, s)
    dest.check(want.astype({1: np.uint8, 2: np.uint16}[width]).view(np.uint8), "dest")
    counts.check(np.bincount(want, minlength=nb).astype(np.int64).view(np.uint8), "bin_counts")


# ------------------------------------------- argument checks (host only)
def test_tile_entry_points_refuse_bad_arguments():
    nb, n = 9, 5 * 64 + 37
    _lib.test_hook("tile_rounds", 1)
    tile_rows = _tile_rows(8, nb)
    rng = np.random.default_rng(11)
    sc = Scanned(rng.integers(0, nb, size=n).astype(np.int64), nb, False, tile_rows)
    T = sc.T
    src = rng.integers(0, 256, size=(n, 8), dtype=np.uint8)
    ids = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
    src_t, ids_t = _dev(src), _dev(ids)
    dst, red, idd, idr = Guarded(n, 8), Guarded(n, 8), Guarded(n, 2), Guarded(n, 2)
    lib = _lib.load()
    s = _lib.stream_handle()

    def tiles(t0, t1, redirect_bin=-1, red_ptr=None, ids_on=False, idr_ptr=None):
        return lib.mgr_pack_tiles(_lib.ptr(src_t), 8, n, _lib.ptr(sc.dest_t), nb, -1, tile_rows,
                                  _lib.ptr(sc.ws), dst.ptr, redirect_bin, red_ptr,
                                  _lib.ptr(ids_t) if ids_on else None, idd.ptr if ids_on else None,
                                  idr_ptr, t0, t1, s)

    def fields(t0, t1, redirect_bin=-1, red_ptr=None, ids_on=False, idr_ptr=None):
        return lib.mgr_pack_fields(1, _vp([src_t.data_ptr()]), _i64([8]), n, _lib.ptr(sc.dest_t),
                                   nb, -1, tile_rows, _lib.ptr(sc.ws), _vp([dst.ptr]), redirect_bin,
                                   _vp([red_ptr]) if red_ptr else None,
                                   _lib.ptr(ids_t) if ids_on else None, idd.ptr if ids_on else None,
                                   idr_ptr, t0, t1, s)

    for call in (tiles, fields):
        assert call(-1, 2) == MGR_EINVAL                      # tile_begin < 0
        assert call(3, 2) == MGR_EINVAL                       # tile_end < tile_begin
        assert call(0, T + 1) == MGR_EINVAL                   # tile_end > T
        assert call(0, T, redirect_bin=nb, red_ptr=red.ptr) == MGR_EINVAL
        assert call(0, T, redirect_bin=2) == MGR_EINVAL       # a redirect with no buffer
        assert call(0, T, redirect_bin=2, red_ptr=red.ptr, ids_on=True) == MGR_EINVAL
        assert call(2, 2, redirect_bin=2, red_ptr=red.ptr, ids_on=True,
                    idr_ptr=idr.ptr) == _lib.MGR_OK           # an empty range: nothing written
        assert call(T, T) == _lib.MGR_OK
    assert tiles(0, -1) == MGR_EINVAL     # (mgr_pack_fields alone reads tile_end < 0 as "all")
    for g, rb in ((dst, 8), (red, 8), (idd, 2), (idr, 2)):
        g.check(np.full((n, rb), SENT, np.uint8), "refused and empty calls write nothing")
