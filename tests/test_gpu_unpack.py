"""The unpack kernels (csrc/mgr_unpack.hip) against numpy, straight on the C
ABI: the public count producers and mgr_scan, mgr_pack into buffers of known
content, then mgr_unpack.  The expectation is computed here -- out[order] =
packed rows with order = argsort(dest, kind="stable") -- and the pack itself is
checked against the same model first, so nothing rests on the pack alone:
unpack(pack(x)) == x, and unpacking a buffer that holds its own slot indexes
gives the inverse permutation.  Byte-exact everywhere, guards included.

Which case reaches which kernel (launch_unpack_fields / unpack_rows):
  <= 64 bins, rows of <= 16 units of 4/8/16 bytes, tiles <= 1024 rows
                      -> unpack_coop_kernel<U, 0, 0, 0> (4/8/12/16/24/32/36/64 B)
  the SoA sets of pack_coop_fields, hook unpack_kernel 0
                      -> unpack_coop_kernel<U0, U1, U2, U3>, one launch
  everything else     -> unpack_kernel<W, u8 | u16, wide> (1/2/3 B: W 1/2/1;
                         68 B: W 4; 260 B: wide; 65/125 bins; 300 bins: u16)
  hook unpack_kernel 1: the generic kernel for every shape; 2: field sets go
  field by field through the single-field cooperative kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mpi_grid_redistribute_amd import _lib  # noqa: E402

FILL = 0xA5
GUARD = 128


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
def _vp(values):
    return (ctypes.c_void_p * len(values))(*values)


def _i64(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


class Buf:
    """``rows`` rows of ``rb`` bytes between two guards, ``shift`` bytes into a
    256-byte aligned allocation, pre-filled with FILL (or given content)."""

    def __init__(self, rows, rb, shift=0, content=None):
        self.rows, self.rb, self.off = rows, rb, GUARD + shift
        self.t = torch.full((self.off + rows * rb + GUARD,), FILL, dtype=torch.uint8,
                            device="cuda")
        if content is not None and rows:
            raw = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
            assert raw.size == rows * rb
            self.t[self.off:self.off + raw.size] = torch.from_numpy(raw.copy()).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off

    def fill(self):
        self.t.fill_(FILL)

    def get(self):
        """The payload as (rows, rb) bytes; the guards must be untouched."""
        a = self.t.cpu().numpy()
        assert (a[:self.off] == FILL).all() and (a[self.off + self.rows * self.rb:] == FILL).all(), \
            "a write outside the buffer"
        return a[self.off:self.off + self.rows * self.rb].reshape(self.rows, self.rb)


def _plan(P):
    topo = np.asarray([P], dtype=np.int64)
    box = np.asarray([1.0], dtype=np.float64)
    h = ctypes.c_void_p()
    _lib.call("mgr_plan_create", 1, topo.ctypes.data_as(ctypes.c_void_p),
              box.ctypes.data_as(ctypes.c_void_p), _lib.MGR_F64, int(P), ctypes.byref(h))
    return h


class Scanned:
    """dest + workspace as the public producers and mgr_scan leave them:
    mgr_bin_ids on int32 ids (out-of-range ids -> the drop bin nb - 1) when
    ``drop``, else mgr_count_ids on uint16 ids."""

    def __init__(self, ids, nb, drop, tile_rows=None, hint_rb=32):
        lib = _lib.load()
        self.n = n = int(ids.size)
        self.nb, self.drop_bin = nb, (nb - 1 if drop else -1)
        self.tile_rows = tr = tile_rows or int(lib.mgr_tile_rows(hint_rb, nb))
        self.T = (n + tr - 1) // tr
        s = _lib.stream_handle()
        width = int(lib.mgr_dest_bytes(nb))
        self.ws = torch.empty(int(lib.mgr_workspace_bytes(n, nb, tr)), dtype=torch.uint8,
                              device="cuda")
        self.dest_t = torch.zeros(n * width + 64, dtype=torch.uint8, device="cuda")
        self.counts_t = torch.full((nb,), -7, dtype=torch.int64, device="cuda")
        if drop:
            P = nb - 1
            self.ids_t = torch.from_numpy(ids.astype(np.int32)).cuda()
            plan = _plan(P)
            try:
                _lib.call("mgr_bin_ids", plan, _lib.ptr(self.ids_t), _lib.MGR_I32, n,
                          _lib.ptr(self.dest_t), tr, _lib.ptr(self.ws), s)
            finally:
                lib.mgr_plan_destroy(plan)
            self.dest = np.where((ids < 0) | (ids >= P), P, ids).astype(np.int64)
        else:
            self.ids_t = torch.from_numpy(ids.astype(np.uint16).view(np.int16)).cuda()
            _lib.call("mgr_count_ids", _lib.ptr(self.ids_t), n, nb, tr, _lib.ptr(self.dest_t),
                      None, _lib.ptr(self.ws), s)
            self.dest = ids.astype(np.int64)
        _lib.call("mgr_scan", n, nb, tr, _lib.ptr(self.ws), _lib.ptr(self.counts_t), s)
        assert np.array_equal(self.counts_t.cpu().numpy(), np.bincount(self.dest, minlength=nb))

    def model(self, redirect_bin):
        """(slot, where) of every row: where 0 = dst, 1 = redirect buffer, 2 =
        dropped; and the row counts of dst and of the redirect buffer."""
        d = self.dest
        order = np.argsort(d, kind="stable")
        counts = np.bincount(d, minlength=self.nb)
        starts = np.concatenate([[0], np.cumsum(counts)])
        slot = np.empty(self.n, dtype=np.int64)
        slot[order] = np.arange(self.n)
        where = np.zeros(self.n, dtype=np.int64)
        if redirect_bin >= 0:
            where[d == redirect_bin] = 1
            slot[d == redirect_bin] -= starts[redirect_bin]
            slot[d > redirect_bin] -= counts[redirect_bin]
        if self.drop_bin >= 0:
            where[d == self.drop_bin] = 2
        return slot, where, int(starts[-1]), int(counts[redirect_bin]) if redirect_bin >= 0 else 0

    def pack(self, src, dst, redirect_bin, red):
        _lib.call("mgr_pack", ctypes.c_void_p(src.ptr), src.rb, self.n, _lib.ptr(self.dest_t),
                  self.nb, self.drop_bin, self.tile_rows, _lib.ptr(self.ws),
                  ctypes.c_void_p(dst.ptr), redirect_bin,
                  ctypes.c_void_p(red.ptr) if redirect_bin >= 0 else None, _lib.stream_handle())

    def unpack(self, packed, out, redirect_bin, red):
        _lib.call("mgr_unpack", ctypes.c_void_p(packed.ptr), packed.rb, self.n,
                  _lib.ptr(self.dest_t), self.nb, self.drop_bin, self.tile_rows,
                  _lib.ptr(self.ws), ctypes.c_void_p(out.ptr), redirect_bin,
                  ctypes.c_void_p(red.ptr) if redirect_bin >= 0 else None, _lib.stream_handle())

    def unpack_fields(self, packed, outs, redirect_bin, reds, t0=0, t1=-1):
        _lib.call("mgr_unpack_fields", len(packed), _vp([p.ptr for p in packed]),
                  _i64([p.rb for p in packed]), self.n, _lib.ptr(self.dest_t), self.nb,
                  self.drop_bin, self.tile_rows, _lib.ptr(self.ws), _vp([o.ptr for o in outs]),
                  redirect_bin, _vp([r.ptr for r in reds]) if redirect_bin >= 0 else None,
                  t0, t1, _lib.stream_handle())


def _ids(rng, n, nb, drop, empty_bin=None, one_bin=None):
    P = nb - 1 if drop else nb
    if one_bin is not None:
        return np.full(n, one_bin, dtype=np.int64)
    ids = rng.integers(-1 if drop else 0, P + (1 if drop else 0), n)   # drop: -1 and P are out of range
    if empty_bin is not None and P > 1:
        ids[ids == empty_bin] = (empty_bin + 1) % P
    return ids


def _redirect(which, nb, drop):
    P = nb - 1 if drop else nb
    return {"none": -1, "first": 0, "mid": P // 2, "last": P - 1}[which]


def _check_case(n, nb, rb, redirect="none", drop=False, hook=0, shift=0, empty_bin=None,
                one_bin=None, tile_rows=None, seed=0):
    rng = np.random.default_rng(1000 * n + 10 * nb + rb + seed)
    sc = Scanned(_ids(rng, n, nb, drop, empty_bin, one_bin), nb, drop, tile_rows, hint_rb=rb)
    rbin = _redirect(redirect, nb, drop)
    slot, where, n_all, n_red = sc.model(rbin)
    n_dst = n_all - n_red               # dst keeps the drop bin's (unwritten) tail rows
    x = rng.integers(0, 256, (n, rb), dtype=np.uint8)
    src = Buf(n, rb, content=x)
    dst, red = Buf(n_dst, rb, shift), Buf(n_red, rb, shift)
    _lib.test_hook("unpack_kernel", hook)
    # 1) the pack against the model (the drop bin's rows, last in dst, stay unwritten)
    sc.pack(src, dst, rbin, red)
    want_dst = np.full((n_dst, rb), FILL, dtype=np.uint8)
    want_red = np.full((n_red, rb), FILL, dtype=np.uint8)
    want_dst[slot[where == 0]] = x[where == 0]
    want_red[slot[where == 1]] = x[where == 1]
    assert np.array_equal(dst.get(), want_dst), "pack: dst"
    assert np.array_equal(red.get(), want_red), "pack: redirect_dst"
    # 2) unpack(pack(x)) == x, dropped rows zero, over a pre-filled out
    out = Buf(n, rb, shift)
    sc.unpack(dst, out, rbin, red)
    want = x.copy()
    want[where == 2] = 0
    got = out.get()
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError(f"unpack: {bad.size} rows differ, first row {bad[0]} "
                             f"(bin {sc.dest[bad[0]]}, slot {slot[bad[0]]})")
    # 3) a buffer that holds its own slot indexes gives the inverse permutation
    #    (8-byte rows on the same dest: another row size than the pack moved)
    idx_dst = Buf(n_dst, 8, content=np.arange(n_dst, dtype=np.int64))
    idx_red = Buf(n_red, 8, content=np.arange(n_red, dtype=np.int64) | (1 << 40))
    out8 = Buf(n, 8)
    sc.unpack(idx_dst, out8, rbin, idx_red)
    inv = np.where(where == 1, slot | (1 << 40), slot)
    inv[where == 2] = 0
    assert np.array_equal(out8.get().view(np.int64).reshape(-1), inv), "inverse permutation"
    if drop and n >= 64:
        assert (where == 2).any()       # the drop bin really holds rows


# ---------------------------------------------------------------- the cases
# (n, bins, row bytes, redirect, drop): every n, every bin count, every row
# size and every redirect position at least once, sparsely combined
CASES = [
    (0, 8, 32, "none", False), (1, 8, 32, "first", False), (63, 2, 8, "last", False),
    (64, 8, 16, "mid", True), (65, 27, 12, "none", False), (511, 64, 4, "mid", False),
    (512, 8, 24, "first", True), (513, 27, 36, "last", True), (1025, 64, 64, "none", True),
    (3 * 512 + 17, 8, 32, "mid", False), (20011, 27, 36, "first", False),
    (20011, 8, 32, "last", True), (1025, 1, 16, "none", False), (513, 1, 8, "first", False),
    (3 * 512 + 17, 2, 1, "none", True), (1025, 8, 2, "mid", False), (513, 27, 3, "last", True),
    (1025, 8, 68, "first", True), (513, 8, 260, "mid", True), (65, 2, 260, "none", False),
    (20011, 65, 32, "mid", True), (3 * 512 + 17, 125, 12, "first", False),
    (20011, 300, 8, "last", True), (1025, 300, 36, "none", False), (511, 65, 3, "mid", True),
    (20011, 64, 64, "last", False), (1, 300, 4, "none", True),
]


@pytest.mark.parametrize("n,nb,rb,redirect,drop", CASES,
                         ids=[f"n{c[0]}-b{c[1]}-r{c[2]}-{c[3]}{'-drop' if c[4] else ''}"
                              for c in CASES])
def test_unpack_matrix(n, nb, rb, redirect, drop):
    _check_case(n, nb, rb, redirect, drop)


GENERIC = [(513, 8, 32, "mid", True), (20011, 27, 36, "first", False), (1025, 64, 16, "last", True),
           (65, 2, 8, "none", False), (3 * 512 + 17, 8, 64, "first", True)]


@pytest.mark.parametrize("n,nb,rb,redirect,drop", GENERIC)
def test_unpack_generic_kernel_on_cooperative_shapes(n, nb, rb, redirect, drop):
    """Hook unpack_kernel 1: unpack_kernel<W, u8> where the product runs the
    cooperative kernel."""
    _check_case(n, nb, rb, redirect, drop, hook=1)


@pytest.mark.parametrize("rb,shift", [(16, 8), (16, 4), (32, 4), (24, 4), (16, 2), (8, 1)])
def test_unpack_misaligned_buffers(rb, shift):
    """packed, redirect_src and out ``shift`` bytes off 16-byte alignment: the
    unit narrows (16 -> 8 -> 4: still cooperative; 2, 1: the generic kernel)."""
    _check_case(3 * 512 + 17, 8, rb, "mid", True, shift=shift)


def test_unpack_empty_bin_and_single_bin():
    _check_case(1025, 8, 32, "mid", False, empty_bin=3)           # redirect bin 4; bin 3 holds no rows
    _check_case(1025, 8, 32, "mid", False, empty_bin=4)           # the redirect bin itself is empty
    _check_case(1025, 8, 32, "mid", False, one_bin=4)             # every row in the redirect bin
    _check_case(1025, 8, 32, "first", False, one_bin=5)           # every row in one travelling bin
    _check_case(513, 65, 12, "none", True, one_bin=64)            # every row dropped


@pytest.mark.parametrize("tile_rows", [64, 256, 1024, 2048])
def test_unpack_tile_sizes(tile_rows):
    """Other tile sizes than the policy's (2048 rows: above the cooperative
    kernel's 16 rounds, the generic kernel takes it)."""
    _check_case(20011, 8, 32, "mid", True, tile_rows=tile_rows)


# -------------------------------------------------------------- tile ranges
@pytest.mark.parametrize("hook", [0, 1])
def test_unpack_tile_ranges(hook):
    n, nb, rb = 3 * 512 + 17, 8, 32
    rng = np.random.default_rng(77)
    sc = Scanned(_ids(rng, n, nb, True), nb, True, hint_rb=rb)
    assert sc.tile_rows == 512 and sc.T == 4
    rbin = 3
    slot, where, n_all, n_red = sc.model(rbin)
    x = rng.integers(0, 256, (n, rb), dtype=np.uint8)
    src, dst, red = Buf(n, rb, content=x), Buf(n_all - n_red, rb), Buf(n_red, rb)
    sc.pack(src, dst, rbin, red)
    want = x.copy()
    want[where == 2] = 0
    _lib.test_hook("unpack_kernel", hook)
    out = Buf(n, rb)
    for t0, t1 in ((3, 4), (0, 1), (1, 3)):                 # any order
        sc.unpack_fields([dst], [out], rbin, [red], t0, t1)
    assert np.array_equal(out.get(), want)
    out.fill()
    sc.unpack_fields([dst], [out], rbin, [red], 1, 3)       # tiles 1, 2 only
    got = out.get()
    assert np.array_equal(got[512:1536], want[512:1536])
    assert (got[:512] == FILL).all() and (got[1536:] == FILL).all()
    out.fill()
    sc.unpack_fields([dst], [out], rbin, [red], 2, 2)       # empty range
    assert (out.get() == FILL).all()


# ------------------------------------------------------------------- fields
FIELD_SETS = {"cfg5": (12, 12, 4, 8), "24-8": (24, 8), "32": (32,), "4-2-36": (4, 2, 36),
              "six": (8, 4, 12, 16, 2, 32)}


@pytest.mark.parametrize("hook", [0, 1, 2])
@pytest.mark.parametrize("name", list(FIELD_SETS))
def test_unpack_fields_against_single_field_unpack(name, hook):
    """mgr_unpack_fields == mgr_unpack field by field (itself checked against
    numpy above and here), with a redirect bin, a drop bin and every kernel:
    0 the multi-field launch where the set has a signature, 2 the single-field
    cooperative kernel per field, 1 the generic kernel."""
    rbs = FIELD_SETS[name]
    n, nb = 3 * 1024 + 17, 9
    rng = np.random.default_rng(len(name) + 31 * hook)
    sc = Scanned(_ids(rng, n, nb, True), nb, True, hint_rb=32)
    rbin = 2
    slot, where, n_all, n_red = sc.model(rbin)
    xs = [rng.integers(0, 256, (n, rb), dtype=np.uint8) for rb in rbs]
    packed, reds = [], []
    for x, rb in zip(xs, rbs):          # the model's pack as the packed content
        d = np.full((n_all - n_red, rb), FILL, dtype=np.uint8)
        r = np.full((n_red, rb), FILL, dtype=np.uint8)
        d[slot[where == 0]] = x[where == 0]
        r[slot[where == 1]] = x[where == 1]
        packed.append(Buf(n_all - n_red, rb, content=d))
        reds.append(Buf(n_red, rb, content=r))
    _lib.test_hook("unpack_kernel", hook)
    outs = [Buf(n, rb) for rb in rbs]
    sc.unpack_fields(packed, outs, rbin, reds)
    _lib.test_hook("unpack_kernel", 0)
    for f, (x, rb) in enumerate(zip(xs, rbs)):
        want = x.copy()
        want[where == 2] = 0
        assert np.array_equal(outs[f].get(), want), (name, f)
        one = Buf(n, rb)
        sc.unpack(packed[f], one, rbin, reds[f])
        assert np.array_equal(one.get(), outs[f].get()), (name, f)


# ------------------------------------------------------------- scan failure
def test_unpack_after_failed_scan_writes_nothing():
    """A failed scan (forced deterministically: scan chunk 0 publishes its
    prefix poisoned, hook scan_poison_chunk) makes the unpack write nothing,
    like every pack: out keeps its fill."""
    from mpi_grid_redistribute_amd import GridPartitioner
    n = 300_000
    rng = np.random.default_rng(9)
    P = GridPartitioner([2, 2, 2], [1.0] * 3)
    pos = torch.from_numpy(rng.uniform(0, 1, (n, 3))).cuda()
    data = torch.from_numpy(rng.integers(0, 256, n * 32, dtype=np.uint8)).cuda()
    _lib.test_hook("scan_poison_chunk", 0)
    try:
        _, counts = P.partition_device(data, 32, pos.clone())
        c = counts.cpu().numpy()
        for hook in (0, 1):
            _lib.test_hook("unpack_kernel", hook)
            out = P.unpartition_device(data, 32)
            out.fill_(FILL)
            out2 = P.unpartition_device(data, 32)
            assert out2.data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            assert bool((out2 == FILL).all()), "an unpack wrote after a failed scan"
    finally:
        _lib.test_hook("scan_poison_chunk", _lib.HOOK_DEFAULTS["scan_poison_chunk"])
        _lib.test_hook("unpack_kernel", 0)
    assert (c == -1).all(), c


# ---------------------------------------------------------- GridPartitioner
def _inverse_of_partition(P, pos_np):
    """numpy: the stable partition's order for these positions (cells by the
    package's own binning entry point are checked elsewhere; here only the
    permutation matters, so it is taken from the destination bytes)."""
    key = P._last_part
    dest = P._cache[key][2].cpu().numpy()[:len(pos_np)].astype(np.int64)
    return np.argsort(dest, kind="stable")


@pytest.mark.parametrize("topo,rb", [([2, 2, 2], 32), ([4, 4, 4], 36)])
def test_partitioner_round_trip(topo, rb):
    from mpi_grid_redistribute_amd import GridPartitioner
    n = 300_000
    rng = np.random.default_rng(rb)
    P = GridPartitioner(topo, [1.0] * 3)
    with pytest.raises(RuntimeError):
        P.unpartition_device(torch.zeros(rb, dtype=torch.uint8, device="cuda"), rb)
    pos_np = rng.uniform(-0.5, 1.5, (n, 3))
    x = rng.integers(0, 256, (n, rb), dtype=np.uint8)
    data = torch.from_numpy(x.reshape(-1)).cuda()
    out, counts = P.partition_device(data, rb, torch.from_numpy(pos_np).cuda())
    order = _inverse_of_partition(P, pos_np)
    packed = out.cpu().numpy().reshape(n, rb)
    assert np.array_equal(packed, x[order])                       # the pack, by numpy
    back = P.unpartition_device(out, rb)
    assert np.array_equal(back.cpu().numpy().reshape(n, rb), x)   # the round trip
    # results of another row size along the same route: out[order] = packed rows
    vals = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    got = P.unpartition_device(torch.from_numpy(vals.reshape(-1)).cuda(), 8)
    want = np.empty_like(vals)
    want[order] = vals
    assert np.array_equal(got.cpu().numpy().reshape(n, 8), want)
    with pytest.raises(ValueError):
        P.unpartition_device(out[:-rb], rb)


def test_partitioner_fields_round_trip_cfg5():
    """Config 5's four arrays (pos f32 x3, vel f32 x3, mass f32, id i64)."""
    from mpi_grid_redistribute_amd import GridPartitioner
    n = 300_000
    rng = np.random.default_rng(55)
    P = GridPartitioner([2, 2, 2], [1.0] * 3)
    pos = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    fields = [pos, rng.normal(size=(n, 3)).astype(np.float32),
              rng.uniform(1, 2, (n, 1)).astype(np.float32),
              np.arange(n, dtype=np.int64).reshape(n, 1)]
    rbs = [12, 12, 4, 8]
    ts = [torch.from_numpy(f).cuda() for f in fields]
    flats = [t.reshape(-1).view(torch.uint8) for t in ts]
    outs, counts = P.partition_fields_device(flats, rbs, ts[0])
    order = _inverse_of_partition(P, pos)
    for f, o, rb in zip(fields, outs, rbs):
        raw = np.ascontiguousarray(f).view(np.uint8).reshape(n, rb)
        assert np.array_equal(o.cpu().numpy().reshape(n, rb), raw[order])
    back = P.unpartition_fields_device(outs, rbs)
    for f, b, rb in zip(fields, back, rbs):
        raw = np.ascontiguousarray(f).view(np.uint8).reshape(n, rb)
        assert np.array_equal(b.cpu().numpy().reshape(n, rb), raw)
