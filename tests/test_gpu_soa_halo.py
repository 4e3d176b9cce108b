"""SoA payloads in the overload (halo) exchange on the GPU.

* The wide multi-selection pack (4..18 fields behind mgr_msel_pack_fields /
  mgr_msel_pack_placed) against NumPy: every byte of every destination
  buffer, sentinel fill included.
* ``exchange_overload_by_position`` with tuple payloads on threaded ranks,
  numpy and torch-GPU containers, byte-exact against the reference's
  per-field outputs (tests/golden/soa_halo_*.npz) and, on larger inputs
  through the two-call route, against the NumPy oracle run once per field.
"""
import numpy as np
import pytest
import torch

from oracle import redist_oracle as ro
from tests import golden_io as G
from tests.fake_mpi import run_ranks

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import MPIGridRedistributor, _lib  # noqa: E402
from mpi_grid_redistribute_amd.halo import DeviceSelect, self_halo_pieces  # noqa: E402
from mpi_grid_redistribute_amd.redistributor import MAX_FIELDS  # noqa: E402

SENTINEL = 0xAB
ROW_BYTES = [1, 2, 3, 4, 6, 8, 12, 16, 24, 36, 100, 200]
ROWS = [1, 63, 1025, 4097, 3 * 4096 + 17]   # a lane, under a wave, chunk edge, tile edge, tiles + tail


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------- kernel vs numpy
def _masks(nsets):
    return {2: [1, 2], 6: [1 << b for b in range(6)], 26: self_halo_pieces(3)}[nsets]


def _fields(nf, n, rng):
    """nf fields of n rows: (rows uint8 [n, rb], byte offset of the field in
    its buffers).  Field 0: 16-byte rows, aligned (16-byte units); field 1:
    200-byte rows at an odd offset (byte units, more than 64 per row: the
    row-by-row copy); the others drawn from ROW_BYTES at mixed offsets, so
    the unit width differs from field to field."""
    rbs = [16, 200] + [int(x) for x in rng.choice(ROW_BYTES, nf - 2)]
    offs = [0, 1] + [int(x) for x in rng.choice([0, 0, 1, 2, 4, 8], nf - 2)]
    return [(rng.integers(0, 256, (n, rb), dtype=np.uint8), off) for rb, off in zip(rbs, offs)]


def _src(rows, off):
    t = torch.zeros(rows.size + off, dtype=torch.uint8, device="cuda")
    t[off:].copy_(torch.from_numpy(rows.reshape(-1)))
    return t[off:]


def _select(flags, masks, tag="_w"):
    sel = DeviceSelect(torch.device("cuda"))
    fl = torch.from_numpy(flags.view(np.int16)).cuda()
    h, cnt = sel.msel_masks(fl, len(flags), masks, tag)
    return sel, h, cnt


def _check_fields(sel, h, fields, sets, rng, dead=()):
    """mgr_msel_pack_fields: the live sets scattered in one buffer per field
    (shuffled order, gaps between them); ``dead`` sets have a null
    destination in field 0 and a real one in the others, which must stay
    untouched (field 0 decides).  Every byte of every buffer is compared."""
    nsets = len(sets)
    gap = 3
    place, o = {}, gap
    for k in rng.permutation(nsets):
        place[int(k)] = o
        o += (0 if k in dead else len(sets[k])) + gap
    bufs, dsts, want = [], [], []
    for f, (rows, off) in enumerate(fields):
        rb = rows.shape[1]
        exp = np.full(off + o * rb + 64, SENTINEL, dtype=np.uint8)
        buf = torch.full((len(exp),), SENTINEL, dtype=torch.uint8, device="cuda")
        d = []
        for k in range(nsets):
            at = off + place[k] * rb
            d.append(None if (k in dead and f == 0) else buf[at:])
            if k not in dead:
                exp[at:at + len(sets[k]) * rb] = rows[sets[k]].reshape(-1)
        bufs.append(buf)
        dsts.append(d)
        want.append(exp)
    sel.msel_pack_fields(h, [_src(r, off) for r, off in fields], [r.shape[1] for r, _ in fields],
                         dsts)
    torch.cuda.synchronize()
    for f, (buf, exp) in enumerate(zip(bufs, want)):
        assert np.array_equal(buf.cpu().numpy(), exp), f"field {f} ({fields[f][0].shape[1]} B)"


def _check_placed(sel, h, fields, sets, cap):
    """mgr_msel_pack_placed: the sets back to back from dsts[f], rows at or
    beyond ``cap`` not written."""
    order = np.concatenate(sets) if len(sets) else np.zeros(0, np.int64)
    total = len(order)
    bufs, want = [], []
    for rows, off in fields:
        rb = rows.shape[1]
        exp = np.full(off + (total + 2) * rb + 64, SENTINEL, dtype=np.uint8)
        exp[off:off + min(cap, total) * rb] = rows[order[:cap]].reshape(-1)
        bufs.append(torch.full((len(exp),), SENTINEL, dtype=torch.uint8, device="cuda"))
        want.append(exp)
    sel.msel_pack_placed(h, [_src(r, off) for r, off in fields], [r.shape[1] for r, _ in fields],
                         [b[off:] for b, (_, off) in zip(bufs, fields)], cap)
    torch.cuda.synchronize()
    for f, (buf, exp) in enumerate(zip(bufs, want)):
        assert np.array_equal(buf.cpu().numpy(), exp), f"field {f} ({fields[f][0].shape[1]} B)"


def _cut(sets):
    """A row cap inside a set in the middle of the output (3 when empty)."""
    sizes = [len(s) for s in sets]
    big = [k for k, s in enumerate(sizes) if s > 1]
    if not big:
        return 3
    k = big[len(big) // 2]
    return sum(sizes[:k]) + sizes[k] // 2


def _random_flags(n, nbits, rng):
    flags = np.zeros(n, dtype=np.uint16)
    for b in range(nbits):
        flags |= (rng.random(n) < 0.3).astype(np.uint16) << b
    return flags


# 18 x 26 and 17 x 26 exceed one launch's destination table: grouped launches
@pytest.mark.parametrize("nf,nsets", [(4, 2), (5, 6), (17, 26), (18, 26), (18, 2), (4, 26),
                                      (17, 6)])
@pytest.mark.parametrize("n", ROWS)
def test_wide_pack_vs_numpy(n, nf, nsets):
    rng = np.random.default_rng(1000 * n + 32 * nf + nsets)
    masks = _masks(nsets)
    flags = _random_flags(n, 6, rng)
    if n == 1:
        flags[:] = 0x3F          # the one row is in every set
    sets = [np.nonzero((flags & m) == m)[0] for m in masks]
    fields = _fields(nf, n, rng)
    sel, h, cnt = _select(flags, masks)
    assert cnt.cpu().tolist() == [len(s) for s in sets]
    dead = set(int(k) for k in rng.permutation(nsets)[: nsets // 3])
    _check_fields(sel, h, fields, sets, rng, dead)
    _check_placed(sel, h, fields, sets, _cut(sets))
    _check_placed(sel, h, fields, sets, sum(len(s) for s in sets) + 5)


@pytest.mark.parametrize("n", [1025, 3 * 4096 + 17])
def test_wide_pack_lists_overflow(n):
    """Every flag bit set with the 26 halo masks: every row is in every set,
    so a chunk lists 26 x 1024 rows -- far beyond the LDS list's capacity --
    and flushes after every second set."""
    rng = np.random.default_rng(n)
    masks = _masks(26)
    flags = np.full(n, 0x3F, dtype=np.uint16)
    sets = [np.arange(n)] * 26
    fields = _fields(4, n, rng)
    sel, h, cnt = _select(flags, masks)
    assert cnt.cpu().tolist() == [n] * 26
    _check_fields(sel, h, fields, sets, rng)
    _check_placed(sel, h, fields, sets, 13 * n + n // 2)


@pytest.mark.parametrize("nf", [1, 3])
def test_wide_kernel_on_few_fields(nf):
    """Test hook msel_wide: the wide kernel on 1..3 fields (which otherwise
    take the three-field kernel), same results."""
    n, rng = 4097, np.random.default_rng(nf)
    masks = _masks(6)
    flags = _random_flags(n, 6, rng)
    sets = [np.nonzero((flags & m) == m)[0] for m in masks]
    fields = _fields(4, n, rng)[:nf]
    sel, h, _ = _select(flags, masks)
    _lib.test_hook("msel_wide", 1)
    try:
        _check_fields(sel, h, fields, sets, rng, {1})
        _check_placed(sel, h, fields, sets, _cut(sets))
    finally:
        _lib.test_hook("msel_wide", _lib.HOOK_DEFAULTS["msel_wide"])


def test_wide_pack_failed_scan_writes_nothing():
    """After a failed scan (forced: scan chunk 0 publishes its prefix
    poisoned) neither form writes a byte in any field."""
    n, rng = 3 * 4096 + 17, np.random.default_rng(3)
    masks = _masks(6)
    flags = _random_flags(n, 6, rng)
    sets = [np.nonzero((flags & m) == m)[0] for m in masks]
    fields = _fields(5, n, rng)
    _lib.test_hook("scan_poison_chunk", 0)
    try:
        sel, h, cnt = _select(flags, masks, "_f")
        c = cnt.cpu().numpy()
    finally:
        _lib.test_hook("scan_poison_chunk", _lib.HOOK_DEFAULTS["scan_poison_chunk"])
    assert (c == -1).all(), c
    total = sum(len(s) for s in sets)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    srcs = [_src(r, off) for r, off in fields]
    rbs = [r.shape[1] for r, _ in fields]
    bufs = [torch.full((off + (total + 2) * rb,), SENTINEL, dtype=torch.uint8, device="cuda")
            for rb, (_, off) in zip(rbs, fields)]
    sel.msel_pack_fields(h, srcs, rbs, [[b[off + int(starts[k]) * rb:] for k in range(6)]
                                        for b, rb, (_, off) in zip(bufs, rbs, fields)])
    sel.msel_pack_placed(h, srcs, rbs, [b[off:] for b, (_, off) in zip(bufs, fields)], total)
    torch.cuda.synchronize()
    for f, b in enumerate(bufs):
        assert bool((b == SENTINEL).all()), f"field {f} written after a failed scan"


# ------------------------------------------------- API, threaded ranks
SOA_HALO = ["soa_halo_p8.npz", "soa_halo_p6_321.npz", "soa_halo_p1_self.npz",
            "soa_halo_p4_2d.npz"]


def _to_torch(x):
    if x.dtype.names:
        x = x.view(np.uint8).reshape(len(x), -1)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("return_positions", [False, True])
@pytest.mark.parametrize("as_torch", [False, True])
@pytest.mark.parametrize("case", SOA_HALO)
def test_soa_halo_golden(case, as_torch, return_positions):
    f = G.load(case)
    size, nf = int(f["size"]), int(f["nfields"])
    topo, box, ol, periodic = f["topology"], f["box"], list(f["overload"]), bool(f["periodic"])
    pos = [f[f"r{r}_pos"] for r in range(size)]
    fields = [[f[f"r{r}_f{i}_in"] for i in range(nf)] for r in range(size)]
    exp_pos = ro.exchange_overload_all_ranks(topo, box, size, pos, pos, ol, periodic=periodic)
    if as_torch:
        fields = [[_to_torch(x) for x in fl] for fl in fields]
        pos = [_to_torch(p) for p in pos]

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, box)
        out = R.exchange_overload_by_position(tuple(fields[r]), pos[r], ol, periodic=periodic,
                                              return_positions=return_positions)
        torch.cuda.synchronize()
        return out

    outs = run_ranks(size, fn)
    for r in range(size):
        got = outs[r]
        if return_positions:
            got, gpos = got
            assert _bytes(gpos) == _bytes(exp_pos[r]), (case, r)
            assert type(gpos) is type(pos[r])
        assert isinstance(got, tuple) and len(got) == nf
        for i in range(nf):
            exp = f[f"r{r}_f{i}_out"]
            assert type(got[i]) is type(fields[r][i])
            if as_torch:
                assert _bytes(got[i]) == _bytes(exp), (case, r, i)
            else:
                assert G.same_bytes(got[i], exp), (case, r, i)


def _payload(nf, n, pos, rng, gid0):
    """nf fields of mixed dtypes and trailing shapes (the first four: config
    5's pos / vel / mass / id)."""
    kinds = [lambda: pos.astype(np.float32), lambda: rng.normal(size=(n, 3)).astype(np.float32),
             lambda: rng.uniform(1, 2, n).astype(np.float32),
             lambda: np.arange(gid0, gid0 + n, dtype=np.int64),
             lambda: rng.integers(0, 256, n).astype(np.uint8),
             lambda: rng.integers(-30000, 30000, (n, 3)).astype(np.int16),
             lambda: rng.normal(size=(n, 2, 2)), lambda: rng.normal(size=(n, 3)),
             lambda: rng.integers(0, 256, (n, 100), dtype=np.uint8),
             lambda: rng.integers(0, 1 << 30, (n, 9)).astype(np.int32)]
    return [kinds[i % len(kinds)]() for i in range(nf)]


@pytest.mark.parametrize("as_torch", [False, True])
@pytest.mark.parametrize("nf", [4, 16])
@pytest.mark.parametrize("topo", [[1, 1, 1], [2, 2, 2], [3, 2, 1], [4, 1]])
def test_soa_two_call_route_vs_oracle(topo, nf, as_torch):
    """redistribute_by_position(fields, pos, return_positions=True), then
    exchange_overload_by_position(fields, local_pos, ol), concatenated per
    field = the oracle's redistribute-with-overload run once per field.  The
    halo of 16 fields packs 18 (+ positions + flags) between ranks; one rank
    with its 26 pieces packs 17, the case split into two launches."""
    size, dim = int(np.prod(topo)), len(topo)
    rng = np.random.default_rng(100 * size + nf)
    box = [1.0, 2.0, 1.5][:dim]
    ol = [0.08, 0.15, 0.1][:dim]
    pos = [rng.uniform(-0.2, 1.2, (int(rng.integers(2000, 5000)), dim)) * np.asarray(box)
           for _ in range(size)]
    fields = [_payload(nf, len(p), p, rng, 1_000_000 * r) for r, p in enumerate(pos)]
    exp = []
    for i in range(nf):
        exp.append(ro.redistribute_by_position_overload_all_ranks(
            topo, box, size, [fl[i] for fl in fields], [p.copy() for p in pos], ol))
    if as_torch:
        fields = [[_to_torch(x) for x in fl] for fl in fields]
        pos = [_to_torch(p) for p in pos]

    def fn(comm, r):
        R = MPIGridRedistributor(comm if size > 1 else None, topo, box)
        if nf < MAX_FIELDS:
            local, lpos = R.redistribute_by_position(tuple(fields[r]), pos[r],
                                                     return_positions=True)
        else:
            # the redistribution moves at most MAX_FIELDS arrays, returned
            # positions included: a full payload's positions (wrapped by the
            # first call) go in a call of their own
            local = R.redistribute_by_position(tuple(fields[r]), pos[r])
            lpos = R.redistribute_by_position(pos[r], pos[r])
        ov = R.exchange_overload_by_position(local, lpos, ol)
        torch.cuda.synchronize()
        cat = torch.cat if as_torch else np.concatenate
        return [cat([a, b]) for a, b in zip(local, ov)]

    outs = run_ranks(size, fn)
    for r in range(size):
        for i in range(nf):
            assert _bytes(outs[r][i]) == _bytes(exp[i][r]), (topo, r, i)


def test_soa_halo_errors():
    R = MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)
    p = np.zeros((10, 3))
    with pytest.raises(ValueError):
        R.exchange_overload_by_position(tuple(np.zeros(10) for _ in range(17)), p, [0.1] * 3)
    with pytest.raises(ValueError):
        R.exchange_overload_by_position((np.zeros(10), np.zeros(9)), p, [0.1] * 3)
    with pytest.raises(ValueError):
        R.exchange_overload_by_position((np.zeros(9), np.zeros(9)), p, [0.1] * 3)
