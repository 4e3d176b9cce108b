"""mgr_msel_unpack_add (the halo's return path kernel) against a sequential
numpy model in the same dtype, bit for bit.

Setup as the forward path: flags -> mgr_msel_count + mgr_scan -> the add.  The
model: for k ascending, ``idx = nonzero((flags & m_k) == m_k); acc[idx] +=
src[k]``.  Row counts sit on the round (64) and tile (4096) edges; the sets are
1, 2 and 6 single-bit masks, the 26 masks of the one-rank halo and 32 sets;
every element type, ncomp 1 and 3, some sources NULL, three flag densities.
Rows in no live set hold a sentinel and must keep it.
"""
import numpy as np
import pytest
import torch

from mpi_grid_redistribute_amd import _lib
from mpi_grid_redistribute_amd.halo import DeviceSelect, self_halo_pieces

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1]
SETS = {
    "1bit": [1],
    "2bits": [1, 2],
    "6bits": [1 << b for b in range(6)],
    "pieces26": self_halo_pieces(3),
    "sets32": [(1 << (k % 10)) | (1 << ((3 * k + 1) % 10)) for k in range(32)],
}
ELEMS = [(_lib.MGR_ELEM_F32, np.float32), (_lib.MGR_ELEM_F64, np.float64),
         (_lib.MGR_ELEM_I32, np.int32), (_lib.MGR_ELEM_I64, np.int64)]
SENTINEL = 0xA5


def _flags(rng, n, masks, density):
    bits = int(np.bitwise_or.reduce(np.asarray(masks))).bit_length()
    if density == "all":
        return np.full(n, (1 << bits) - 1, dtype=np.uint16)
    if density == "none":
        return np.zeros(n, dtype=np.uint16)
    f = rng.integers(1, 1 << bits, n).astype(np.uint16)
    f[rng.random(n) >= 0.1] = 0
    return f


def _values(rng, shape, dt):
    if np.dtype(dt).kind == "f":
        return rng.uniform(-1.0, 1.0, shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)   # sums wrap


def _live(masks, variant):
    """Which sets get a source: all, or every third one NULL."""
    return [variant == "full" or k % 3 != 1 for k in range(len(masks))]


def _run_case(rng, sel, n, masks, flags, handle, elem, dt, ncomp, live):
    members = [np.nonzero((flags & m) == m)[0] for m in masks]
    srcs = [_values(rng, (len(idx), ncomp), dt) if lv else None
            for idx, lv in zip(members, live)]
    touched = np.zeros(n, dtype=bool)
    for idx, lv in zip(members, live):
        if lv:
            touched[idx] = True
    acc0 = _values(rng, (n, ncomp), dt)
    acc0.view(np.uint8).reshape(n, -1)[~touched] = SENTINEL
    want = acc0.copy()
    with np.errstate(over="ignore"):
        for idx, s in zip(members, srcs):   # k ascending, one add per set, in dt
            if s is not None:
                want[idx] += s
    acc = torch.from_numpy(acc0.copy()).cuda()
    dsrc = [None if s is None
            else torch.from_numpy(s if len(s) else np.zeros((1, ncomp), dt)).cuda() for s in srcs]
    sel.msel_unpack_add(handle, acc.view(-1).view(torch.uint8), elem, ncomp,
                        [None if t is None else t.view(-1).view(torch.uint8) for t in dsrc])
    got = acc.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (n, len(masks), np.dtype(dt).name, ncomp)
    untouched = got.view(np.uint8).reshape(n, -1)[~touched]
    assert (untouched == SENTINEL).all()


@pytest.mark.parametrize("sets", list(SETS))
@pytest.mark.parametrize("n", NS)
def test_against_numpy_model(n, sets):
    masks = SETS[sets]
    rng = np.random.default_rng(1000 * n + len(masks))
    sel = DeviceSelect(torch.device("cuda", torch.cuda.current_device()))
    for density in ("all", "tenth", "none"):
        flags = _flags(rng, n, masks, density)
        ft = torch.from_numpy(flags.view(np.int16)).cuda()
        handle, counts = sel.msel_masks(ft, n, masks, "")
        exp = [int(((flags & m) == m).sum()) for m in masks]
        assert counts.cpu().tolist() == exp
        for i, (elem, dt) in enumerate(ELEMS):
            for ncomp in (1, 3):
                variant = "full" if (i + ncomp) % 2 == 0 or len(masks) == 1 else "nulls"
                _run_case(rng, sel, n, masks, flags, handle, elem, dt, ncomp,
                          _live(masks, variant))


@pytest.mark.parametrize("ncomp", [2, 4, 5, 9])
def test_other_component_counts(ncomp):
    """ncomp 2 and 4 have kernels of their own, larger ones go four at a time."""
    n, masks = 2 * 4096 + 77, SETS["6bits"]
    rng = np.random.default_rng(ncomp)
    sel = DeviceSelect(torch.device("cuda", torch.cuda.current_device()))
    flags = _flags(rng, n, masks, "tenth")
    handle, _ = sel.msel_masks(torch.from_numpy(flags.view(np.int16)).cuda(), n, masks, "")
    for elem, dt in ELEMS[:2]:
        _run_case(rng, sel, n, masks, flags, handle, elem, dt, ncomp, _live(masks, "nulls"))


def test_inverse_of_msel_pack():
    """Pack a field's sets, add them back onto zeros: every row comes back
    once per live set that holds it, at the place the pack gave it."""
    n, masks = 3 * 4096 + 1, SETS["pieces26"]
    rng = np.random.default_rng(5)
    sel = DeviceSelect(torch.device("cuda", torch.cuda.current_device()))
    flags = _flags(rng, n, masks, "tenth")
    handle, counts = sel.msel_masks(torch.from_numpy(flags.view(np.int16)).cuda(), n, masks, "")
    cnt = counts.cpu().numpy()
    src = rng.integers(-1000, 1000, (n, 3)).astype(np.float32)   # sums exact in float32
    st = torch.from_numpy(src).cuda()
    dsts = [torch.zeros(max(int(c), 1) * 12, dtype=torch.uint8, device="cuda") for c in cnt]
    sel.msel_pack(handle, st.view(-1).view(torch.uint8), 12, dsts)
    acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    sel.msel_unpack_add(handle, acc.view(-1).view(torch.uint8), _lib.MGR_ELEM_F32, 3, dsts)
    times = sum(((flags & m) == m).astype(np.float32) for m in masks)
    assert np.array_equal(acc.cpu().numpy(), src * times[:, None])


def test_failed_scan_leaves_acc_untouched():
    """A workspace whose scan error word is set: nothing is written."""
    n, masks = 3 * 4096 + 1, SETS["6bits"]
    rng = np.random.default_rng(6)
    sel = DeviceSelect(torch.device("cuda", torch.cuda.current_device()))
    flags = _flags(rng, n, masks, "all")
    _lib.test_hook("scan_poison_chunk", 0)
    try:
        handle, counts = sel.msel_masks(torch.from_numpy(flags.view(np.int16)).cuda(), n, masks,
                                        "")
        assert (counts.cpu().numpy() == -1).all()
    finally:
        _lib.test_hook("scan_poison_chunk", _lib.HOOK_DEFAULTS["scan_poison_chunk"])
    acc0 = rng.random((n, 3)).astype(np.float32)
    acc = torch.from_numpy(acc0.copy()).cuda()
    srcs = [torch.ones(n * 12, dtype=torch.uint8, device="cuda") for _ in masks]
    sel.msel_unpack_add(handle, acc.view(-1).view(torch.uint8), _lib.MGR_ELEM_F32, 3, srcs)
    assert acc.cpu().numpy().tobytes() == acc0.tobytes()
    # the same workspace scanned clean: the add goes through
    handle, counts = sel.msel_masks(torch.from_numpy(flags.view(np.int16)).cuda(), n, masks, "")
    assert (counts.cpu().numpy() == n).all()
    z = [torch.zeros(n * 12, dtype=torch.uint8, device="cuda") for _ in masks]
    z[0].view(torch.float32).fill_(1.0)
    sel.msel_unpack_add(handle, acc.view(-1).view(torch.uint8), _lib.MGR_ELEM_F32, 3, z)
    assert np.array_equal(acc.cpu().numpy(), acc0 + np.float32(1.0))
