"""Host checks of the packs' C ABI (mgr_pack, mgr_pack_ids, mgr_pack_tiles,
mgr_pack_fields, mgr_msel_pack_fields, mgr_msel_pack_placed): the symbols are
exported, their ctypes signatures are the header's, and every argument error
is refused on the host, before any launch, with the return code and message
recorded in tests/golden/capi_pack_errors.json (tests/golden/make_capi_pack_errors.py).

Every case changes one argument of a valid call (5 rows in one 512-row tile,
4 bins; two fields; two selection sets).  No case reaches a launch: each is
refused, or covers no tile, or has no rows."""
import ctypes
import json
import os

import pytest

from tests.test_capi_unpack import header_signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_pack_errors.json")
MGR_OK, MGR_EINVAL = 0, -1
MAX_BINS, MAX_FIELDS, MSEL_MAX_FIELDS, MAX_SETS, MAX_TILE_ROWS = 4096, 16, 18, 32, 65536
ENTRIES = ["mgr_pack", "mgr_pack_ids", "mgr_pack_tiles", "mgr_pack_fields",
           "mgr_msel_pack_fields", "mgr_msel_pack_placed"]
V = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", ENTRIES)
def test_exported_with_the_headers_signature(lib, name):
    from mpi_grid_redistribute_amd import _lib
    assert hasattr(lib, name)
    res, args = _lib.SIGNATURES[name]
    assert (res, args) == header_signature(name)
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args


_BUF = ctypes.create_string_buffer(256)
P = ctypes.cast(_BUF, V).value


def _ptrs(v):
    return None if v is None else (V * max(len(v), 1))(*v)


def _i64s(v):
    return None if v is None else (ctypes.c_int64 * max(len(v), 1))(*v)


def _pack(lib, name, src=P, rb=8, n=5, dest=P, nbins=4, drop=-1, tile=512, ws=P, dst=P, red=-1,
          red_dst=None, ids_src=P, ids_dst=P, ids_red=None, t0=0, t1=1):
    head = (src, rb, n, dest, nbins, drop, tile, ws, dst, red, red_dst)
    if name == "mgr_pack":
        return lib.mgr_pack(*head, None)
    if name == "mgr_pack_ids":
        return lib.mgr_pack_ids(*head, ids_src, ids_dst, ids_red, None)
    return lib.mgr_pack_tiles(*head, ids_src, ids_dst, ids_red, t0, t1, None)


def _pack_fields(lib, nf=2, srcs=(P, P), rbs=(8, 4), n=5, dest=P, nbins=4, drop=-1, tile=512, ws=P,
                 dsts=(P, P), red=-1, reds=None, ids_src=None, ids_dst=None, ids_red=None, t0=0,
                 t1=1):
    return lib.mgr_pack_fields(nf, _ptrs(srcs), _i64s(rbs), n, dest, nbins, drop, tile, ws,
                               _ptrs(dsts), red, _ptrs(reds), ids_src, ids_dst, ids_red, t0, t1,
                               None)


def _msel(lib, name, nf=2, srcs=(P, P), rbs=(8, 4), n=5, flags=P, nsets=2, masks=(1, 2), tile=512,
          ws=P, dsts=(P, P, P, P), cap=10):
    mk = None if masks is None else (ctypes.c_int * max(len(masks), 1))(*masks)
    head = (nf, _ptrs(srcs), _i64s(rbs), n, flags, nsets, mk, tile, ws, _ptrs(dsts))
    if name == "mgr_msel_pack_fields":
        return lib.mgr_msel_pack_fields(*head, None)
    return lib.mgr_msel_pack_placed(*head, cap, None)


TILES = {"tile_rows 0": 0, "tile_rows 63": 63, "tile_rows 65": 65,
         "tile_rows above the maximum": MAX_TILE_ROWS + 64}
# 5 rows of 512-row tiles are one tile
BAD_RANGES = {"tiles: negative begin": (-1, 1), "tiles: end before begin": (1, 0),
              "tiles: end beyond T": (0, 2), "tiles: begin and end beyond T": (2, 2)}
EMPTY_RANGES = {"tiles: empty at 0": (0, 0), "tiles: empty at T": (1, 1)}


def cases():
    """{entry: {case: keyword arguments of the entry's caller above}}; every
    case but those named "ok: ..." is an argument error."""
    out = {}
    for name in ("mgr_pack", "mgr_pack_ids", "mgr_pack_tiles"):
        c = {"null src": dict(src=None), "null dest": dict(dest=None),
             "null workspace": dict(ws=None), "row_bytes 0": dict(rb=0),
             "nbins 0": dict(nbins=0), "nbins above the maximum": dict(nbins=MAX_BINS + 1),
             "redirect without a buffer": dict(red=2, red_dst=None),
             "redirect_bin == nbins": dict(red=4, red_dst=P, ids_red=P),
             "redirect_bin > nbins": dict(red=7, red_dst=P, ids_red=P),
             # doubly wrong: the order of the checks decides the message
             "tile_rows 0 and row_bytes 0": dict(tile=0, rb=0),
             "row_bytes 0 and nbins 0": dict(rb=0, nbins=0),
             "nbins 0 and null src": dict(nbins=0, src=None),
             "null src and redirect without a buffer": dict(src=None, red=2),
             "redirect without a buffer and out of range": dict(red=4, red_dst=None),
             "ok: no rows, no pointers": dict(n=0, src=None, dest=None, ws=None, dst=None,
                                              ids_src=None, ids_dst=None, t0=0, t1=0)}
        c.update({k: dict(tile=v) for k, v in TILES.items()})
        if name != "mgr_pack":
            c["redirect without an ids buffer"] = dict(red=2, red_dst=P, ids_red=None)
        if name == "mgr_pack_ids":
            c["null ids_src"] = dict(ids_src=None)
        if name == "mgr_pack_tiles":
            c.update({k: dict(t0=a, t1=b) for k, (a, b) in BAD_RANGES.items()})
            c.update({"ok: " + k: dict(t0=a, t1=b) for k, (a, b) in EMPTY_RANGES.items()})
            c["tiles: end -1"] = dict(t0=0, t1=-1)
            c["tiles: end -1, no rows"] = dict(n=0, t0=0, t1=-1)
            c["tiles: a range of no rows"] = dict(n=0, t0=0, t1=1)
            c["tiles: bad range and redirect out of range"] = dict(t0=0, t1=2, red=4, red_dst=P,
                                                                   ids_red=P)
        out[name] = c

    many = (P,) * (MAX_FIELDS + 1)
    c = {"nfields 0": dict(nf=0),
         "nfields above the maximum": dict(nf=MAX_FIELDS + 1, srcs=many, rbs=(8,) * len(many),
                                           dsts=many),
         "null srcs": dict(srcs=None), "null row_bytes": dict(rbs=None), "null dsts": dict(dsts=None),
         "null srcs[1]": dict(srcs=(P, None)), "null dest": dict(dest=None),
         "null workspace": dict(ws=None), "row_bytes 0": dict(rbs=(8, 0)),
         "nbins 0": dict(nbins=0), "nbins above the maximum": dict(nbins=MAX_BINS + 1),
         "redirect without buffers": dict(red=2, reds=None),
         "redirect without a buffer for field 1": dict(red=2, reds=(P, None)),
         "redirect without an ids buffer": dict(red=2, reds=(P, P), ids_src=P, ids_dst=P),
         "ids without an output": dict(ids_src=P, ids_dst=None),
         "redirect_bin == nbins": dict(red=4, reds=(P, P)),
         "redirect_bin > nbins": dict(red=7, reds=(P, P)),
         "tile_rows 0 and nfields 0": dict(tile=0, nf=0),
         "nfields 0 and null srcs": dict(nf=0, srcs=None),
         "nbins 0 and row_bytes 0": dict(nbins=0, rbs=(0, 4)),
         "redirect out of range and null srcs[0]": dict(red=4, reds=(P, P), srcs=(None, P)),
         "null srcs[0] and null dest": dict(srcs=(None, P), dest=None),
         "null dest and bad range": dict(dest=None, t0=0, t1=2),
         "ok: tiles: end -1, no rows": dict(n=0, dest=None, ws=None, srcs=(None, None),
                                           dsts=(None, None), t0=0, t1=-1),
         "tiles: a range of no rows": dict(n=0, t0=0, t1=1)}
    c.update({k: dict(tile=v) for k, v in TILES.items()})
    c.update({k: dict(t0=a, t1=b) for k, (a, b) in BAD_RANGES.items()})
    c.update({"ok: " + k: dict(t0=a, t1=b) for k, (a, b) in EMPTY_RANGES.items()})
    out["mgr_pack_fields"] = c

    for name in ("mgr_msel_pack_fields", "mgr_msel_pack_placed"):
        many = (P,) * (MSEL_MAX_FIELDS + 1)
        c = {"nfields 0": dict(nf=0),
             "nfields above the maximum": dict(nf=len(many), srcs=many, rbs=(8,) * len(many),
                                               dsts=many * 2),
             "null srcs": dict(srcs=None), "null row_bytes": dict(rbs=None),
             "null dsts": dict(dsts=None), "null srcs[1]": dict(srcs=(P, None)),
             "null flags": dict(flags=None), "null workspace": dict(ws=None),
             "null masks": dict(masks=None), "row_bytes 0": dict(rbs=(8, 0)),
             "nsets 0": dict(nsets=0), "nsets above the maximum": dict(nsets=MAX_SETS + 1),
             "flag mask 0": dict(masks=(1, 0)), "flag mask above 16 bits": dict(masks=(1 << 16, 2)),
             "tile_rows 0 and nsets 0": dict(tile=0, nsets=0),
             "nsets 0 and nfields 0": dict(nsets=0, nf=0),
             "nfields 0 and row_bytes 0": dict(nf=0, rbs=(0, 4)),
             "row_bytes 0 and null flags": dict(rbs=(0, 4), flags=None),
             "ok: no rows, no pointers": dict(n=0, flags=None, ws=None, dsts=None,
                                              srcs=(None, None))}
        c.update({k: dict(tile=v) for k, v in TILES.items()})
        if name == "mgr_msel_pack_placed":
            c["cap_rows -1"] = dict(cap=-1)
            c["null dsts[1]"] = dict(dsts=(P, None))
            c["nfields 0 and cap_rows -1"] = dict(nf=0, cap=-1)
            c["cap_rows -1 and row_bytes 0"] = dict(cap=-1, rbs=(0, 4))
            c["ok: cap_rows 0, null dsts[1]"] = dict(cap=0, dsts=(P, None))
        out[name] = c
    return out


def run(lib, entry, kw):
    """(return code, message) of one case; the message of a refused call only."""
    if entry == "mgr_pack_fields":
        rc = _pack_fields(lib, **kw)
    elif entry.startswith("mgr_msel"):
        rc = _msel(lib, entry, **kw)
    else:
        rc = _pack(lib, entry, **kw)
    return [rc, lib.mgr_last_error().decode() if rc else ""]


def record(lib):
    return {entry: {case: run(lib, entry, kw) for case, kw in cs.items()}
            for entry, cs in cases().items()}


@pytest.fixture(scope="module")
def expected():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_the_table_covers_every_case(expected):
    assert {e: sorted(c) for e, c in expected.items()} == {e: sorted(c) for e, c in cases().items()}
    assert sorted(expected) == sorted(ENTRIES)


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_are_refused_before_any_launch(lib, expected, entry):
    for case, kw in cases()[entry].items():
        got = run(lib, entry, kw)
        assert got == expected[entry][case], (entry, case)
        # nothing but a refusal or a call that has nothing to launch
        assert got[0] == (MGR_OK if case.startswith("ok: ") else MGR_EINVAL), (entry, case)
        assert got[0] == MGR_OK or got[1], (entry, case)
