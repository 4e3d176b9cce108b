"""CPU checks of mgr_partition_onepass_fields' host validation (no launch):
every MGR_EINVAL and MGR_EUNSUPPORTED case of include/mgr.h returns a negative
status and a mgr_last_error that names the argument; the onepass_poison_tile
test hook takes its default and refuses a value below -1."""
import ctypes

import numpy as np
import pytest

MGR_EINVAL, MGR_EUNSUPPORTED = -1, -4
F32, F64, I32 = 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from mpi_grid_redistribute_amd import _lib
    return _lib.load()


def _plan(lib, topo, box, fine=None):
    topo = np.array(topo, dtype=np.int64)
    box = np.array(box, dtype=np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = ctypes.c_void_p()
    if fine is None:
        rc = lib.mgr_plan_create(len(topo), vp(topo), vp(box), F64, int(np.prod(topo)),
                                 ctypes.byref(h))
    else:
        fn = np.array(fine, dtype=np.int64)
        rc = lib.mgr_plan_create_fine(len(topo), vp(topo), vp(fn), vp(box), F64, ctypes.byref(h))
    assert rc == 0
    return h


class _Args:
    """A valid config-5 argument set on host memory (never launched: every
    test breaks one argument); 64-byte aligned so that a source can be moved
    off its 16-byte alignment on purpose."""

    def __init__(self, lib, topo=(2, 2, 2), rbs=(12, 12, 4, 8)):
        self.lib = lib
        self.plan = _plan(lib, topo, [1.0] * len(topo))
        self.raw = ctypes.create_string_buffer(4096 + 64)
        self.base = (ctypes.addressof(self.raw) + 63) & ~63
        self.nf = len(rbs)
        self.rbs = list(rbs)
        self.srcs = [self.base + 256 * f for f in range(self.nf)]
        self.outs = [self.base + 2048 + 64 * f for f in range(self.nf)]
        self.kw = dict(plan=self.plan, fine=None, nf=self.nf, srcs="srcs", rbs="rbs", pf=0, off=0,
                       dtype=F32, n=4, periodic=1, outs="outs", fine_out=None, cap=8,
                       counts=self.base + 3072, ws=self.base + 3200)

    def call(self, **over):
        kw = dict(self.kw, **over)
        P = ctypes.c_void_p
        srcs = kw["srcs"]
        if srcs == "srcs":
            srcs = (P * len(self.srcs))(*self.srcs)
        elif isinstance(srcs, list):
            srcs = (P * len(srcs))(*srcs)
        outs = kw["outs"]
        if outs == "outs":
            outs = (P * len(self.outs))(*self.outs)
        elif isinstance(outs, list):
            outs = (P * len(outs))(*outs)
        rbs = kw["rbs"]
        if rbs == "rbs":
            rbs = self.rbs
        if rbs is not None:
            rbs = (ctypes.c_int64 * len(rbs))(*rbs)
        rc = self.lib.mgr_partition_onepass_fields(
            kw["plan"], kw["fine"], kw["nf"], srcs, rbs, kw["pf"], kw["off"], kw["dtype"], kw["n"],
            kw["periodic"], outs, kw["fine_out"], kw["cap"], kw["counts"], kw["ws"], None)
        return rc, self.lib.mgr_last_error()


@pytest.fixture(scope="module")
def args(lib):
    a = _Args(lib)
    yield a
    lib.mgr_plan_destroy(a.plan)


@pytest.mark.parametrize("over, word", [
    (dict(plan=None), b"plan"),
    (dict(srcs=None), b"srcs"),
    (dict(rbs=None), b"row_bytes"),
    (dict(counts=None), b"bin_counts"),
    (dict(nf=0), b"nfields"),
    (dict(nf=17), b"nfields"),
    (dict(pf=-1), b"pos_field"),
    (dict(pf=4), b"pos_field"),
    (dict(n=-1), b"n -1"),
    (dict(cap=-1), b"cap_rows"),
    (dict(outs=None), b"outs"),
])
def test_einval_names_the_argument(args, over, word):
    rc, msg = args.call(**over)
    assert rc == MGR_EINVAL, (over, rc, msg)
    assert word in msg, (over, msg)


def test_einval_null_source_and_output(args):
    srcs = list(args.srcs)
    srcs[2] = None
    rc, msg = args.call(srcs=srcs)
    assert rc == MGR_EINVAL and b"srcs[2]" in msg, msg
    outs = list(args.outs)
    outs[1] = None                                    # not the position field's
    rc, msg = args.call(outs=outs)
    assert rc == MGR_EINVAL and b"outs[1]" in msg, msg
    rc, msg = args.call(ws=None)
    assert rc == MGR_EINVAL and b"workspace" in msg, msg


def test_einval_fine_plan_without_fine_out(lib, args):
    fine = _plan(lib, [2, 2, 2], [1.0] * 3, fine=[8, 8, 8])
    try:
        rc, msg = args.call(fine=fine, fine_out=None)
        assert rc == MGR_EINVAL and b"fine_out" in msg, msg
    finally:
        lib.mgr_plan_destroy(fine)


@pytest.mark.parametrize("over, word", [
    (dict(dtype=I32), b"pos_dtype"),                               # not float32 / float64
    (dict(dtype=0), b"pos_dtype"),
    (dict(rbs=[12, 12, 2, 8]), b"row_bytes"),                      # a 2-byte row
    (dict(rbs=[12, 12, 6, 8]), b"row_bytes"),                      # not a multiple of 4
    (dict(rbs=[12, 68, 4, 8]), b"row_bytes"),                      # a row above 64 bytes
    (dict(rbs=[12, 64, 48, 8]), b"row_bytes"),                     # 132 staged bytes per row
    (dict(off=4), b"pos_offset"),                                  # three f32 do not fit 12 B at 4
    (dict(off=-4), b"pos_offset"),
    (dict(off=2, rbs=[16, 12, 4, 8]), b"pos_offset"),              # unaligned coordinates
    (dict(dtype=F64), b"pos_offset"),                              # three f64 need 24 bytes
])
def test_eunsupported_names_the_argument(args, over, word):
    rc, msg = args.call(**over)
    assert rc == MGR_EUNSUPPORTED, (over, rc, msg)
    assert word in msg, (over, msg)


def test_eunsupported_fields_alignment_and_plans(lib, args):
    nine = dict(nf=9, rbs=[4] * 9, srcs=[args.base + 64 * f for f in range(9)],
                outs=[args.base + 2048 + 16 * f for f in range(9)])
    rc, msg = args.call(**nine)
    assert rc == MGR_EUNSUPPORTED and b"nfields" in msg, msg
    srcs = list(args.srcs)
    srcs[1] += 8                                                   # not 16-byte aligned
    rc, msg = args.call(srcs=srcs)
    assert rc == MGR_EUNSUPPORTED and b"srcs" in msg, msg
    outs = list(args.outs)
    outs[3] += 2                                                   # not 4-byte aligned
    rc, msg = args.call(outs=outs)
    assert rc == MGR_EUNSUPPORTED and b"outs" in msg, msg
    for topo in ([2, 3], [5, 5, 5]):                               # 2-D; 125 bins
        plan = _plan(lib, topo, [1.0] * len(topo))
        try:
            rc, msg = args.call(plan=plan)
            assert rc == MGR_EUNSUPPORTED and b"plan" in msg, (topo, msg)
        finally:
            lib.mgr_plan_destroy(plan)


def test_poison_tile_hook(lib):
    from mpi_grid_redistribute_amd import _lib
    assert _lib.HOOK_DEFAULTS["onepass_poison_tile"] == -1
    _lib.test_hook("onepass_poison_tile", 40)
    _lib.test_hook("onepass_poison_tile", _lib.HOOK_DEFAULTS["onepass_poison_tile"])
    with pytest.raises(_lib.MgrError):
        _lib.test_hook("onepass_poison_tile", -2)
    assert lib.mgr_test_hook(b"onepass_poison_tile", -2) < 0
    assert b"onepass_poison_tile" in lib.mgr_last_error()
