"""SoA payloads in the overload (halo) exchange, on the CPU (no GPU):

* the C ABI's field limit of the multi-selection packs (host-only calls);
* ``halo.exchange_overload`` with LIST payloads -- one entry per field -- on
  threaded ranks, the selections done by the NumPy stand-in of
  tests/test_halo_cpu.py, byte-exact against the reference's own per-field
  outputs (tests/golden/soa_halo_*.npz, make_golden_soa_halo.py), with and
  without an arena and carried positions; the existing halo_direct_*
  fixtures too, their payload columns split into fields;
* the NumPy oracle, run per field, pinned to the new fixtures.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mpi_grid_redistribute_amd import _lib
from mpi_grid_redistribute_amd.comm import MpiHostComm, SelfComm
from mpi_grid_redistribute_amd.halo import exchange_overload, thresholds
from oracle import redist_oracle as ro
from tests import golden_io as G
from tests.fake_mpi import run_ranks
from tests.test_halo_cpu import _POS_NP, CpuSelect, GeoRank, _flat

SOA_HALO = ["soa_halo_p8.npz", "soa_halo_p6_321.npz", "soa_halo_p1_self.npz",
            "soa_halo_p4_2d.npz"]
DIRECT = ["halo_direct_p6_321_nonperiodic.npz", "halo_direct_p8_nonperiodic.npz"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI
def _msel_call(lib, name, nfields, n=0):
    k = max(nfields, 1)
    srcs = (ctypes.c_void_p * k)()
    rbs = (ctypes.c_int64 * k)(*([4] * k))
    masks = (ctypes.c_int * 2)(1, 2)
    args = [nfields, srcs, rbs, n, None, 2, masks, 4096, None, None]
    if name == "mgr_msel_pack_placed":
        args.append(16)
    return getattr(lib, name)(*args, None)


@pytest.mark.parametrize("name", ["mgr_msel_pack_fields", "mgr_msel_pack_placed"])
def test_msel_pack_field_limit(name):
    """1..MGR_MSEL_MAX_FIELDS (= MGR_MAX_FIELDS + 2 = 18) fields: an empty
    call (n = 0) is MGR_OK for 4 and 18 fields, MGR_EINVAL for 0 and 19, the
    message naming the range."""
    lib = _lib.load()
    for nf in (1, 3, 4, 18):
        assert _msel_call(lib, name, nf) == _lib.MGR_OK, nf
    for nf in (0, 19):
        assert _msel_call(lib, name, nf) == -1, nf          # MGR_EINVAL
        assert b"1..18" in lib.mgr_last_error()


def test_field_limits_match_header():
    text = open(os.path.join(ROOT, "include", "mgr.h")).read()
    mx = int(re.search(r"#define MGR_MAX_FIELDS (\d+)", text).group(1))
    assert re.search(r"#define MGR_MSEL_MAX_FIELDS \(MGR_MAX_FIELDS \+ 2\)", text)
    assert _lib.MAX_FIELDS == mx and _lib.MSEL_MAX_FIELDS == mx + 2
    from mpi_grid_redistribute_amd.redistributor import MAX_FIELDS
    assert MAX_FIELDS == mx


# ------------------------------------------- exchange_overload, list payloads
def _soa_inputs(f, case):
    """Per rank: (fields, position, expected overload rows per field)."""
    size = int(f["size"])
    if case.startswith("halo_direct_"):   # the (n, 2) payload's columns as two fields
        return [([np.ascontiguousarray(f[f"r{r}_data"][:, c]) for c in range(2)], f[f"r{r}_pos"],
                 [np.ascontiguousarray(f[f"r{r}_out"][:, c]) for c in range(2)])
                for r in range(size)], False
    nf = int(f["nfields"])
    return [([f[f"r{r}_f{i}_in"] for i in range(nf)], f[f"r{r}_pos"],
             [f[f"r{r}_f{i}_out"] for i in range(nf)]) for r in range(size)], bool(f["periodic"])


def _row_bytes(a):
    return a.dtype.itemsize * int(np.prod(a.shape[1:], dtype=np.int64))


def run_rank_fields(f, inputs, periodic, transport, r, spare, carry_pos):
    """exchange_overload of rank r's fields as a list payload; ``spare``:
    None = stores of the exchange's own, else every field's local rows sit
    at the head of a store with ``spare`` free rows (the arena).  Returns the
    overload rows per field as arrays of the fields' dtypes and shapes."""
    size = int(f["size"])
    fields, p, _ = inputs[r]
    R = GeoRank(f["topology"], f["box"], size, r)
    code = {v: k for k, v in _POS_NP.items()}[p.dtype]
    n = len(p)
    rbs = [_row_bytes(x) for x in fields]
    rbp = _row_bytes(p)
    flats, p_flat, arena = [_flat(x) for x in fields], _flat(p), None
    if spare is not None:
        st = [torch.full(((n + spare) * rb,), 0xA5, dtype=torch.uint8) for rb in rbs]
        st_p = torch.full(((n + spare) * rbp,), 0x5A, dtype=torch.uint8)
        for s, x, rb in zip(st, flats, rbs):
            s[: n * rb].copy_(x)
        st_p[: n * rbp].copy_(p_flat)
        flats, p_flat = [s[: n * rb] for s, rb in zip(st, rbs)], st_p[: n * rbp]
        arena = (st, st_p if carry_pos else None, n, spare)
    flags = None
    if not carry_pos:
        hi, lo = thresholds(R, list(f["overload"]))
        flags = CpuSelect().flags(p_flat, n, p.shape[1], code, R.dim, hi, lo)
        p_flat = None
    ov, ov_p, m, in_arena = exchange_overload(R, transport, flats, rbs, p_flat, p.shape[1], code,
                                              n, list(f["overload"]), periodic=periodic,
                                              sel=CpuSelect(), arena=arena, flags=flags)
    assert isinstance(ov, list) and len(ov) == len(fields)
    assert (ov_p is None) == (not carry_pos)
    if carry_pos:
        assert ov_p.numel() == m * rbp
    if spare is not None:
        assert in_arena == (m <= spare), (m, spare, in_arena)
        for s, x, rb, o in zip(st, fields, rbs, ov):
            assert torch.equal(s[: n * rb], _flat(x)), "the local rows were overwritten"
            if in_arena:   # appended in place, the rest of the store untouched
                assert torch.equal(s[n * rb:(n + m) * rb], o)
                assert (s[(n + m) * rb:] == 0xA5).all()
    return [o.numpy().view(x.dtype).reshape((m,) + x.shape[1:]) for o, x in zip(ov, fields)]


@pytest.mark.parametrize("carry_pos", [True, False])
@pytest.mark.parametrize("spare", [None, 0, 3, 10**6])
@pytest.mark.parametrize("case", SOA_HALO + DIRECT)
def test_threaded_soa_halo(case, spare, carry_pos):
    f = G.load(case)
    size = int(f["size"])
    inputs, periodic = _soa_inputs(f, case)
    outs = run_ranks(size, lambda comm, r: run_rank_fields(
        f, inputs, periodic, MpiHostComm(comm) if size > 1 else SelfComm(), r, spare, carry_pos))
    for r in range(size):
        for i, (got, exp) in enumerate(zip(outs[r], inputs[r][2])):
            assert G.same_bytes(got, exp), (case, r, i)


def test_single_tensor_form_unchanged():
    """One tensor in, one tensor out (not a list of one)."""
    f = G.load("soa_halo_p1_self.npz")
    x, p = f["r0_f0_in"], f["r0_pos"]
    R = GeoRank(f["topology"], f["box"], 1, 0)
    ov, ov_p, m, _ = exchange_overload(R, SelfComm(), _flat(x), _row_bytes(x), _flat(p), 3,
                                       _lib.MGR_F64, len(x), list(f["overload"]), sel=CpuSelect())
    assert isinstance(ov, torch.Tensor)
    assert G.same_bytes(ov.numpy().view(x.dtype), f["r0_f0_out"])


def test_field_count_checked():
    f = G.load("soa_halo_p1_self.npz")
    x, p = f["r0_f0_in"], f["r0_pos"]
    R = GeoRank(f["topology"], f["box"], 1, 0)
    for nf, nrb in ((17, 17), (0, 0), (2, 3)):
        with pytest.raises(ValueError):
            exchange_overload(R, SelfComm(), [_flat(x)] * nf, [8] * nrb, _flat(p), 3, _lib.MGR_F64,
                              len(x), list(f["overload"]), sel=CpuSelect())


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("case", SOA_HALO)
def test_oracle_per_field(case):
    """oracle/redist_oracle.py's exchange_overload_all_ranks, run once per
    field, reproduces the reference's per-field outputs."""
    f = G.load(case)
    size = int(f["size"])
    inputs, periodic = _soa_inputs(f, case)
    pos = [inp[1] for inp in inputs]
    for i in range(int(f["nfields"])):
        got = ro.exchange_overload_all_ranks(f["topology"], f["box"], size,
                                             [inp[0][i] for inp in inputs], pos,
                                             list(f["overload"]), periodic=periodic)
        for r in range(size):
            assert G.same_bytes(got[r], inputs[r][2][i]), (case, i, r)
