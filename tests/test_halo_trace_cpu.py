"""The call sequence of ``halo.exchange_overload`` on the CPU, pinned to a
recording (tests/golden/halo_trace.json, made by tests/golden/make_halo_trace.py
on the commit before halo.py was split): per rank and in order, every
point-to-point group as (kind, peer, bytes), every scratch buffer by name and
size, every selection as (rows, masks, tag), every pack with the selection it
reads, its sources, its row bytes, its accounted rows and per field and set
the size of the destination (null: not written), and every host read.  What
the outputs of tests/test_halo_cpu.py cannot see -- message order, staging
layout, which pass packs which sets, the number of host syncs -- is equal or
the test fails.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from mpi_grid_redistribute_amd.comm import MpiHostComm, SelfComm
from mpi_grid_redistribute_amd.halo import exchange_overload, thresholds
from tests import golden_io as G
from tests.fake_mpi import run_ranks
from tests.test_halo_cpu import _POS_NP, CpuSelect, GeoRank, _flat, local_inputs
from tests.test_soa_halo_cpu import _row_bytes, _soa_inputs

FIXTURE = os.path.join(G.GOLDEN, "halo_trace.json")
GENERAL = ["halo_p8_f64_rec32.npz", "halo_p6_321_i32.npz", "halo_direct_p6_321_nonperiodic.npz",
           "soa_halo_p6_321.npz"]
# (case, carry_pos, spare rows of the arena or None)
RUNS = [(case, cp, None) for case in GENERAL for cp in (True, False)] \
    + [("halo_p1_self.npz", cp, spare) for cp in (True, False) for spare in (None, 3, 10**6)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(fixture, per rank (payload array or list of field arrays, positions),
    periodic): the local rows the halo step starts from."""
    f = G.load(case)
    if case.startswith("soa_"):
        per_rank, periodic = _soa_inputs(f, case)
        return f, [(fields, p) for fields, p, _ in per_rank], periodic
    data, pos, periodic = local_inputs(f, case)
    return f, list(zip(data, pos)), periodic


def exchange(f, r, transport, sel, payload, p, periodic, carry_pos=True, spare=None, **kw):
    """exchange_overload of rank r.  ``spare``: None = stores of the
    exchange's own, else every field's local rows sit at the head of a store
    with ``spare`` free rows after them (the arena)."""
    multi = isinstance(payload, list)
    fields = payload if multi else [payload]
    R = GeoRank(f["topology"], f["box"], int(f["size"]), r)
    code = {v: k for k, v in _POS_NP.items()}[p.dtype]
    n, ncols = len(p), p.shape[1]
    rbs = [_row_bytes(x) for x in fields]
    flats, p_flat, arena, flags = [_flat(x) for x in fields], _flat(p), None, None
    if not carry_pos:
        flags = CpuSelect().flags(p_flat, n, ncols, code, R.dim,
                                  *thresholds(R, list(f["overload"])))
    if spare is not None:
        st = [torch.zeros((n + spare) * rb, dtype=torch.uint8) for rb in rbs + [_row_bytes(p)]]
        for s, x in zip(st, flats + [p_flat]):
            s[: x.numel()].copy_(x)
        flats, p_flat = [s[: n * rb] for s, rb in zip(st, rbs)], st[-1][: p_flat.numel()]
        arena = (st[:-1] if multi else st[0], st[-1] if carry_pos else None, n, spare)
    return exchange_overload(R, transport, flats if multi else flats[0],
                             rbs if multi else rbs[0], p_flat if carry_pos else None, ncols,
                             code, n, list(f["overload"]), periodic=periodic, sel=sel,
                             arena=arena, flags=flags, **kw)


class TraceComm:
    """Delegates to a transport and logs every p2p group."""

    def __init__(self, inner, log):
        self._inner, self._log = inner, log

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def p2p(self, ops):
        self._log.append(["p2p", [[k, int(peer), t.numel()] for k, peer, t in ops]])
        self._inner.p2p(ops)


class TraceSelect(CpuSelect):
    """CpuSelect logging every call; a pack names its selection by the
    ordinal of the msel call that made the handle."""

    def __init__(self, log):
        self._log, self._handles = log, []

    def _ordinal(self, handle):
        return next(i for i, h in enumerate(self._handles) if h is handle)

    def _buf(self, name, nbytes):
        self._log.append(["buf", name, int(nbytes)])
        return super()._buf(name, nbytes)

    def msel_masks(self, flags, n, masks, tag):
        self._log.append(["msel", int(n), [int(m) for m in masks], tag])
        handle, counts = super().msel_masks(flags, n, masks, tag)
        self._handles.append(handle)
        return handle, counts

    def msel_pack_fields(self, handle, srcs, row_bytes, dsts, rows_out=0):
        self._log.append(["pack_fields", self._ordinal(handle), [t.numel() for t in srcs],
                          [int(rb) for rb in row_bytes], int(rows_out),
                          [[None if t is None else t.numel() for t in row] for row in dsts]])
        super().msel_pack_fields(handle, srcs, row_bytes, dsts, rows_out)

    def msel_pack_placed(self, handle, srcs, row_bytes, dsts, cap_rows):
        self._log.append(["pack_placed", self._ordinal(handle), [t.numel() for t in srcs],
                          [int(rb) for rb in row_bytes], int(cap_rows)])
        super().msel_pack_placed(handle, srcs, row_bytes, dsts, cap_rows)

    def to_host(self, tensors):
        self._log.append(["read", len(tensors)])
        return CpuSelect.to_host(self, tensors)

    def to_host_start(self, tensors):
        self._log.append(["read", len(tensors)])
        return CpuSelect.to_host(self, tensors)


def key(case, carry_pos, spare):
    return f"{case[:-4]} pos={int(carry_pos)} spare={spare}"


def record(case, carry_pos, spare):
    """The per-rank traces of one run, as JSON gives them back."""
    f, per_rank, periodic = inputs(case)
    size = int(f["size"])

    def fn(comm, r):
        log = []
        inner = MpiHostComm(comm) if size > 1 else SelfComm()
        exchange(f, r, TraceComm(inner, log), TraceSelect(log), *per_rank[r], periodic,
                 carry_pos, spare)
        return log

    return json.loads(json.dumps(run_ranks(size, fn)))


@functools.lru_cache(maxsize=None)
def _golden():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case,carry_pos,spare", RUNS, ids=[key(*run) for run in RUNS])
def test_call_sequence(case, carry_pos, spare):
    got, want = record(case, carry_pos, spare), _golden()[key(case, carry_pos, spare)]
    dim = len(G.load(case)["topology"])
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        # 1 + (dim - 1) host syncs on the general path, one on the one-rank path
        assert sum(e[0] == "read" for e in g) == (dim if len(got) > 1 else 1), (case, r)
        for i, (eg, ew) in enumerate(zip(g, w)):
            assert eg == ew, (case, r, i)
        assert len(g) == len(w), (case, r)


def test_fixture_holds_these_runs_only():
    assert sorted(_golden()) == sorted(key(*run) for run in RUNS)
    assert os.path.getsize(FIXTURE) < 1 << 20
