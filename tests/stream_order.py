"""Stream-ordering harness of the GPU tests (tests/test_gpu_stream_order.py,
tests/test_gpu_graph_replay.py) and their CPU companion
(tests/test_stream_order_cpu.py).  A plain module: no fixtures, no settings.

Every pipeline is a chain of C entries with two fully valid inputs of the same
shapes: a decoy A and the real input B.  The device input buffers start out
holding A.  ``late`` then queues on a side stream ``s`` a delay, device-to-device
copies of B from tensors staged and synchronized beforehand, and an event
``arrived``.  A chain enqueued on ``s`` afterwards must see B; a kernel (the
whole launch, or one helper kernel of it) that went to another stream runs at
once, sees A or what an earlier call left in the workspace, and the result
differs from ``model(B)``.  Nothing but the caller's own inputs is ever swapped,
and both inputs are in contract, so a kernel that reads the decoy stays inside
its buffers.  Workspaces are zero-filled once and then the library's alone, as
between a caller's calls (``Run.clear`` zeroes result buffers only).

Not covered: the stream of the one-pass entries' workspace zeroing (their only
memset).  Zeroing on another stream would run ahead of the delayed kernel and
still precede it; to tell it apart the kernel would have to run on the words of
an earlier call, and it indexes its look-back words by the ticket it finds
there -- a wrong result could not be had without an access out of bounds.

``arrived.query()`` must be false immediately before the call under test (the
inputs really are late) and, for entries documented as free of host syncs,
still false right after it returns (nothing waited for the stream).  Both are
assertions with a message naming the delay, never skips.

Delay: ``torch.cuda._sleep(DELAY_CYCLES)`` with DELAY_CYCLES = 120_000_000.
Event-timed on one MI355X the sleep kernel ran 0.420 ms per 1_000_000 cycles,
2.084 ms per 5_000_000 and 8.327 ms per 20_000_000 (three repeats each, equal
to 0.1 %), so the delay is 50 ms; the longest chain takes well under 1 ms to
enqueue.  5_000_000 cycles (2 ms) proved too short: the two-pass chain's ten
calls had not all returned when the inputs arrived.

Models: tests/pack_model.py, the oracle (oracle/redist_oracle.py), and the numpy
models of tests/test_gpu_ghost_kernels.py, tests/test_gpu_wide_cells.py,
tests/test_gpu_unsort.py and tests/test_gpu_msel_unpack_add.py (imported, or
for the add lifted from its _run_case)."""
import ctypes

import numpy as np
import torch

from mpi_grid_redistribute_amd import _lib
from oracle import redist_oracle as ro
from tests.pack_model import pack_model
from tests.test_gpu_ghost_kernels import _ids_model, _shift_model
from tests.test_gpu_unsort import _inv
from tests.test_gpu_wide_cells import _model_ids, _offsets

DELAY_CYCLES = 120_000_000
DELAY_NOTE = "torch.cuda._sleep(120_000_000), about 50 ms"

F64, F32, I32 = _lib.MGR_F64, _lib.MGR_F32, _lib.MGR_I32
TOPO, BOX = [2, 2, 2], [1.0, 1.0, 1.0]
SEEDS = {"A": 1, "B": 2}


# ------------------------------------------------------------------ helpers
def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else int(t.data_ptr()) for t in ts])


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _bytes(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)


def _dev(a):
    """The bytes of a numpy array on the device, 16 spare zero bytes behind
    them (the multi-field kernels stage sources in 16-byte units)."""
    raw = _bytes(a)
    t = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    t[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t


def _zeros(nbytes):
    return torch.zeros(int(nbytes) + 16, dtype=torch.uint8, device="cuda")


def _host(t, dtype, shape):
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    return t[:nbytes].cpu().numpy().view(dtype).reshape(shape)


def _plan(topo=TOPO, box=BOX, fine=None):
    t = np.asarray(topo, dtype=np.int64)
    b = np.asarray(box, dtype=np.float64)
    h = ctypes.c_void_p()
    if fine is None:
        _lib.call("mgr_plan_create", len(t), _vp(t), _vp(b), F64, int(np.prod(t)), ctypes.byref(h))
    else:
        f = np.asarray(fine, dtype=np.int64)
        _lib.call("mgr_plan_create_fine", len(t), _vp(t), _vp(f), _vp(b), F64, ctypes.byref(h))
    return h


def _tile_rows(rb, nb):
    return int(_lib.load().mgr_tile_rows(int(rb), int(nb)))


def _ranked_rows(rb, nb):
    return int(_lib.load().mgr_ranked_tile_rows(int(rb), int(nb)))


def _geo():
    return ro.Geometry(TOPO, BOX, 8)


def _payload(rng, n, rb):
    return rng.integers(0, 256, (n, rb), dtype=np.uint8)


# ------------------------------------------------------------ the harness
def deferred(run, s):
    """The C calls of a pipeline's chain on ``s`` as a list of (name, args),
    not yet made: two chains can then be enqueued call by call in turns."""
    calls = []
    run.enqueue(s, call=lambda name, *args: calls.append((name, args)))
    return calls


def late_copies(s, bufs, staged, sync=True):
    """On ``s``: the delay, device-to-device copies staged[i] -> bufs[i], and
    the event that follows them (returned)."""
    if sync:
        torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(DELAY_CYCLES)
        for b, t in zip(bufs, staged):
            b.copy_(t, non_blocking=True)
    arrived = torch.cuda.Event()
    arrived.record(s)
    return arrived


class Run:
    """Device side of one pipeline: its input buffers (holding A), staged
    copies of B, and whatever ``setup`` allocated."""

    def __init__(self, pipe):
        self.pipe = pipe
        self.A, self.B = pipe.inputs("A"), pipe.inputs("B")
        self.inp = {k: _dev(v) for k, v in self.A.items()}
        self.staged = {w: {k: _dev(v) for k, v in src.items()}
                       for w, src in (("A", self.A), ("B", self.B))}
        self.outputs = []
        pipe.setup(self)
        torch.cuda.synchronize()

    def zeros(self, nbytes):
        """A zero-filled buffer the chain writes results into (``clear``)."""
        self.outputs.append(_zeros(nbytes))
        return self.outputs[-1]

    def workspace(self, n, nb, tr):
        """A workspace of mgr_workspace_bytes: zero-filled once, then the
        library's alone -- never cleared or written by the harness."""
        return _zeros(_lib.load().mgr_workspace_bytes(int(n), int(nb), int(tr)))

    def clear(self):
        """The result buffers back to zeros: rows an earlier run left where
        this run writes none (a bin's region beyond its count, a set's slots
        beyond its size) would else remain.  Workspaces keep what the earlier
        run left in them, as they do between a caller's calls."""
        for t in self.outputs:
            t.zero_()

    def load(self, which, stream=None):
        """Copy input set A or B into the input buffers (stream-ordered)."""
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            for k, t in self.inp.items():
                t.copy_(self.staged[which][k], non_blocking=True)

    def late(self, s, which="B", sync=True):
        """The delay, the copies of ``which`` and the event on ``s``."""
        keys = list(self.inp)
        return late_copies(s, [self.inp[k] for k in keys], [self.staged[which][k] for k in keys],
                           sync)

    def enqueue(self, s, call=_lib.call):
        """The chain's calls on ``s`` through ``call(name, *args)``."""
        self.pipe.enqueue(self, s, _lib.stream_handle(s), call)

    def read(self):
        return self.pipe.read(self)


def still_late(arrived, when):
    assert not arrived.query(), (
        f"the late inputs had arrived {when}: the delay ({DELAY_NOTE}) is too short, or the "
        "call waited for the stream on the host")


def compare(got, want, what):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k in sorted(want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape,
                                                           w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(_bytes(g) != _bytes(w))
            raise AssertionError(f"{what}: output {k!r} differs in {bad.size} bytes, first at "
                                 f"byte {bad[0]}")


def differs(a, b):
    """The outputs that are NOT bytewise different between two model results."""
    return [k for k in a if np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()]


def same_outputs(pipe, a, b):
    """``differs`` without the pipeline's constant outputs: must be empty."""
    return [k for k in differs(a, b) if k not in pipe.constant]


def run_late(pipe, s, run=None):
    """The stream-order check of one pipeline on side stream ``s``."""
    run = run or Run(pipe)
    run.load("A")
    torch.cuda.synchronize()
    run.enqueue(s)            # once eagerly on complete inputs: the code objects load
    s.synchronize()
    run.clear()
    run.load("A")
    arrived = run.late(s)
    still_late(arrived, "before the call")
    run.enqueue(s)
    still_late(arrived, "when the last call of the chain returned")
    s.synchronize()
    compare(run.read(), pipe.model(run.B), f"{pipe.name} on a side stream, inputs late")
    return run


def run_control(pipe, s, idle):
    """The same arrangement with the chain on a second, idle stream: it must
    see the decoy.  Read before the late inputs overwrite the in-place ones."""
    run = Run(pipe)
    run.load("A")
    torch.cuda.synchronize()
    run.enqueue(idle)         # once eagerly: the idle stream's queue and the code objects exist
    idle.synchronize()
    run.clear()
    run.load("A")
    arrived = run.late(s)
    run.enqueue(idle)
    idle.synchronize()
    got = run.read()
    still_late(arrived, "after the control read its results")
    s.synchronize()
    want_a, want_b = pipe.model(run.A), pipe.model(run.B)
    compare(got, want_a, f"{pipe.name} control on an idle stream")
    assert not same_outputs(pipe, want_a, want_b)


# ------------------------------------------------------- mgr_synth_uniform
# The generator has no device input to arrive late; what arrives late is a
# decoy fill of its OUTPUT buffers: a launch on the right stream overwrites the
# decoy, a launch anywhere else runs first and is overwritten by it.
SYNTH_N, SYNTH_SEED, SYNTH_GID0, SYNTH_DECOY_VALUE = 3 * 256 + 77, 20261015, 1000, -7.0


def synth_model(n, seed=SYNTH_SEED, gid0=SYNTH_GID0):
    """(positions, 32-byte records [x, y, z (f64), id (i64)]) of the oracle."""
    pos = ro.synth_uniform(seed, gid0, n)
    rec = np.empty((n, 4), dtype=np.float64)
    rec[:, :3] = pos
    rec.view(np.int64)[:, 3] = np.arange(gid0, gid0 + n)
    return pos, rec.view(np.uint8).reshape(n, 32)


# ------------------------------------------------------------ the pipelines
class Pipeline:
    name = ""
    constant = ()      # outputs that hold the same value for every valid input

    def positions(self, rng, n, dt=np.float64):
        return rng.uniform(-0.3, 1.3, (n, 3)).astype(dt)

    def check_contract(self, inp):
        """Asserts that an input set is in contract (CPU)."""

    def sets_nonempty(self, inp):
        """Per-bin / per-set row counts that must all be positive in B."""
        return np.ones(1, dtype=np.int64)


class TwoPass(Pipeline):
    """mgr_bin_count -> mgr_scan -> mgr_pack_fields (12 B + 36 B) ->
    mgr_unpack_fields; mgr_pack, mgr_pack_tiles and mgr_unpack on the same scan;
    mgr_partition_by_position on a second copy of the positions."""
    name = "two-pass"
    nb = 8

    def __init__(self):
        self.tr = _tile_rows(32, self.nb)
        self.tr1 = _tile_rows(36, self.nb)
        self.n = 3 * self.tr + 77

    def inputs(self, which):
        rng = np.random.default_rng(100 + SEEDS[which])
        n = self.n
        pos = self.positions(rng, n)
        return {"pos": pos, "pos2": pos.copy(), "f12": _payload(rng, n, 12),
                "f36": _payload(rng, n, 36)}

    def bins(self, inp):
        p = inp["pos"].copy()
        return p, ro.cell_number_from_position(_geo(), p)

    def check_contract(self, inp):
        _, cell = self.bins(inp)
        assert cell.min() >= 0 and cell.max() < self.nb

    def sets_nonempty(self, inp):
        return np.bincount(self.bins(inp)[1], minlength=self.nb)

    def model(self, inp):
        p, cell = self.bins(inp)
        m = pack_model([inp["f12"], inp["f36"]], cell, self.nb, tile_rows=self.tr, sentinel=0)
        return {"pos": p, "pos2": p, "dest": cell.astype(np.uint8), "counts": m.counts,
                "counts2": m.counts, "p12": m.dst[0], "p36": m.dst[1], "u12": inp["f12"],
                "u36": inp["f36"], "p36b": m.dst[1], "p12b": m.dst[0], "u36b": inp["f36"],
                "part": m.dst[1]}

    def setup(self, r):
        n, nb = self.n, self.nb
        r.plan = _plan()
        r.ws, r.ws2 = r.workspace(n, nb, self.tr), r.workspace(n, nb, self.tr1)
        r.dest, r.dest2 = r.zeros(n), r.zeros(n)
        r.counts, r.counts2 = r.zeros(8 * nb), r.zeros(8 * nb)
        for k, rb in (("p12", 12), ("p36", 36), ("u12", 12), ("u36", 36), ("p36b", 36),
                      ("p12b", 12), ("u36b", 36), ("part", 36)):
            setattr(r, k, r.zeros(n * rb))

    def enqueue(self, r, s, sh, call):
        n, nb, tr, p = self.n, self.nb, self.tr, _lib.ptr
        i = r.inp
        common = (n, p(r.dest), nb, -1, tr, p(r.ws))
        call("mgr_bin_count", r.plan, p(i["pos"]), F64, n, 3, 1, p(r.dest), tr, p(r.ws), sh)
        call("mgr_scan", n, nb, tr, p(r.ws), p(r.counts), sh)
        call("mgr_pack_fields", 2, _ptrs([i["f12"], i["f36"]]), _i64([12, 36]), *common,
             _ptrs([r.p12, r.p36]), -1, None, None, None, None, 0, -1, sh)
        call("mgr_unpack_fields", 2, _ptrs([r.p12, r.p36]), _i64([12, 36]), *common,
             _ptrs([r.u12, r.u36]), -1, None, 0, -1, sh)
        call("mgr_pack", p(i["f36"]), 36, *common, p(r.p36b), -1, None, sh)
        T = (n + tr - 1) // tr
        for t0, t1 in ((2, T), (0, 2)):
            call("mgr_pack_tiles", p(i["f12"]), 12, *common, p(r.p12b), -1, None, None, None,
                 None, t0, t1, sh)
        call("mgr_unpack", p(r.p36b), 36, *common, p(r.u36b), -1, None, sh)
        call("mgr_partition_by_position", r.plan, p(i["pos2"]), F64, n, 3, 1, p(i["f36"]), 36,
             p(r.part), p(r.dest2), p(r.counts2), self.tr1, p(r.ws2), sh)

    def read(self, r):
        n, nb = self.n, self.nb
        out = {"pos": _host(r.inp["pos"], np.float64, (n, 3)),
               "pos2": _host(r.inp["pos2"], np.float64, (n, 3)),
               "dest": _host(r.dest, np.uint8, (n,)),
               "counts": _host(r.counts, np.int64, (nb,)),
               "counts2": _host(r.counts2, np.int64, (nb,))}
        for k, rb in (("p12", 12), ("p36", 36), ("u12", 12), ("u36", 36), ("p36b", 36),
                      ("p12b", 12), ("u36b", 36), ("part", 36)):
            out[k] = _host(getattr(r, k), np.uint8, (n, rb))
        return out


class ByIds(Pipeline):
    """mgr_cell_ids; mgr_bin_ids (a drop bin) -> mgr_scan -> mgr_pack_ids;
    mgr_cell_number_from_indexes."""
    name = "by-ids"
    P = 8

    def __init__(self):
        self.nb = self.P + 1
        self.tr = _tile_rows(8, self.nb)
        self.n = 3 * self.tr + 77

    def inputs(self, which):
        rng = np.random.default_rng(200 + SEEDS[which])
        n = self.n
        return {"pos": self.positions(rng, n),
                "ids": rng.integers(-1, self.P + 1, n).astype(np.int32),
                "src": _payload(rng, n, 8), "side": rng.integers(0, 1 << 16, n, dtype=np.uint16),
                "idx": rng.integers(-5, 8, (n, 3)).astype(np.int64)}

    def dest(self, inp):
        ids = inp["ids"].astype(np.int64)
        return np.where((ids < 0) | (ids >= self.P), self.P, ids)

    def check_contract(self, inp):
        d = self.dest(inp)
        assert d.min() >= 0 and d.max() < self.nb

    def sets_nonempty(self, inp):
        return np.bincount(self.dest(inp), minlength=self.nb)

    def model(self, inp):
        p = inp["pos"].copy()
        geo = _geo()
        idx = ro.cell_indexes_from_position(geo, p)
        d = self.dest(inp)
        m = pack_model([inp["src"]], d, self.nb, drop_bin=self.P, tile_rows=self.tr,
                       ids=inp["side"], sentinel=0)
        return {"pos": p, "cell": ro.cell_number_from_indexes(geo, idx), "cidx": idx,
                "dest": d.astype(np.uint8), "counts": m.counts, "dst": m.dst[0],
                "side_dst": m.ids_dst.reshape(-1).view(np.uint16),
                "cellnum": ro.cell_number_from_indexes(geo, inp["idx"])}

    def setup(self, r):
        n, nb = self.n, self.nb
        r.plan = _plan()
        r.ws, r.dest, r.counts = r.workspace(n, nb, self.tr), r.zeros(n), r.zeros(8 * nb)
        r.cell, r.cidx, r.cellnum = r.zeros(8 * n), r.zeros(24 * n), r.zeros(8 * n)
        r.dst, r.side_dst = r.zeros(8 * n), r.zeros(2 * n)

    def enqueue(self, r, s, sh, call):
        n, nb, tr, p = self.n, self.nb, self.tr, _lib.ptr
        i = r.inp
        call("mgr_cell_ids", r.plan, p(i["pos"]), F64, n, 3, 1, p(r.cell), p(r.cidx), sh)
        call("mgr_bin_ids", r.plan, p(i["ids"]), I32, n, p(r.dest), tr, p(r.ws), sh)
        call("mgr_scan", n, nb, tr, p(r.ws), p(r.counts), sh)
        call("mgr_pack_ids", p(i["src"]), 8, n, p(r.dest), nb, self.P, tr, p(r.ws), p(r.dst),
             -1, None, p(i["side"]), p(r.side_dst), None, sh)
        call("mgr_cell_number_from_indexes", r.plan, p(i["idx"]), n, 1, p(r.cellnum), sh)

    def read(self, r):
        n = self.n
        return {"pos": _host(r.inp["pos"], np.float64, (n, 3)),
                "cell": _host(r.cell, np.int64, (n,)), "cidx": _host(r.cidx, np.int64, (n, 3)),
                "dest": _host(r.dest, np.uint8, (n,)),
                "counts": _host(r.counts, np.int64, (self.nb,)),
                "dst": _host(r.dst, np.uint8, (n, 8)),
                "side_dst": _host(r.side_dst, np.uint16, (n,)),
                "cellnum": _host(r.cellnum, np.int64, (n,))}


class FineSort(Pipeline):
    """mgr_bin_count_fine -> mgr_rank_ids -> mgr_scan -> mgr_pack_ranked ->
    mgr_unpack_ranked_fields."""
    name = "fine-sort"
    constant = ("bad",)
    fine, nf = [4, 4, 4], 64

    def __init__(self):
        self.tr = _tile_rows(36, 8)
        self.rtr = _ranked_rows(36, self.nf)
        self.n = 3 * self.rtr + 77

    def inputs(self, which):
        rng = np.random.default_rng(300 + SEEDS[which])
        n = self.n
        return {"pos": self.positions(rng, n), "src": _payload(rng, n, 36),
                "v12": _payload(rng, n, 12), "v8": _payload(rng, n, 8)}

    def ids(self, inp):
        p = inp["pos"].copy()
        cell = ro.cell_number_from_position(_geo(), p)
        return p, cell, ro.fine_cell_ids(TOPO, self.fine, BOX, p)

    def check_contract(self, inp):
        _, cell, fid = self.ids(inp)
        assert cell.min() >= 0 and cell.max() < 8 and fid.min() >= 0 and fid.max() < self.nf

    def sets_nonempty(self, inp):
        return np.bincount(self.ids(inp)[2], minlength=self.nf)

    def model(self, inp):
        p, cell, fid = self.ids(inp)
        perm = np.argsort(fid, kind="stable")
        inv = _inv(perm)
        return {"pos": p, "dest": cell.astype(np.uint8), "fid": fid.astype(np.uint16),
                "counts": np.bincount(fid, minlength=self.nf).astype(np.int64),
                "sorted": inp["src"][perm], "u12": inp["v12"][inv], "u8": inp["v8"][inv],
                "bad": np.zeros(1, dtype=np.uint32)}

    def setup(self, r):
        n, nf = self.n, self.nf
        T = (n + self.rtr - 1) // self.rtr
        r.plan, r.fplan = _plan(), _plan(fine=self.fine)
        r.ws1, r.ws = r.workspace(n, 8, self.tr), r.workspace(n, nf, self.rtr)
        r.dest, r.fid, r.counts = r.zeros(n), r.zeros(2 * n), r.zeros(8 * nf)
        r.ranks, r.tstarts, r.bad = r.zeros(2 * n), r.zeros(8 * T * nf), r.zeros(4)
        r.sorted, r.u12, r.u8 = r.zeros(36 * n), r.zeros(12 * n), r.zeros(8 * n)

    def enqueue(self, r, s, sh, call):
        n, nf, rtr, p = self.n, self.nf, self.rtr, _lib.ptr
        i = r.inp
        with torch.cuda.stream(s):
            r.bad.zero_()              # the caller-zeroed word, in stream order
        call("mgr_bin_count_fine", r.plan, r.fplan, p(i["pos"]), F64, n, 3, 1, p(r.dest),
             p(r.fid), self.tr, p(r.ws1), sh)
        call("mgr_rank_ids", p(r.fid), n, nf, rtr, p(r.ranks), p(r.tstarts), p(r.bad),
             p(r.ws), sh)
        call("mgr_scan", n, nf, rtr, p(r.ws), p(r.counts), sh)
        call("mgr_pack_ranked", p(i["src"]), 36, n, p(r.fid), p(r.ranks), p(r.tstarts), nf,
             rtr, p(r.ws), p(r.sorted), sh)
        call("mgr_unpack_ranked_fields", 2, _ptrs([i["v12"], i["v8"]]), _i64([12, 8]), n,
             p(r.fid), p(r.ranks), p(r.tstarts), nf, rtr, p(r.ws), _ptrs([r.u12, r.u8]), sh)

    def read(self, r):
        n = self.n
        return {"pos": _host(r.inp["pos"], np.float64, (n, 3)),
                "dest": _host(r.dest, np.uint8, (n,)), "fid": _host(r.fid, np.uint16, (n,)),
                "counts": _host(r.counts, np.int64, (self.nf,)),
                "sorted": _host(r.sorted, np.uint8, (n, 36)),
                "u12": _host(r.u12, np.uint8, (n, 12)), "u8": _host(r.u8, np.uint8, (n, 8)),
                "bad": _host(r.bad, np.uint32, (1,))}


class OnePass(Pipeline):
    """mgr_partition_onepass (36-byte records holding f32 positions) and
    mgr_partition_onepass_fields (positions, velocities, masses, ids); both
    zero their workspace themselves, in stream order."""
    name = "one-pass"
    nb, RBS = 8, (12, 12, 4, 8)

    def __init__(self):
        self.n = self.cap = 3 * 1024 + 77        # the one-pass kernels' tiles hold 1024 rows

    def inputs(self, which):
        rng = np.random.default_rng(400 + SEEDS[which])
        n = self.n
        pos = self.positions(rng, n, np.float32)
        rec = _payload(rng, n, 36)
        rec[:, :12] = pos.view(np.uint8).reshape(n, 12)
        return {"pos": pos, "vel": _payload(rng, n, 12), "mass": _payload(rng, n, 4),
                "id": _payload(rng, n, 8), "rec": rec}

    def bins(self, inp):
        p = inp["pos"].copy()
        return p, ro.cell_number_from_position(_geo(), p)

    def check_contract(self, inp):
        p, cell = self.bins(inp)
        assert p.dtype == np.float32 and cell.min() >= 0 and cell.max() < self.nb

    def sets_nonempty(self, inp):
        return np.bincount(self.bins(inp)[1], minlength=self.nb)

    def regions(self, rows, cell):
        """Bin b's rows, in order, from row b * cap of a zero-filled output."""
        out = np.zeros((self.nb * self.cap, rows.shape[1]), dtype=np.uint8)
        for b in range(self.nb):
            sel = rows[cell == b]
            out[b * self.cap: b * self.cap + len(sel)] = sel
        return out

    def model(self, inp):
        p, cell = self.bins(inp)
        n = self.n
        pb = p.view(np.uint8).reshape(n, 12)
        counts = np.bincount(cell, minlength=self.nb).astype(np.int64)
        rec = inp["rec"].copy()
        rec[:, :12] = pb
        out = {"pos": p, "rec": rec, "counts": counts, "counts2": counts,
               "o_rec": self.regions(rec, cell), "o_pos": self.regions(pb, cell)}
        for k in ("vel", "mass", "id"):
            out["o_" + k] = self.regions(inp[k], cell)
        return out

    def setup(self, r):
        n, nb, cap = self.n, self.nb, self.cap
        wsb = int(_lib.load().mgr_onepass_workspace_bytes(n, nb))
        r.plan = _plan()
        r.ws, r.ws2 = _zeros(wsb), _zeros(wsb)      # workspaces: not cleared
        r.counts, r.counts2 = r.zeros(8 * nb), r.zeros(8 * nb)
        r.o_rec = r.zeros(nb * cap * 36)
        r.outs = [r.zeros(nb * cap * rb) for rb in self.RBS]

    def enqueue(self, r, s, sh, call):
        n, p = self.n, _lib.ptr
        i = r.inp
        call("mgr_partition_onepass", r.plan, None, p(i["rec"]), 36, 0, F32, n, 1, p(r.o_rec),
             None, self.cap, p(r.counts), p(r.ws), sh)
        call("mgr_partition_onepass_fields", r.plan, None, 4,
             _ptrs([i["pos"], i["vel"], i["mass"], i["id"]]), _i64(self.RBS), 0, 0, F32, n, 1,
             _ptrs(r.outs), None, self.cap, p(r.counts2), p(r.ws2), sh)

    def read(self, r):
        n, rows = self.n, self.nb * self.cap
        out = {"pos": _host(r.inp["pos"], np.float32, (n, 3)),
               "rec": _host(r.inp["rec"], np.uint8, (n, 36)),
               "counts": _host(r.counts, np.int64, (self.nb,)),
               "counts2": _host(r.counts2, np.int64, (self.nb,)),
               "o_rec": _host(r.o_rec, np.uint8, (rows, 36))}
        for k, t, rb in zip(("pos", "vel", "mass", "id"), r.outs, self.RBS):
            out["o_" + k] = _host(t, np.uint8, (rows, rb))
        return out


class Halo(Pipeline):
    """mgr_halo_flags, mgr_bin_count_halo; mgr_msel_count -> mgr_scan ->
    mgr_msel_pack, mgr_msel_pack_fields (4 fields: the wide kernel),
    mgr_msel_pack_placed -> mgr_msel_unpack_add."""
    name = "halo"
    K, TR, OL = 6, 4096, 0.1
    RBS = (12, 4, 8, 36)

    def __init__(self, seed=0):
        self.seed = seed
        self.tr1 = _tile_rows(36, 8)
        self.n = 3 * self.TR + 77
        self.masks = [1 << b for b in range(self.K)]

    def inputs(self, which):
        rng = np.random.default_rng(500 + SEEDS[which] + 10 * self.seed)
        n = self.n
        inp = {"pos": self.positions(rng, n),
               "acc": rng.integers(-1000, 1000, (n, 3)).astype(np.float32),
               "add": rng.integers(-1000, 1000, (self.K, n, 3)).astype(np.float32)}
        for f, rb in enumerate(self.RBS):
            inp[f"f{f}"] = _payload(rng, n, rb)
        return inp

    def flags(self, inp):
        """mgr_halo_flags of the positions as they arrive: bit 2d = x_d > hi_d,
        bit 2d + 1 = x_d < lo_d (float64)."""
        x = inp["pos"]
        f = np.zeros(self.n, dtype=np.uint16)
        for d in range(3):
            f |= ((x[:, d] > 1.0 - self.OL).astype(np.uint16) << np.uint16(2 * d))
            f |= ((x[:, d] < self.OL).astype(np.uint16) << np.uint16(2 * d + 1))
        return f

    def fused(self, inp):
        """mgr_bin_count_halo: the wrap and the cell (the oracle's), and the flags
        against the limits of the cell the row lands in (redist.py:271-275)."""
        geo = _geo()
        p = inp["pos"].copy()
        idx = ro.periodic_wrap(ro.cell_indexes_from_position(geo, p), geo.grid_topology)
        cell = ro.cell_number_from_indexes(geo, idx)
        lim = ro.cell_limits_from_indexes(geo, idx)
        f = np.zeros(self.n, dtype=np.uint16)
        for d in range(3):
            f |= ((p[:, d] > lim[:, d, 1] - self.OL).astype(np.uint16) << np.uint16(2 * d))
            f |= ((p[:, d] < lim[:, d, 0] + self.OL).astype(np.uint16) << np.uint16(2 * d + 1))
        return p, cell, f

    def members(self, inp):
        f = self.flags(inp)
        return [np.nonzero((f & m) == m)[0] for m in self.masks]

    def check_contract(self, inp):
        _, cell, f = self.fused(inp)
        allbits = (1 << self.K) - 1
        assert cell.min() >= 0 and cell.max() < 8
        assert (f & ~np.uint16(allbits)).max() == 0 and (self.flags(inp) & ~np.uint16(allbits)).max() == 0

    def sets_nonempty(self, inp):
        return np.array([len(m) for m in self.members(inp)])

    def model(self, inp):
        n, K = self.n, self.K
        p, cell, fused = self.fused(inp)
        mem = self.members(inp)
        counts = np.array([len(m) for m in mem], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)])
        out = {"pos": p, "flags": self.flags(inp), "dest": cell.astype(np.uint8), "fused": fused,
               "counts": counts}
        for f, rb in enumerate(self.RBS):
            src = inp[f"f{f}"]
            sets = np.zeros((K, n, rb), dtype=np.uint8)
            placed = np.zeros((K * n, rb), dtype=np.uint8)
            for k, m in enumerate(mem):
                sets[k, :len(m)] = src[m]
                placed[starts[k]: starts[k] + len(m)] = src[m]
            out[f"sets{f}"], out[f"placed{f}"] = sets, placed
        out["single"] = out["sets0"]
        acc = inp["acc"].copy()
        for k, m in enumerate(mem):       # k ascending, one float32 add per set
            acc[m] += inp["add"][k, :len(m)]
        out["acc"] = acc
        return out

    def setup(self, r):
        n, K = self.n, self.K
        r.plan = _plan()
        r.ws1, r.ws = r.workspace(n, 8, self.tr1), r.workspace(n, K, self.TR)
        r.flags, r.fused, r.dest, r.counts = r.zeros(2 * n), r.zeros(2 * n), r.zeros(n), r.zeros(8 * K)
        r.single = r.zeros(K * n * 12)
        r.sets = [r.zeros(K * n * rb) for rb in self.RBS]
        r.placed = [r.zeros(K * n * rb) for rb in self.RBS]
        r.hi = np.full(3, 1.0 - self.OL)
        r.lo = np.full(3, self.OL)
        r.cl = np.full(3, 0.5)
        r.ol = np.full(3, self.OL)
        r.cmasks = _ints(self.masks)

    def enqueue(self, r, s, sh, call):
        n, K, TR, p = self.n, self.K, self.TR, _lib.ptr
        i = r.inp
        sel = (n, p(r.flags), K, r.cmasks, TR, p(r.ws))
        srcs = [i[f"f{f}"] for f in range(4)]
        at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
        call("mgr_halo_flags", p(i["pos"]), F64, n, 3, 3, _vp(r.hi), _vp(r.lo), p(r.flags), sh)
        call("mgr_bin_count_halo", r.plan, p(i["pos"]), F64, n, 3, 1, p(r.dest), p(r.fused),
             _vp(r.cl), _vp(r.ol), self.tr1, p(r.ws1), sh)
        call("mgr_msel_count", p(r.flags), n, K, r.cmasks, TR, p(r.ws), sh)
        call("mgr_scan", n, K, TR, p(r.ws), p(r.counts), sh)
        one = (ctypes.c_void_p * K)(*[r.single.data_ptr() + k * n * 12 for k in range(K)])
        call("mgr_msel_pack", p(i["f0"]), 12, *sel, one, sh)
        dsts = (ctypes.c_void_p * (4 * K))(*[r.sets[f].data_ptr() + k * n * rb
                                             for f, rb in enumerate(self.RBS) for k in range(K)])
        call("mgr_msel_pack_fields", 4, _ptrs(srcs), _i64(self.RBS), *sel, dsts, sh)
        call("mgr_msel_pack_placed", 4, _ptrs(srcs), _i64(self.RBS), *sel, _ptrs(r.placed),
             K * n, sh)
        add = (ctypes.c_void_p * K)(*[at(i["add"], k * n * 12).value for k in range(K)])
        call("mgr_msel_unpack_add", p(i["acc"]), _lib.MGR_ELEM_F32, 3, *sel, add, sh)

    def read(self, r):
        n, K = self.n, self.K
        out = {"pos": _host(r.inp["pos"], np.float64, (n, 3)),
               "flags": _host(r.flags, np.uint16, (n,)), "dest": _host(r.dest, np.uint8, (n,)),
               "fused": _host(r.fused, np.uint16, (n,)),
               "counts": _host(r.counts, np.int64, (K,)),
               "single": _host(r.single, np.uint8, (K, n, 12)),
               "acc": _host(r.inp["acc"], np.float32, (n, 3))}
        for f, rb in enumerate(self.RBS):
            out[f"sets{f}"] = _host(r.sets[f], np.uint8, (K, n, rb))
            out[f"placed{f}"] = _host(r.placed[f], np.uint8, (K * n, rb))
        return out


class Ghost(Pipeline):
    """mgr_shift_regions -> mgr_ghost_cells; mgr_ghost_cells_wide on an 11 x 11
    x 11 extended grid -> mgr_id_digit -> two passes of mgr_rank_ids, mgr_scan
    and mgr_pack_ranked -> mgr_cell_offsets."""
    name = "ghost"
    constant = ("bad",)
    FINE, GHOST = [4, 4, 4], [1, 1, 1]
    WFINE, NCELLS = [9, 9, 9], 11 ** 3
    B0, B1, NB0, NB1 = 6, 5, 64, 21          # the balanced split of 11 bits
    SHIFTS = [[0.0, 0.0, 0.0], [1.0, 0.0, -1.0], [0.0, -1.0, 0.0]]

    def __init__(self):
        self.rtr0, self.rtr1 = _ranked_rows(36, self.NB0), _ranked_rows(36, self.NB1)
        self.n = 3 * self.rtr0 + 77
        self.n_owned = self.n // 2
        h = self.n - self.n_owned
        self.ends = [self.n_owned, self.n_owned + h // 2, self.n]
        self.origin = np.full(3, 0.25)
        self.width = np.full(3, 0.125)
        self.wwidth = 0.5 / np.asarray(self.WFINE, dtype=np.float64)

    def inputs(self, which):
        """Owned rows inside the cell [0.25, 0.75)^3; halo rows over the ghost
        layer of the wider of the two grids, stored as the periodic image
        that mgr_shift_regions moves beside the cell; some lie beyond the layers
        (clamped and counted in *outside)."""
        rng = np.random.default_rng(600 + SEEDS[which])
        n, no = self.n, self.n_owned
        pos = np.empty((n, 3))
        pos[:no] = 0.25 + rng.random((no, 3)) * 0.5
        pos[no:] = 0.11 + rng.random((n - no, 3)) * 0.78
        b = 0
        for e, sh in zip(self.ends, self.SHIFTS):
            pos[b:e] -= np.asarray(sh)
            b = e
        return {"pos": pos, "src": _payload(rng, n, 36)}

    def ids(self, inp):
        p = _shift_model(inp["pos"], 3, self.ends, self.SHIFTS)
        ids16, out16, _ = _ids_model(p, self.n_owned, 3, self.origin, self.width,
                                     np.asarray(self.FINE), np.asarray(self.GHOST))
        wide, outw = _model_ids(p, self.n_owned, self.origin, self.wwidth, self.WFINE, self.GHOST)
        return p, ids16, out16, wide, outw

    def check_contract(self, inp):
        _, ids16, _, wide, _ = self.ids(inp)
        assert ids16.max() < 6 ** 3 and wide.min() >= 0 and wide.max() < self.NCELLS
        s = np.sort(wide, kind="stable")
        assert (np.diff(s) >= 0).all()           # mgr_cell_offsets reads sorted ids

    def sets_nonempty(self, inp):
        wide = self.ids(inp)[3]
        return np.concatenate([np.bincount(wide & (self.NB0 - 1), minlength=self.NB0),
                               np.bincount(wide >> self.B0, minlength=self.NB1)])

    def model(self, inp):
        p, ids16, out16, wide, outw = self.ids(inp)
        order = np.argsort(wide, kind="stable")
        return {"pos": p, "ids16": ids16, "outside": np.array([out16, outw], dtype=np.uint32),
                "wide": wide.astype(np.uint32), "sorted": inp["src"][order],
                "sorted_ids": wide[order].astype(np.uint32),
                "offsets": _offsets(wide[order], self.NCELLS), "bad": np.zeros(1, np.uint32)}

    def setup(self, r):
        n = self.n
        T0, T1 = (n + self.rtr0 - 1) // self.rtr0, (n + self.rtr1 - 1) // self.rtr1
        r.ids16, r.wide, r.outside, r.bad = r.zeros(2 * n), r.zeros(4 * n), r.zeros(8), r.zeros(4)
        r.d0, r.d1 = r.zeros(2 * n), r.zeros(2 * n)
        r.ws0, r.ws1 = r.workspace(n, self.NB0, self.rtr0), r.workspace(n, self.NB1, self.rtr1)
        r.ranks0, r.ranks1 = r.zeros(2 * n), r.zeros(2 * n)
        r.ts0, r.ts1 = r.zeros(8 * T0 * self.NB0), r.zeros(8 * T1 * self.NB1)
        r.c0, r.c1 = r.zeros(8 * self.NB0), r.zeros(8 * self.NB1)
        r.mid, r.mid_ids = r.zeros(36 * n), r.zeros(4 * n)
        r.sorted, r.sorted_ids = r.zeros(36 * n), r.zeros(4 * n)
        r.offsets = r.zeros(8 * (self.NCELLS + 1))
        r.ends = _i64(self.ends)
        r.shifts = (ctypes.c_double * 9)(*[v for row in self.SHIFTS for v in row])

    def enqueue(self, r, s, sh, call):
        n, p = self.n, _lib.ptr
        i = r.inp
        with torch.cuda.stream(s):
            r.outside.zero_()          # the caller-zeroed words, in stream order
            r.bad.zero_()
        call("mgr_shift_regions", p(i["pos"]), F64, n, 3, 3, 3, r.ends, r.shifts, sh)
        grid = (p(i["pos"]), F64, n, self.n_owned, 3, 3, _vp(self.origin))
        call("mgr_ghost_cells", *grid, _vp(self.width), _ints(self.FINE), _ints(self.GHOST),
             p(r.ids16), p(r.outside), sh)
        call("mgr_ghost_cells_wide", *grid, _vp(self.wwidth), _ints(self.WFINE),
             _ints(self.GHOST), p(r.wide), ctypes.c_void_p(r.outside.data_ptr() + 4), sh)
        passes = ((r.wide, 0, self.B0, r.d0, self.NB0, self.rtr0, r.ranks0, r.ts0, r.ws0, r.c0,
                   i["src"], r.mid, r.mid_ids),
                  (r.mid_ids, self.B0, self.B1, r.d1, self.NB1, self.rtr1, r.ranks1, r.ts1, r.ws1,
                   r.c1, r.mid, r.sorted, r.sorted_ids))
        for ids, shift, bits, d, nb, rtr, ranks, ts, ws, c, src, out, ids_out in passes:
            call("mgr_id_digit", p(ids), n, shift, bits, p(d), sh)
            call("mgr_rank_ids", p(d), n, nb, rtr, p(ranks), p(ts), None, p(ws), sh)
            call("mgr_scan", n, nb, rtr, p(ws), p(c), sh)
            for a, b, rb in ((src, out, 36), (ids, ids_out, 4)):
                call("mgr_pack_ranked", p(a), rb, n, p(d), p(ranks), p(ts), nb, rtr, p(ws),
                     p(b), sh)
        call("mgr_cell_offsets", p(r.sorted_ids), n, self.NCELLS, p(r.offsets), p(r.bad), sh)

    def read(self, r):
        n = self.n
        return {"pos": _host(r.inp["pos"], np.float64, (n, 3)),
                "ids16": _host(r.ids16, np.uint16, (n,)),
                "outside": _host(r.outside, np.uint32, (2,)),
                "wide": _host(r.wide, np.uint32, (n,)),
                "sorted": _host(r.sorted, np.uint8, (n, 36)),
                "sorted_ids": _host(r.sorted_ids, np.uint32, (n,)),
                "offsets": _host(r.offsets, np.int64, (self.NCELLS + 1,)),
                "bad": _host(r.bad, np.uint32, (1,))}


PIPELINES = {c.name: c for c in (TwoPass, ByIds, FineSort, OnePass, Halo, Ghost)}
