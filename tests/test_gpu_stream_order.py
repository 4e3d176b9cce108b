"""Stream ordering of the device entry points (include/mgr.h: "everything that
takes a stream is stream-ordered and asynchronous: no host synchronisation").

Every chain runs on a side stream while torch's current stream stays the default
one; its inputs arrive late on that side stream (tests/stream_order.py: a delay,
then device copies of the real input B over the decoy A).  A kernel launched on
any other stream reads the decoy; a host sync inside an entry
shows as the late inputs having arrived when the call returns.  Results are
compared exactly with the suite's numpy models.  One control per pipeline runs
the same chain on an idle second stream and must get model(A)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import stream_order as so

pytestmark = pytest.mark.gpu

from mpi_grid_redistribute_amd import (CELLS_MAX, GridPartitioner, MPIGridRedistributor,  # noqa: E402
                                       SortRoute, _lib, synth_uniform)

C_CHAINS = ["two-pass", "by-ids", "fine-sort", "one-pass", "halo", "ghost"]
_STREAMS = {}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _streams():
    """The two side streams of this module (one process, no third stream)."""
    if not _STREAMS:
        _STREAMS["s"], _STREAMS["t"] = torch.cuda.Stream(), torch.cuda.Stream()
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    return _STREAMS["s"], _STREAMS["t"]


# ----------------------------------------------------------------- C entries
@pytest.mark.parametrize("name", C_CHAINS)
def test_c_chain_follows_its_stream(name):
    s, _ = _streams()
    so.run_late(so.PIPELINES[name](), s)


@pytest.mark.parametrize("name", C_CHAINS)
def test_control_on_an_idle_stream_sees_the_decoy(name):
    s, idle = _streams()
    so.run_control(so.PIPELINES[name](), s, idle)


def _synth_buffers(n):
    pos = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    rec = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    decoy = [torch.full_like(pos, so.SYNTH_DECOY_VALUE), torch.full_like(rec, so.SYNTH_DECOY_VALUE)]
    return pos, rec, decoy


def _synth_call(pos, rec, stream):
    box = np.ones(3, dtype=np.float64)
    _lib.call("mgr_synth_uniform", ctypes.c_uint64(so.SYNTH_SEED), so.SYNTH_GID0, so.SYNTH_N, 3,
              box.ctypes.data_as(ctypes.c_void_p), _lib.ptr(pos), _lib.ptr(rec),
              _lib.stream_handle(stream))


def test_c_synth_uniform_follows_its_stream():
    """The decoy fill of the outputs is late on ``s``; the generator launched on
    ``s`` overwrites it.  Control: launched on the idle stream it is overwritten."""
    s, idle = _streams()
    n = so.SYNTH_N
    want_pos, want_rec = so.synth_model(n)
    pos, rec, decoy = _synth_buffers(n)
    for st in (s, idle):               # once eagerly: the code object and both queues exist
        _synth_call(pos, rec, st)
        st.synchronize()
    pos.zero_()
    rec.zero_()
    arrived = so.late_copies(s, [pos, rec], decoy)
    so.still_late(arrived, "before the call")
    _synth_call(pos, rec, s)
    so.still_late(arrived, "when mgr_synth_uniform returned")
    s.synchronize()
    assert pos.cpu().numpy().tobytes() == want_pos.tobytes()
    assert rec.cpu().numpy().view(np.uint8).reshape(n, 32).tobytes() == want_rec.tobytes()
    pos, rec, decoy = _synth_buffers(n)
    arrived = so.late_copies(s, [pos, rec], decoy)
    _synth_call(pos, rec, idle)
    idle.synchronize()
    assert pos.cpu().numpy().tobytes() == want_pos.tobytes()      # it did run
    so.still_late(arrived, "after the control read its result")
    s.synchronize()
    assert bool((pos == so.SYNTH_DECOY_VALUE).all()) and bool((rec == so.SYNTH_DECOY_VALUE).all())


# ------------------------------------------------- Python stream= parameters
def _np(x):
    """Every tensor inside a (nested) result as numpy, in order."""
    if isinstance(x, torch.Tensor):
        return [x.detach().cpu().numpy().copy()]
    if isinstance(x, np.ndarray):
        return [x.copy()]
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _np(y)]
    return []


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i, g.dtype, w.dtype, g.shape,
                                                           w.shape)
        assert g.tobytes() == w.tobytes(), f"{what}: result {i} differs from the default-stream one"


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _late_call(s, inputs_a, inputs_b, call, what, no_sync=True, on_current=False):
    """``call(tensors, stream)`` on the default stream with B (the reference,
    copied to the host at once: the library reuses its cached outputs), then
    with the buffers holding A and B arriving late on ``s``; both results (and
    the inputs, which a call may wrap in place) must agree."""
    ref_in = [_cuda(b) for b in inputs_b]
    want = _np(call(ref_in, None)) + _np(ref_in)
    torch.cuda.synchronize()
    bufs, staged = [_cuda(a) for a in inputs_a], [_cuda(b) for b in inputs_b]
    arrived = so.late_copies(s, bufs, staged)
    so.still_late(arrived, "before the call")
    if on_current:
        with torch.cuda.stream(s):
            res = call(bufs, None)
    else:
        res = call(bufs, s)
    if no_sync:
        so.still_late(arrived, f"when {what} returned")
    s.synchronize()
    _same(_np(res) + _np(bufs), want, what)


def _flat(t):
    return t.view(torch.uint8).reshape(-1)


def _filled(out, counts, cap, rb):
    """The rows the one-pass partition wrote: bin b's counts[b] rows from row
    b * cap (the rest of a region is not written)."""
    c = counts.cpu().tolist()
    return [out[b * cap * rb: (b * cap + int(k)) * rb] for b, k in enumerate(c)]


def test_partitioner_stream_parameters():
    s, _ = _streams()
    pipe = so.PIPELINES["two-pass"]()
    a, b = pipe.inputs("A"), pipe.inputs("B")
    n = pipe.n
    P = GridPartitioner(so.TOPO, so.BOX)

    def part(t, st):
        out, counts = P.partition_device(_flat(t[1]), 36, t[0], stream=st)
        return out[:n * 36], counts

    _late_call(s, [a["pos"], a["f36"]], [b["pos"], b["f36"]], part, "partition_device")

    def unpart(t, st):      # the way back through the partition made just above
        return P.unpartition_device(_flat(t[0]), 36, stream=st)[:n * 36]

    _late_call(s, [a["f36"]], [b["f36"]], unpart, "unpartition_device")

    def part_fields(t, st):
        outs, counts = P.partition_fields_device([_flat(t[1]), _flat(t[2])], [12, 36], t[0],
                                                 stream=st)
        return [o[:n * rb] for o, rb in zip(outs, (12, 36))], counts

    _late_call(s, [a["pos"], a["f12"], a["f36"]], [b["pos"], b["f12"], b["f36"]], part_fields,
               "partition_fields_device")

    def unpart_fields(t, st):
        outs = P.unpartition_fields_device([_flat(t[0]), _flat(t[1])], [12, 36], stream=st)
        return [o[:n * rb] for o, rb in zip(outs, (12, 36))]

    _late_call(s, [a["f12"], a["f36"]], [b["f12"], b["f36"]], unpart_fields,
               "unpartition_fields_device")


def test_partitioner_onepass_stream_parameters():
    s, _ = _streams()
    pipe = so.PIPELINES["one-pass"]()
    a, b = pipe.inputs("A"), pipe.inputs("B")
    P = GridPartitioner(so.TOPO, so.BOX)

    def onepass(t, st):
        rec = t[0]
        out, _, counts, cap = P.partition_onepass_device(_flat(rec), 36, rec.view(torch.float32)
                                                         [:, :3], stream=st)
        if st is not None:
            st.synchronize()
        return _filled(out, counts, cap, 36), counts

    def onepass_nosync(t, st):
        rec = t[0]
        return P.partition_onepass_device(_flat(rec), 36, rec.view(torch.float32)[:, :3],
                                          stream=st)[2]

    _late_call(s, [a["rec"]], [b["rec"]], onepass_nosync, "partition_onepass_device")
    _late_call(s, [a["rec"]], [b["rec"]], onepass, "partition_onepass_device", no_sync=False)
    keys, rbs = ("pos", "vel", "mass", "id"), [12, 12, 4, 8]

    def fields(t, st):
        outs, _, counts, cap = P.partition_onepass_fields_device([_flat(x) for x in t], rbs, t[0],
                                                                 stream=st)
        if st is not None:
            st.synchronize()
        return [_filled(o, counts, cap, rb) for o, rb in zip(outs, rbs)], counts

    def fields_nosync(t, st):
        return P.partition_onepass_fields_device([_flat(x) for x in t], rbs, t[0], stream=st)[2]

    ia, ib = [a[k] for k in keys], [b[k] for k in keys]
    _late_call(s, ia, ib, fields_nosync, "partition_onepass_fields_device")
    _late_call(s, ia, ib, fields, "partition_onepass_fields_device", no_sync=False)


def test_synth_uniform_stream_parameter():
    """synth_uniform(stream=s) returns tensors that are complete: read on the
    default stream straight after the call.  The default-stream reference stays
    alive meanwhile, so the allocator cannot hand its blocks (which already
    hold the right bytes) to the side-stream call."""
    s, _ = _streams()
    n = 1 << 20
    ref_pos, ref_rec = synth_uniform(n, seed=so.SYNTH_SEED, gid0=so.SYNTH_GID0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(so.DELAY_CYCLES)
    pos, rec = synth_uniform(n, seed=so.SYNTH_SEED, gid0=so.SYNTH_GID0, stream=s)
    got_pos, got_rec = pos.cpu(), rec.cpu()          # default stream, no sync of ours
    s.synchronize()
    assert pos.data_ptr() != ref_pos.data_ptr() and rec.data_ptr() != ref_rec.data_ptr()
    assert torch.equal(got_pos, ref_pos.cpu()), "synth_uniform(stream=s) returned before s was done"
    assert torch.equal(got_rec, ref_rec.cpu())
    want_pos, _ = so.synth_model(so.SYNTH_N)
    assert got_pos[:so.SYNTH_N].numpy().tobytes() == want_pos.tobytes()


# ------------------------------------------- current-stream APIs on a side stream
def _rows(n, seed, lo=-0.3, hi=1.3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(lo, hi, (n, 3)), rng.integers(0, 256, (n, 36), dtype=np.uint8),
            rng.integers(-1000, 1000, (n, 3)).astype(np.float32)]


N_API = 3 * 4096 + 77


def test_redistribute_by_position_on_a_side_stream():
    s, _ = _streams()
    R = MPIGridRedistributor(None, [1, 1, 1], so.BOX)
    a, b = _rows(N_API, 1)[:2], _rows(N_API, 2)[:2]
    _late_call(s, a, b, lambda t, st: R.redistribute_by_position(t[1], t[0]),
               "redistribute_by_position", no_sync=False, on_current=True)
    _late_call(s, a, b, lambda t, st: R.redistribute_by_position(
        t[1], t[0], overload_lengths=[0.1, 0.1, 0.1], return_positions=True),
        "redistribute_by_position(overload_lengths=)", no_sync=False, on_current=True)


def test_fine_cell_sort_and_unsort_on_a_side_stream():
    s, _ = _streams()
    R = MPIGridRedistributor(None, [1, 1, 1], so.BOX)

    def call(t, st):
        res = R.fine_cell_sort(t[1], t[0], [4, 4, 4], return_route=True)
        route = [x for x in res if isinstance(x, SortRoute)][0]
        return res, R.unsort(t[2], route)

    _late_call(s, _rows(N_API, 3, 0.0, 1.0), _rows(N_API, 4, 0.0, 1.0), call,
               "fine_cell_sort + unsort", no_sync=False, on_current=True)


def test_ghost_cell_sort_wide_on_a_side_stream():
    s, _ = _streams()
    R = MPIGridRedistributor(None, [1, 1, 1], so.BOX)
    fine = [11, 11, 11]                # 1331 cells: the two-digit sort

    def call(t, st):
        return R.ghost_cell_sort(t[1], t[0], N_API, fine, [0.0, 0.0, 0.0], return_positions=True,
                                 max_cells=CELLS_MAX)

    _late_call(s, _rows(N_API, 5, 0.0, 1.0)[:2], _rows(N_API, 6, 0.0, 1.0)[:2], call,
               "ghost_cell_sort(max_cells=)", no_sync=False, on_current=True)


def test_return_to_source_on_a_side_stream():
    s, _ = _streams()
    R = MPIGridRedistributor(None, [1, 1, 1], so.BOX)
    pos, data, _ = [_cuda(x) for x in _rows(N_API, 7)]
    _, route = R.redistribute_by_position(data, pos, return_route=True)
    torch.cuda.synchronize()
    _late_call(s, _rows(N_API, 8)[2:], _rows(N_API, 9)[2:],
               lambda t, st: R.return_to_source(t[0], route), "return_to_source", no_sync=False,
               on_current=True)


# ------------------------------------------------------- two streams at once
def test_two_chains_overlap_on_two_streams():
    """The two-pass chain on one stream and the halo chain on the other, each
    with workspaces and a late B of its own, enqueued call by call in turns."""
    s, t = _streams()
    one, two = so.Run(so.TwoPass()), so.Run(so.Halo(seed=1))
    for run, st in ((one, s), (two, t)):    # once eagerly on complete inputs
        run.load("A")
        torch.cuda.synchronize()
        run.enqueue(st)
        st.synchronize()
        run.clear()
    one.load("A")
    two.load("A")
    torch.cuda.synchronize()
    arrived = [one.late(s, sync=False), two.late(t, sync=False)]
    calls = [so.deferred(one, s), so.deferred(two, t)]
    for i in range(max(len(c) for c in calls)):
        for c in calls:
            if i < len(c):
                _lib.call(c[i][0], *c[i][1])
    for ev in arrived:
        so.still_late(ev, "when both chains were enqueued")
    s.synchronize()
    t.synchronize()
    so.compare(one.read(), one.pipe.model(one.B), "two-pass beside the halo chain")
    so.compare(two.read(), two.pipe.model(two.B), "halo beside the two-pass chain")
