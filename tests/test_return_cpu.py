"""The reverse exchange on the host (no GPU): exchange() forward with a numpy
stable partition as the pack, then exchange_back() with a numpy stand-in for
the unpack, must be the identity on every rank -- threads over MpiHostComm
and gloo processes over TorchDistComm, skewed counts with an empty rank, both
redirect_self values, two fields of different row bytes.  The way back never
exchanges counts, and its traffic is the forward call's with the directions
swapped."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mpi_grid_redistribute_amd.comm import MpiHostComm, TorchDistComm
from mpi_grid_redistribute_amd.exchange import exchange, exchange_back, plan_layout
from tests.fake_mpi import run_ranks

ROW_BYTES = [24, 4]            # forward payload: 24-byte records + 4-byte tags
BACK_BYTES = [8, 12]           # what comes back: unrelated row sizes


def rank_inputs(size, rank, empty_rank):
    """Skewed destinations: most rows of every rank go to rank 0."""
    rng = np.random.default_rng(1000 + 17 * size + rank)
    n = 0 if rank == empty_rank else int(rng.integers(200, 1500)) * (1 + 2 * (rank % 2))
    dest = np.where(rng.random(n) < 0.6, 0, rng.integers(0, size, n)).astype(np.int64)
    gid = np.arange(n, dtype=np.int64) + 1_000_000 * rank
    f0 = np.zeros((n, 3), dtype=np.int64)
    f0[:, 0], f0[:, 1], f0[:, 2] = gid, gid * 3 + 1, dest
    f1 = (gid & 0x7FFFFFFF).astype(np.int32).reshape(n, 1)
    return dest, gid, [f0, f1]


def slots_of(dest, size, redirect_bin):
    """(slot, in_redirect) of every row for mgr_pack's layout: bin-major,
    stable, the redirect bin from row 0 of its own buffer and its gap closed."""
    order = np.argsort(dest, kind="stable")
    counts = np.bincount(dest, minlength=size)
    starts = np.concatenate([[0], np.cumsum(counts)])
    slot = np.empty(len(dest), dtype=np.int64)
    slot[order] = np.arange(len(dest))
    red = dest == redirect_bin
    if redirect_bin >= 0:
        slot[red] -= starts[redirect_bin]
        slot[dest > redirect_bin] -= counts[redirect_bin]
    return slot, red, counts


def numpy_pack(fields, row_bytes, dest, size):
    """Stand-in for mgr_pack_fields (exchange()'s pack_all)."""
    def pack_all(sends, outs, redirect_bin, offs):
        slot, red, _ = slots_of(dest, size, redirect_bin)
        for f, rb in enumerate(row_bytes):
            raw = torch.from_numpy(np.ascontiguousarray(fields[f]).view(np.uint8).reshape(-1, rb))
            if (~red).any():
                snd = sends[f][: int((~red).sum()) * rb].view(-1, rb)
                snd[torch.from_numpy(slot[~red])] = raw[torch.from_numpy(~red)]
            if red.any():
                k = int(red.sum())
                out = outs[f][offs[f]: offs[f] + k * rb].view(-1, rb)
                out[torch.from_numpy(slot[red])] = raw[torch.from_numpy(red)]
    return pack_all


def numpy_unpack(row_bytes, dest, size):
    """Stand-in for mgr_unpack_fields (exchange_back()'s unpack_all)."""
    def unpack_all(stagings, values, redirect_bin, offs):
        slot, red, _ = slots_of(dest, size, redirect_bin)
        outs = []
        for f, rb in enumerate(row_bytes):
            out = np.zeros((len(dest), rb), dtype=np.uint8)
            stg = stagings[f].numpy()
            val = values[f].numpy()[offs[f]:]
            out[~red] = stg[: int((~red).sum()) * rb].reshape(-1, rb)[slot[~red]]
            if red.any():
                out[red] = val[: int(red.sum()) * rb].reshape(-1, rb)[slot[red]]
            outs.append(out)
        return outs
    return unpack_all


class CountingTransport:
    """Delegates to a transport; counts the count exchanges."""

    def __init__(self, inner):
        self.inner, self.count_calls = inner, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def exchange_counts(self, c):
        self.count_calls += 1
        return self.inner.exchange_counts(c)

    def exchange_count_rows(self, c):
        self.count_calls += 1
        return self.inner.exchange_count_rows(c)


def round_trip(transport, size, rank, empty_rank, redirect_self):
    dest, gid, fields = rank_inputs(size, rank, empty_rank)
    t = CountingTransport(transport)
    counts = torch.from_numpy(np.bincount(dest, minlength=size).astype(np.int64))
    t.reset_traffic()
    outs, lay = exchange(t, ROW_BYTES, counts, rank, "cpu", None,
                         pack_all=numpy_pack(fields, ROW_BYTES, dest, size))
    assert t.count_calls == 1
    fwd = t.traffic
    if redirect_self != lay.redirect_self:
        # the other flag (a pipelined forward always redirects the self rows): the
        # received rows are laid out the same way, only the send side differs
        lay = plan_layout(lay.send_counts, lay.recv_counts, rank, redirect_self)
    m = lay.total_recv
    got = outs[0][: m * 24].numpy().view(np.int64).reshape(m, 3)
    assert (got[:, 2] == rank).all()                      # every received row is this rank's
    # the "result" computed at the destination: functions of the received ids
    v0 = (got[:, 0] * 7 + 5).astype(np.int64).reshape(m, 1)
    v1 = np.stack([got[:, 0] % 251, got[:, 1] % 65521, got[:, 0] % 7], axis=1).astype(np.int32)
    values = [torch.from_numpy(v.view(np.uint8).reshape(-1).copy()) for v in (v0, v1)]
    t.reset_traffic()
    back = exchange_back(t, BACK_BYTES, lay, values, rank, "cpu",
                         numpy_unpack(BACK_BYTES, dest, size))
    assert t.count_calls == 1                             # no count exchange on the way back
    r0 = back[0].view(np.int64).reshape(-1)
    r1 = back[1].view(np.int32).reshape(-1, 3)
    assert np.array_equal(r0, gid * 7 + 5)
    assert np.array_equal(r1, np.stack([gid % 251, (gid * 3 + 1) % 65521, gid % 7],
                                       axis=1).astype(np.int32))
    # traffic: the forward rows with send and receive swapped, at the back row
    # bytes, and without the count messages
    fb, bb = sum(ROW_BYTES), sum(BACK_BYTES)
    peers = np.arange(size) != rank
    assert ((fwd.send - 8 * peers) % fb == 0).all()
    assert np.array_equal(t.traffic.recv, (fwd.send - 8 * peers) // fb * bb)
    assert np.array_equal(t.traffic.send, (fwd.recv - 8 * peers) // fb * bb)
    assert t.traffic.send[rank] == 0 and t.traffic.recv[rank] == 0
    return True


@pytest.mark.parametrize("redirect_self", [True, False])
@pytest.mark.parametrize("size,empty_rank", [(4, 2), (3, None)])
def test_threads_forward_then_back_is_identity(size, empty_rank, redirect_self):
    def fn(comm, r):
        return round_trip(MpiHostComm(comm), size, r, empty_rank, redirect_self)
    assert all(run_ranks(size, fn))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, size, port, empty_rank, redirect_self):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=size)
    try:
        comm = TorchDistComm()
        assert round_trip(comm, size, rank, empty_rank, redirect_self)
        comm.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("size,empty_rank,redirect_self", [(2, 1, False), (2, None, True),
                                                           (3, 0, False), (3, 1, True)])
def test_gloo_forward_then_back_is_identity(size, empty_rank, redirect_self):
    mp.spawn(_gloo_worker, args=(size, _free_port(), empty_rank, redirect_self), nprocs=size,
             join=True)


def test_single_rank_self_comm():
    """World 1: nothing travels, the unpack reads the values in place."""
    from mpi_grid_redistribute_amd.comm import SelfComm
    assert round_trip(SelfComm(), 1, 0, None, True)
