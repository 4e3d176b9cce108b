"""One rank of the multi-process return-path run (tests/test_gpu_return_multi.py):
redistribute with ``return_route=True`` over RcclComm, compute per-row values
at the destination, bring them back with ``return_to_source`` -- the reverse
row exchange as one RCCL group between distinct processes.  The ids pin the
bijection, so every check is this rank's own ids against what came back.

Environment as tests/rccl_worker.py: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT
(gloo rendezvous for the RCCL unique id), MGR_TEST_OUT (result file),
MGR_TEST_SHARED_GPU=1 when the ranks share GPU 0 (each rank then presents its
own NCCL_HOSTID and RCCL connects them over loopback sockets), MGR_CASE_TIMEOUT.
Every case runs under a watchdog; the first failing case ends this rank (and,
through the barrier, the run).
"""
from __future__ import annotations

import json
import os
import sys
import threading
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK = int(os.environ["RANK"])
WORLD = int(os.environ["WORLD_SIZE"])
SHARED = os.environ.get("MGR_TEST_SHARED_GPU") == "1"
if SHARED:   # before anything loads RCCL
    os.environ["NCCL_HOSTID"] = f"mgr-test-rank-{RANK}"
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_DEBUG", "WARN")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tests import golden_io as G  # noqa: E402

TOPO = {2: [2, 1, 1], 4: [2, 2, 1]}
BOX = [1.0, 1.0, 1.0]
CASE_TIMEOUT_S = float(os.environ.get("MGR_CASE_TIMEOUT", "60"))


def log(msg):
    print(f"[rank {RANK}/{WORLD} {time.strftime('%H:%M:%S')}] {msg}", flush=True)


def _sizes():
    sizes = [int(np.random.default_rng(40 + r).integers(2000, 40_000)) for r in range(WORLD)]
    sizes[WORLD - 1] = 0                                   # an empty rank
    return sizes


def _inputs(seed):
    n = _sizes()[RANK]
    rng = np.random.default_rng(seed + RANK)
    return rng.uniform(-0.5, 1.5, (n, 3)), np.arange(n, dtype=np.int64) + 1_000_000 * RANK


def _values(ids):
    v1 = ids * 3 + 1
    v2 = np.stack([ids % 1000, ids % 77, -(ids % 13)], axis=1).astype(np.float32)
    v3 = (ids & 255).astype(np.uint8)
    return v1, v2, v3


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def case_round_trip(mgr, comm, seed, as_torch, chunks):
    """(pos, ids) forward; one array back, then three fields (SoA) back along
    the same route; traffic = the forward call's, directions swapped."""
    R = mgr.MPIGridRedistributor(comm, TOPO[WORLD], BOX)
    R.exchange_chunks = chunks
    pos, ids = _inputs(seed)
    conv = (lambda x: torch.from_numpy(x).cuda()) if as_torch else (lambda x: x)
    p_in = conv(pos.copy())
    (lpos, lids), route = R.redistribute_by_position((p_in, conv(ids.copy())), p_in,
                                                     return_route=True)
    fwd = R.last_traffic
    assert route.n_source == len(ids) and route.n_local == len(lids)
    one = R.return_to_source(conv(_np(lids) * 3 + 1), route)
    assert G.same_bytes(_np(one), ids * 3 + 1), "single array"
    back = R.return_to_source(tuple(conv(v) for v in _values(_np(lids))), route)
    bwd = R.last_traffic
    for b, w in zip(back, _values(ids)):
        assert G.same_bytes(_np(b), w), "SoA return"
    wrapped = ((pos % 1.0) + 1.0) % 1.0
    assert G.same_bytes(_np(R.return_to_source(lpos, route)), wrapped), "positions"
    k = 1 if chunks == 1 else 1 + chunks                   # int64 words of a count message
    for p in range(WORLD):
        if p == RANK:
            continue
        fs, fr = fwd["send_per_peer"][p] - 8 * k, fwd["recv_per_peer"][p] - 8 * k
        assert fs % 32 == 0 and fr % 32 == 0
        assert bwd["recv_per_peer"][p] == fs // 32 * 21, "traffic"
        assert bwd["send_per_peer"][p] == fr // 32 * 21, "traffic"
    torch.cuda.synchronize()


def case_cell_number(mgr, comm, seed):
    R = mgr.MPIGridRedistributor(comm, TOPO[WORLD], BOX)
    _, ids = _inputs(seed)
    to = np.random.default_rng(seed + 100 + RANK).integers(-1, WORLD + 1, len(ids))
    lids, route = R.redistribute_by_cell_number(ids, to, return_route=True)
    v1, v2, _ = _values(lids)
    b1, b2 = R.return_to_source((v1, v2), route)
    kept = (to >= 0) & (to < WORLD)
    w1, w2, _ = _values(ids)
    w1[~kept] = 0
    w2[~kept] = 0
    assert G.same_bytes(b1, w1) and G.same_bytes(b2, w2), "dropped rows"
    torch.cuda.synchronize()


def main():
    out_path = os.environ["MGR_TEST_OUT"]
    results = {}
    torch.cuda.set_device(0 if SHARED else RANK)
    dist.init_process_group("gloo", rank=RANK, world_size=WORLD)
    import mpi_grid_redistribute_amd as mgr
    comm = mgr.RcclComm.from_torch_distributed()
    log("RcclComm up")
    cases = [
        ("round_trip_empty_rank", lambda: case_round_trip(mgr, comm, 81, False, 1)),
        ("round_trip_pipelined_forward", lambda: case_round_trip(mgr, comm, 82, True, 4)),
        ("cell_number_drops", lambda: case_cell_number(mgr, comm, 83)),
    ]

    def finish(code):
        with open(out_path, "w") as fh:
            json.dump(results, fh)
        os._exit(code)

    for name, fn in cases:
        t0 = time.perf_counter()

        def _hung(n=name):
            log(f"{n}: HUNG (> {CASE_TIMEOUT_S} s), exiting")
            results[n] = f"FAIL: hung > {CASE_TIMEOUT_S} s"
            finish(4)
        dog = threading.Timer(CASE_TIMEOUT_S, _hung)
        dog.daemon = True
        dog.start()
        try:
            fn()
            results[name] = "ok"
            dist.barrier()                  # a peer that failed has left: this raises
        except Exception as e:
            results[name] = f"FAIL: {e!r}\n{traceback.format_exc()}"
        dog.cancel()
        log(f"{name}: {results[name].splitlines()[0]} ({time.perf_counter() - t0:.2f} s)")
        if results[name] != "ok":
            finish(3)                       # a failing rank ends the run
    comm.close()
    dist.destroy_process_group()
    with open(out_path, "w") as fh:
        json.dump(results, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main())
