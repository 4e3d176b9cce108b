"""One rank of the multi-process run of the return path through the fine-cell
sort (tests/test_gpu_unsort_multi.py): redistribute with ``return_route=True``
over RcclComm, ``fine_cell_sort(..., return_route=True)`` on the received rows,
compute per-row values in sorted order, bring them back with
``return_to_source(..., sort_route=)``.  The ids pin the bijection, so every
check is this rank's own ids against what came back.

Environment, watchdog and result file as tests/rccl_return_worker.py.
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

from oracle import redist_oracle as ro  # noqa: E402
from tests import golden_io as G  # noqa: E402

TOPO = {2: [2, 1, 1], 4: [2, 2, 1]}
BOX = [1.0, 1.0, 1.0]
FINE = [8, 8, 8]
CASE_TIMEOUT_S = float(os.environ.get("MGR_CASE_TIMEOUT", "60"))


def log(msg):
    print(f"[rank {RANK}/{WORLD} {time.strftime('%H:%M:%S')}] {msg}", flush=True)


def _sizes():
    sizes = [int(np.random.default_rng(40 + r).integers(2000, 40_000)) for r in range(WORLD)]
    sizes[WORLD - 1] = 0                                   # an empty rank
    return sizes


def _values(ids):
    v1 = ids * 3 + 1
    v2 = np.stack([ids % 1000, ids % 77, -(ids % 13)], axis=1).astype(np.float32)
    v3 = (ids & 255).astype(np.uint8)
    return v1, v2, v3


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def case_recipe(mgr, comm, seed, as_torch, chunks):
    R = mgr.MPIGridRedistributor(comm, TOPO[WORLD], BOX)
    R.exchange_chunks = chunks
    n = _sizes()[RANK]
    rng = np.random.default_rng(seed + RANK)
    pos = rng.uniform(-0.5, 1.5, (n, 3))
    ids = np.arange(n, dtype=np.int64) + 1_000_000 * RANK
    conv = (lambda x: torch.from_numpy(x).cuda()) if as_torch else (lambda x: x)
    (lids, lpos), route = R.redistribute_by_position(conv(ids.copy()), conv(pos.copy()),
                                                     return_positions=True, return_route=True)
    (sids, spos), offsets, sroute = R.fine_cell_sort((lids, lpos), lpos, FINE, return_route=True)
    assert sroute.n == route.n_local
    cells = ro.fine_cell_ids(TOPO[WORLD], FINE, BOX, _np(spos))
    assert (np.diff(cells) >= 0).all(), "not sorted"
    back = R.return_to_source(tuple(conv(v) for v in _values(_np(sids))), route,
                              sort_route=sroute)
    for b, w in zip(back, _values(ids)):
        assert G.same_bytes(_np(b), w), "values"
    wrapped = ((pos % 1.0) + 1.0) % 1.0
    bpos = R.return_to_source(spos, route, sort_route=sroute)
    assert G.same_bytes(_np(bpos), wrapped), "positions"
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
        ("recipe_empty_rank", lambda: case_recipe(mgr, comm, 91, False, 1)),
        ("recipe_pipelined_forward", lambda: case_recipe(mgr, comm, 92, True, 4)),
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
