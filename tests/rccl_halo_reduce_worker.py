"""One rank of the multi-process halo return-path run
(tests/test_gpu_halo_reduce_multi.py): the halo exchange with
``return_route=True`` over RcclComm, values on the overload rows, and
``reduce_overload`` -- the reverse messages as RCCL groups between distinct
processes.  Pinned by global row ids as tests/test_gpu_halo_reduce.py: the
ranks gather each other's overload ids (gloo) and every rank checks its own
rows against ``np.add.at`` over all of them.

Environment as tests/rccl_return_worker.py: RANK, WORLD_SIZE, MASTER_ADDR,
MASTER_PORT, MGR_TEST_OUT, MGR_TEST_SHARED_GPU=1 when the ranks share GPU 0
(each rank then presents its own NCCL_HOSTID), MGR_CASE_TIMEOUT.  Every case
runs under a watchdog; the first failing case ends this rank (and, through the
barrier, the run).
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

TOPO = {2: [2, 1, 1], 4: [2, 2, 1]}
BOX = [1.0, 1.0, 1.0]
M = 1_000_000
ROWS = 10_000
CASE_TIMEOUT_S = float(os.environ.get("MGR_CASE_TIMEOUT", "60"))


def log(msg):
    print(f"[rank {RANK}/{WORLD} {time.strftime('%H:%M:%S')}] {msg}", flush=True)


def _vals(q, n, ncomp, dt, salt=0):
    j = np.arange(n, dtype=np.int64)
    v = ((q * 7 + j * 3 + salt)[:, None] + np.arange(ncomp)) % 11 - 5
    return v.astype(dt).reshape((n, ncomp) if ncomp > 1 else (n,))


def _gather(x):
    out = [None] * WORLD
    dist.all_gather_object(out, x)
    return out


def _expected_mine(n_own, all_ids, vals_of, local):
    """local + the values on every rank's rows whose id is one of this rank's
    n_own rows (id = RANK * M + row); also the contribution counts."""
    exp, cnt = local.copy(), np.zeros(n_own, dtype=np.int64)
    for q in range(WORLD):
        m = all_ids[q] // M == RANK
        np.add.at(exp, all_ids[q][m] % M, vals_of(q, len(all_ids[q]))[m])
        np.add.at(cnt, all_ids[q][m] % M, 1)
    return exp, cnt


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def case_direct(mgr, comm, empty):
    topo = TOPO[WORLD]
    R = mgr.MPIGridRedistributor(comm, topo, BOX)
    n = 0 if (empty and RANK == WORLD - 1) else ROWS
    rng = np.random.default_rng(500 + RANK)
    pos = (np.array(np.unravel_index(RANK, topo)) + rng.random((n, 3))) / np.asarray(topo)
    ids = np.arange(n, dtype=np.int64) + M * RANK
    hids, route = R.exchange_overload_by_position(ids, pos, [0.25 / t for t in topo],
                                                  return_route=True)
    assert route.n_local == n and route.n_halo == len(hids)
    all_h = _gather(hids)
    worst = 0
    for dt, nc, as_torch in ((np.float32, 3, True), (np.float64, 1, False), (np.int32, 1, True),
                             (np.int64, 3, False)):
        c = (lambda x: torch.from_numpy(x).cuda()) if as_torch else (lambda x: x)
        got = _np(R.reduce_overload(c(_vals(RANK, len(hids), nc, dt)), route,
                                    local_values=c(_vals(RANK, n, nc, dt, salt=1))))
        exp, cnt = _expected_mine(n, all_h, lambda q, k: _vals(q, k, nc, dt),
                                  _vals(RANK, n, nc, dt, salt=1))
        assert got.dtype == np.dtype(dt) and got.tobytes() == exp.tobytes(), (np.dtype(dt).name, nc)
        worst = max(worst, int(cnt.max()) if n else 0)
    assert max(_gather(worst)) >= 3, "no owner received a copy of a copy"
    route.release()
    torch.cuda.synchronize()


def case_all_the_way_home(mgr, comm):
    topo = TOPO[WORLD]
    R = mgr.MPIGridRedistributor(comm, topo, BOX)
    n = ROWS
    pos = np.random.default_rng(600 + RANK).uniform(-0.2, 1.2, (n, 3))
    ids = np.arange(n, dtype=np.int64) + M * RANK
    (lids, lpos), route = R.redistribute_by_position(ids, pos, return_positions=True,
                                                     return_route=True)
    hids, hroute = R.exchange_overload_by_position(lids, lpos, [0.25 / t for t in topo],
                                                   return_route=True)
    nl = len(lids)
    assert route.n_local == nl == hroute.n_local and route.n_source == n
    out = np.concatenate([lids, hids])
    all_out = _gather(out)
    v = torch.from_numpy(_vals(RANK, len(out), 3, np.float32)).cuda()
    back = _np(R.return_to_source(R.reduce_overload(v[nl:], hroute, local_values=v[:nl]), route))
    hroute.release()
    exp, cnt = _expected_mine(n, all_out, lambda q, k: _vals(q, k, 3, np.float32),
                              np.zeros((n, 3), np.float32))
    assert back.tobytes() == exp.tobytes()
    assert int(cnt.min()) >= 1 and max(_gather(int(cnt.max()))) >= 4
    route.release()
    torch.cuda.synchronize()


def case_one_call(mgr, comm):
    """redistribute_by_position(overload_lengths=, reduce_route=True), then
    return_to_source of n_local + n_halo values."""
    topo = TOPO[WORLD]
    R = mgr.MPIGridRedistributor(comm, topo, BOX)
    n = ROWS
    pos = np.random.default_rng(700 + RANK).uniform(-0.2, 1.2, (n, 3))
    ids = np.arange(n, dtype=np.int64) + M * RANK
    out, route = R.redistribute_by_position(ids, pos, overload_lengths=[0.25 / t for t in topo],
                                            reduce_route=True)
    assert route.n_local + route.n_halo == len(out) and route.n_source == n
    all_out = _gather(out)
    back = _np(R.return_to_source(torch.from_numpy(_vals(RANK, len(out), 3, np.float32)).cuda(),
                                  route))
    exp, cnt = _expected_mine(n, all_out, lambda q, k: _vals(q, k, 3, np.float32),
                              np.zeros((n, 3), np.float32))
    assert back.tobytes() == exp.tobytes()
    assert int(cnt.min()) >= 1 and max(_gather(int(cnt.max()))) >= 4
    route.release()
    assert route.halo.released
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
        ("direct", lambda: case_direct(mgr, comm, False)),
        ("one_call_form", lambda: case_one_call(mgr, comm)),
        ("all_the_way_home", lambda: case_all_the_way_home(mgr, comm)),
        ("direct_empty_rank", lambda: case_direct(mgr, comm, True)),
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
