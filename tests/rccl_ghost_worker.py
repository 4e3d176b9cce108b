"""One rank of the multi-process ghost-cell run (tests/test_gpu_ghost_multi.py):
the halo exchange with ``unwrap=True`` over RcclComm, ``ghost_cell_sort``, the
one-call form, and the way back (``unsort``, ``reduce_overload``) -- between
distinct processes.  The checks are those of tests/test_gpu_ghost_halo.py,
whose brute-force model this worker imports: the ranks gather each other's
rows (gloo) and every rank checks its own copies.

Environment as tests/rccl_halo_reduce_worker.py: RANK, WORLD_SIZE, MASTER_ADDR,
MASTER_PORT, MGR_TEST_OUT, MGR_TEST_SHARED_GPU=1 when the ranks share GPU 0,
MGR_CASE_TIMEOUT.  Every case runs under a watchdog; the first failing case
ends this rank (and, through the barrier, the run).
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
CASE_TIMEOUT_S = float(os.environ.get("MGR_CASE_TIMEOUT", "60"))


def log(msg):
    print(f"[rank {RANK}/{WORLD} {time.strftime('%H:%M:%S')}] {msg}", flush=True)


def _gather(x):
    out = [None] * WORLD
    dist.all_gather_object(out, x)
    return out


def case_unwrap_and_sort(mgr, comm, frac, dt):
    from tests import test_gpu_ghost_halo as T
    topo = TOPO[WORLD]
    ol = T._ol(topo, frac)
    fine = [T.FINE] * 3
    R = mgr.MPIGridRedistributor(comm, topo, [1.0] * 3)
    ids, pos = T._local_rows(topo, RANK, T.ROWS, dt)
    h0, p0 = R.exchange_overload_by_position(ids, pos, ol, return_positions=True)
    h1, p1, hroute = R.exchange_overload_by_position(ids, pos, ol, return_positions=True,
                                                     unwrap=True, return_route=True)
    assert h1.tobytes() == h0.tobytes() and p1.shape == p0.shape
    all_ids, all_pos, all_h = _gather(ids), _gather(pos), _gather(h1)
    mi, mp = T._model_copies(topo, ol, RANK, np.concatenate(all_ids), np.concatenate(all_pos), dt)
    assert len(mi) == len(h1) > 0
    assert T._multiset(h1, p1) == T._multiset(mi, mp)
    if frac > 0.5:   # a row arrives twice; unwrapped, its copies differ
        m0, m1 = T._multiset(h0, p0), T._multiset(h1, p1)
        assert len(set(m0)) < len(m0) and len(set(m1)) == len(m1)
    nl = len(ids)
    both, bpos = np.concatenate([ids, h1]), np.concatenate([pos, p1])
    srt, spos, offs, sroute = R.ghost_cell_sort(both, bpos, nl, fine, ol, return_positions=True,
                                                return_route=True)
    cells, ghost, ext, interior = T._model_cells(topo, ol, RANK, bpos, nl)
    assert np.array_equal(interior, np.arange(len(both)) < nl)
    order = np.argsort(cells, kind="stable")
    assert np.array_equal(offs, np.concatenate(
        [[0], np.cumsum(np.bincount(cells, minlength=int(np.prod(ext))))]))
    assert srt.tobytes() == both[order].tobytes() and spos.tobytes() == bpos[order].tobytes()
    vals = R.unsort(T._val(srt, RANK), sroute)
    assert np.array_equal(vals, T._val(both, RANK))
    summed = R.reduce_overload(vals[nl:], hroute, local_values=vals[:nl])
    exp = T._val(ids, RANK).copy()
    for q in range(WORLD):
        m = all_h[q] // T.M == RANK
        np.add.at(exp, all_h[q][m] % T.M, T._val(all_h[q][m], q))
    assert np.array_equal(summed, exp)
    hroute.release()
    torch.cuda.synchronize()


def case_one_call(mgr, comm, frac, dt):
    from tests import test_gpu_ghost_halo as T
    topo = TOPO[WORLD]
    ol = T._ol(topo, frac)
    fine = [T.FINE] * 3
    R = mgr.MPIGridRedistributor(comm, topo, [1.0] * 3)
    pos = np.random.default_rng(900 + RANK).uniform(-0.2, 1.2, (T.ROWS, 3)).astype(dt)
    ids = np.arange(T.ROWS, dtype=np.int64) + T.M * RANK
    one = R.redistribute_by_position(ids, pos.copy(), overload_lengths=ol, fine_cells=fine,
                                     return_positions=True)
    lids, lpos = R.redistribute_by_position(ids, pos.copy(), return_positions=True)
    h, p = R.exchange_overload_by_position(lids, lpos, ol, return_positions=True, unwrap=True)
    comp = R.ghost_cell_sort(np.concatenate([lids, h]), np.concatenate([lpos, p]), len(lids),
                             fine, ol, return_positions=True)
    assert len(one) == len(comp) == 3 and len(h) > 0
    for a, b in zip(one, comp):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
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
        ("unwrap_sort_lt_half_f64", lambda: case_unwrap_and_sort(mgr, comm, 0.2, np.float64)),
        ("unwrap_sort_gt_half_f32", lambda: case_unwrap_and_sort(mgr, comm, 0.6, np.float32)),
        ("one_call_gt_half_f64", lambda: case_one_call(mgr, comm, 0.6, np.float64)),
        ("one_call_lt_half_f32", lambda: case_one_call(mgr, comm, 0.2, np.float32)),
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
