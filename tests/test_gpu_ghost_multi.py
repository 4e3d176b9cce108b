"""Ghost-cell lists between processes over the product transport (RcclComm):
world 2 ([2,1,1], where a row arrives twice) and 4 ([2,2,1]), one process per
rank (tests/rccl_ghost_worker.py): the halo with ``unwrap=True`` against the
brute-force model of tests/test_gpu_ghost_halo.py, ``ghost_cell_sort`` against
a numpy stable argsort, ``unsort`` + ``reduce_overload`` on the way back, and
the one-call form against the composed one -- all in one worker run per world.
With fewer GPUs than ranks all ranks share GPU 0, each with its own
NCCL_HOSTID (RCCL's socket transport), as tests/test_gpu_return_multi.py.
"""
import json
import os
import signal
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = int(os.environ.get("MGR_MULTI_TIMEOUT", "300"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 4])
def test_rccl_ghost(world, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    shared = torch.cuda.device_count() < world
    port = _free_port()
    procs, logs = [], []
    for r in range(world):        # at most 4 GPU processes at once
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   MGR_TEST_OUT=str(tmp_path / f"rank{r}.json"),
                   MGR_TEST_SHARED_GPU="1" if shared else "0")
        logs.append(open(tmp_path / f"ghost_w{world}_rank{r}.log", "w"))
        procs.append(subprocess.Popen([sys.executable, "-u", "-m",
                                       "tests.rccl_ghost_worker"], cwd=ROOT, env=env,
                                      start_new_session=True, stdout=logs[-1],
                                      stderr=subprocess.STDOUT))
    codes = []
    try:
        for p in procs:
            codes.append(p.wait(timeout=TIMEOUT_S))
    except subprocess.TimeoutExpired:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
        for p in procs:
            p.wait()
        pytest.fail(f"world {world}: ranks did not finish within {TIMEOUT_S} s")
    finally:
        for fh in logs:
            fh.close()
    failures = {}
    for r in range(world):
        path = tmp_path / f"rank{r}.json"
        tail = (tmp_path / f"ghost_w{world}_rank{r}.log").read_text()[-2000:]
        assert path.exists(), f"rank {r} exited {codes[r]} without results\n{tail}"
        res = json.loads(path.read_text())
        assert res, f"rank {r}: no cases ran"
        failures.update({f"rank{r}:{k}": v for k, v in res.items() if v != "ok"})
    assert not failures, "\n".join(f"{k}: {v}" for k, v in failures.items())
    assert all(c == 0 for c in codes), codes
