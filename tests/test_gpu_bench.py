"""GPU: bench.py's JSON line keeps the driver's contract (metric, value,
unit, steps, roofline with achieved / peak / frac / traffic, config
workload ...) -- run as a child process on a small config-2 input."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


N_SMALL = (1 << 20) + 37      # odd, many tiles, 65536 sampled rows of ~1M


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--particles", str(N_SMALL), "--steps", "2", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump"))
    return _bench("--dump-outputs", d), d


def test_plain_run_is_lean(plain_run):
    """Without --full the line keeps its headline keys and the kernels timed
    inside the region; everything that takes a run of its own is null."""
    rec, _ = plain_run
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["dtype"] == "f64"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["unit"] == "particles/s"
    assert abs(rec["value"] - N_SMALL / (rec["ms_per_step"] / 1e3)) / rec["value"] < 1e-6
    for k in ("cpu_baseline", "cpu_baseline_cfg1", "cpu_baseline_c", "count_skew", "onepass",
              "xgmi", "rccl", "exchange_ab", "n1_same_workload_ms"):
        assert rec[k] is None, k
    assert rec["kernels"] and all(e["in_timed_region"] for e in rec["kernels"].values())
    assert rec["roofline"]["kernel"] == "pack"


def test_dump_outputs_are_the_partition(plain_run):
    """--dump-outputs: the sampled send buffer is the stable partition of the
    seeded input (rows in bin order, ids ascending inside a bin, every record
    carrying its wrapped position), the counts sum to n."""
    import numpy as np

    _, d = plain_run
    assert sorted(os.listdir(d)) == ["bin_counts.npy", "position.npy", "send_records.npy"]
    cnt = np.load(os.path.join(d, "bin_counts.npy"))
    rec = np.load(os.path.join(d, "send_records.npy"))
    pos = np.load(os.path.join(d, "position.npy"))
    assert cnt.dtype == rec.dtype == pos.dtype == np.float64
    assert cnt.shape == (8,) and cnt.sum() == N_SMALL and cnt.min() > 0
    assert rec.ndim == 2 and rec.shape[1] == 4 and 60000 < len(rec) <= 65536
    assert pos.shape == (len(rec), 3) and (pos >= 0).all() and (pos < 1).all()
    xyz, ids = rec[:, :3], rec[:, 3]
    assert (xyz >= 0).all() and (xyz < 1).all()
    from oracle import redist_oracle as ro                  # checker only
    cell = ro.cell_number_from_position(ro.Geometry([2, 2, 2], [1.0, 1.0, 1.0], 8), xyz.copy())
    assert np.array_equal(np.bincount(cell, minlength=8) > 0, cnt > 0)
    assert (np.diff(cell) >= 0).all()                       # bins laid end to end
    same = np.diff(cell) == 0
    assert (np.diff(ids)[same] > 0).all()                   # stable inside a bin
    assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < N_SMALL
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) < 64 << 20


def test_dump_outputs_repeat(plain_run, tmp_path):
    """The same arguments give the same inputs, the same sample, the same arrays."""
    import numpy as np

    _, d = plain_run
    _bench("--dump-outputs", str(tmp_path))
    for f in os.listdir(d):
        assert np.array_equal(np.load(os.path.join(d, f)), np.load(str(tmp_path / f))), f


def test_full_run_keeps_the_rest():
    """--full: the detail pass (kernels timed outside the region), the count
    skew and, unless --no-cpu-baseline, the CPU baselines."""
    rec = _bench("--full", "--no-cpu-baseline")
    assert rec["count_skew"] is not None and rec["cpu_baseline"] is None
    outside = [k for k, e in rec["kernels"].items() if not e["in_timed_region"]]
    assert "bin_count" in outside and "scan" in outside and "pack" in rec["kernels"]


def test_bench_line_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--particles", "4194304",
                        "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    rec = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["higher_is_better"] is True and rec["unit"] == "particles/s"
    assert abs(rec["value"] - 4194304 / (rec["ms_per_step"] / 1e3)) / rec["value"] < 1e-6
    assert rec["config"]["workload"].startswith("cfg2_")
    rl = rec["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(rl)
    assert rl["bound"] == "hbm" and rl["unit"] == "GB/s" and rl["peak"] == 8000.0
    assert abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-9
