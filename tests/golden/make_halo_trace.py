#!/usr/bin/env python3
"""Record tests/golden/halo_trace.json: the call sequence of
``halo.exchange_overload`` on the runs of tests/test_halo_trace_cpu.py, taken
from the checked-out code through that module's own wrappers.

Run by hand (never by the suite), on a commit whose sequence is known good,
and only when the sequence is meant to change:

    python tests/golden/make_halo_trace.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.test_halo_trace_cpu import FIXTURE, RUNS, key, record  # noqa: E402

if __name__ == "__main__":
    runs = {key(*run): record(*run) for run in RUNS}
    with open(FIXTURE, "w") as fh:   # one line per rank
        fh.write("{\n" + ",\n".join(
            json.dumps(k) + ": [\n" + ",\n".join(json.dumps(rank, separators=(",", ":"))
                                                 for rank in v) + "\n]"
            for k, v in runs.items()) + "\n}\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(runs), "runs")
