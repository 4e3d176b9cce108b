#!/usr/bin/env python3
"""Record tests/golden/capi_pack_errors.json: return code and message of
every case of tests/test_capi_pack.py, from the checked-out library.

Run by hand (never by the suite), on a commit whose refusals are known good,
and only when a return code or message is meant to change:

    python tests/golden/make_capi_pack_errors.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mpi_grid_redistribute_amd import _lib  # noqa: E402
from tests.test_capi_pack import FIXTURE, record  # noqa: E402

if __name__ == "__main__":
    table = record(_lib.load())
    with open(FIXTURE, "w") as fh:   # one line per case
        fh.write("{\n" + ",\n".join(
            json.dumps(entry) + ": {\n" + ",\n".join(
                " " + json.dumps(case) + ": " + json.dumps(res) for case, res in cs.items()) + "\n}"
            for entry, cs in table.items()) + "\n}\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", sum(len(c) for c in table.values()), "cases")
