"""Graph capture and replay of the device entry points (DESIGN.md, C ABI:
"stream-ordered, no allocation inside, no host sync, so graph-capturable").

Each chain of tests/stream_order.py is warmed up once, captured on one side
stream while its inputs hold the decoy A, and replayed twice: with the real
input B copied into the same buffers, then with A restored (the positions are
wrapped in place).  A host sync or an allocation inside an entry makes the
capture fail; a launcher that sized or routed its work from device data it read
on the host replays A's work on B's data.  The graphs are linear: one stream,
no fork or join.  Profiling stays off and no setting is touched.

The one-pass partition (mgr_partition_onepass_fields) is not among the chains:
its capture went through, but a replay ended in an illegal memory access whose
cause is not found yet; INTEGRATION.md does not promise capture for it."""
import pytest
import torch

from tests import stream_order as so

pytestmark = pytest.mark.gpu

CHAINS = ["two-pass", "fine-sort", "halo", "ghost"]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.mark.parametrize("name", CHAINS)
def test_chain_replays_on_new_inputs(name):
    pipe = so.PIPELINES[name]()
    run = so.Run(pipe)
    s = torch.cuda.Stream()
    run.load("A")
    torch.cuda.synchronize()
    run.enqueue(s)                      # eager warm-up
    s.synchronize()
    run.load("A")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run.enqueue(s)
    torch.cuda.synchronize()
    for which in ("B", "A"):
        run.clear()
        run.load(which)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        so.compare(run.read(), pipe.model(getattr(run, which)),
                   f"{name}: replay on input {which}")
