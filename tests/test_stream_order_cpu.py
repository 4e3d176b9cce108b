"""The two properties the GPU stream-order and graph-replay tests rest on,
from the numpy models alone (tests/stream_order.py): for every pipeline's
decoy input A and real input B

  * model(A) != model(B) in every compared output -- else a result computed
    from the decoy could pass for the real one;
  * both inputs are in contract (ids and cells in range, sorted ids sorted),
    and every bin and every set holds rows in B.

Host-only calls of the library (tile sizes) size the inputs; no GPU."""
import numpy as np
import pytest

from tests import stream_order as so


@pytest.mark.parametrize("name", list(so.PIPELINES))
def test_models_tell_the_inputs_apart(name):
    pipe = so.PIPELINES[name]()
    a, b = pipe.inputs("A"), pipe.inputs("B")
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    ma, mb = pipe.model(a), pipe.model(b)
    assert sorted(ma) == sorted(mb)
    assert so.same_outputs(pipe, ma, mb) == []
    for k in pipe.constant:
        assert np.asarray(ma[k]).tobytes() == np.asarray(mb[k]).tobytes(), k
    # the models leave their inputs alone: a second evaluation agrees
    assert set(so.differs(ma, pipe.model(a))) == set(ma)


@pytest.mark.parametrize("name", list(so.PIPELINES))
def test_inputs_are_in_contract(name):
    pipe = so.PIPELINES[name]()
    for which in ("A", "B"):
        pipe.check_contract(pipe.inputs(which))
    counts = np.asarray(pipe.sets_nonempty(pipe.inputs("B")))
    assert counts.size and (counts > 0).all(), counts
    assert pipe.n % 64 != 0 and pipe.n > 3 * 64      # a ragged last round, several tiles


def test_synth_decoy_differs_from_the_generator():
    pos, rec = so.synth_model(so.SYNTH_N)
    assert not (pos == so.SYNTH_DECOY_VALUE).any()
    assert pos.shape == (so.SYNTH_N, 3) and rec.shape == (so.SYNTH_N, 32)
