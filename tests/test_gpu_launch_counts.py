"""Launches per kernel of every entry point that goes through the shared
bin / scan / pack / unpack stages (_stage.py), pinned to a table recorded
from the commit before the split of redistributor.py (5b5def7): the Python
that drives libmgr.so may be rearranged, the kernels it launches per call may
not change.  Counted by the library's profiler (_lib.profile_*, one count per
launch and profiler kernel name); one rank (SelfComm), 3000 rows -- several
tiles with a ragged last one.

Recording (prints the table as a dict, on a GPU):
    python -m tests.test_gpu_launch_counts
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

mgr = pytest.importorskip("mpi_grid_redistribute_amd")
from mpi_grid_redistribute_amd import GridPartitioner, MPIGridRedistributor, _lib  # noqa: E402

N = 3000
FINE = [8, 8, 8]        # 512 fine cells: the ranked sort
FINE_BIG = [16] * 3     # 4096: the counted sort
GFINE, OL = [4, 4, 4], [0.05] * 3   # ghost grid 6^3 = 216 cells


def _u8(t):
    return t.view(torch.uint8).reshape(-1)


class _In:
    """Fresh inputs of one case: 36-byte records with their f32 positions
    inside, and the same values as the SoA set (pos, vel, mass, id)."""

    def __init__(self):
        self.rec, self.pos = mgr.synth_wide(N, seed=11, lo=-0.25, hi=1.25)
        self.soa = mgr.synth_wide_soa(N, seed=11, lo=-0.25, hi=1.25)
        self.rbs = [12, 12, 4, 8]

    def flats(self):
        return [_u8(t) for t in self.soa]

    def half(self):
        """f16 positions and records without them: no one-pass shape."""
        return self.rec.clone(), self.pos.to(torch.float16)


def _part():
    return GridPartitioner([2, 2, 2], [1.0] * 3)


def _red():
    return MPIGridRedistributor(None, [1, 1, 1], [1.0] * 3)


def _soa_onepass():
    P = _part()
    P.soa_onepass = True
    return P


def _local(soa=False):
    """A redistributor and its redistributed rows with their wrapped positions."""
    R, i = _red(), _In()
    if soa:
        return (R,) + R.redistribute_by_position(i.soa, i.soa[0], return_positions=True)
    return (R,) + R.redistribute_by_position(i.rec, i.pos, return_positions=True)


def _vals(n):
    return (torch.arange(n, dtype=torch.float32, device="cuda"),
            torch.arange(3 * n, dtype=torch.int64, device="cuda").reshape(n, 3))


# name -> (setup, call): setup() runs uncounted and returns the arguments of call
def _c_route(**kw):
    def setup():
        R, i = _red(), _In()
        res, route = R.redistribute_by_position(i.rec, i.pos, return_route=True, **kw)
        return R, res, route
    return setup


def _c_sorted_route():
    R, i = _red(), _In()
    (data, pos), route = R.redistribute_by_position(i.rec, i.pos, return_positions=True,
                                                    return_route=True)
    _, _, sroute = R.fine_cell_sort(data, pos, FINE, return_route=True)
    return R, route, sroute


def _c_sort_route(fine):
    def setup():
        R, data, pos = _local()
        _, _, sroute = R.fine_cell_sort(data, pos, fine, return_route=True)
        return R, sroute
    return setup


def _c_reduce_route():
    R, i = _red(), _In()
    res, route = R.redistribute_by_position(i.rec, i.pos, overload_lengths=OL, reduce_route=True)
    return R, route


def _c_drop_route():
    R, i = _red(), _In()
    ids = torch.arange(N, device="cuda") % 3 - 1        # -1 and 1 are dropped
    res, route = R.redistribute_by_cell_number(i.soa, ids, return_route=True)
    return R, route


CASES = {
    # ------------------------------------------------------ GridPartitioner
    "partition_device": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_device(_u8(i.rec), 36, i.pos)),
    "partition_device_fine": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_device(_u8(i.rec), 36, i.pos, fine_cells=FINE)),
    "partition_fields_device": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_fields_device(i.flats(), i.rbs, i.soa[0])),
    "partition_fields_device_fine": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_fields_device(i.flats(), i.rbs, i.soa[0], fine_cells=FINE)),
    "unpartition_fields_device": (
        lambda: (lambda P, i: (P, i, P.partition_fields_device(i.flats(), i.rbs, i.soa[0])))(
            _part(), _In()),
        lambda P, i, _: P.unpartition_fields_device(i.flats(), i.rbs)),
    "partition_by_position": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_by_position(i.rec, i.pos)),
    "partition_by_position_soa": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_by_position(i.soa, i.soa[0])),
    "partition_by_position_numpy": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_by_position(i.rec.cpu().numpy(),
                                             i.pos.contiguous().cpu().numpy())),
    "partition_lists_onepass": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_lists(i.rec, i.pos)),
    "partition_lists_onepass_fine": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_lists(i.rec, i.pos, fine_cells=FINE)),
    "partition_lists_soa_onepass": (
        lambda: (_soa_onepass(), _In()),
        lambda P, i: P.partition_lists(i.soa, i.soa[0])),
    "partition_lists_soa_onepass_fine": (
        lambda: (_soa_onepass(), _In()),
        lambda P, i: P.partition_lists(i.soa, i.soa[0], fine_cells=FINE)),
    "partition_lists_soa_default": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_lists(i.soa, i.soa[0])),
    "partition_lists_twopass_f16": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_lists(*i.half())),
    "partition_lists_twopass_f16_fine": (
        lambda: (_part(), _In()),
        lambda P, i: P.partition_lists(*i.half(), fine_cells=FINE)),
    "partition_lists_soa_twopass_f16": (
        lambda: (_soa_onepass(), _In()),
        lambda P, i: P.partition_lists(i.soa[1:], i.half()[1])),
    # ------------------------------------------------- MPIGridRedistributor
    "redistribute": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos)),
    "redistribute_soa": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.soa, i.soa[0])),
    "redistribute_numpy": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec.cpu().numpy(),
                                                i.pos.contiguous().cpu().numpy())),
    "redistribute_positions": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, return_positions=True)),
    "redistribute_route": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, return_route=True)),
    "redistribute_fine": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, fine_cells=FINE)),
    "redistribute_fine_soa_positions": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.soa[1:], i.soa[0], fine_cells=FINE,
                                                return_positions=True)),
    "redistribute_halo": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, overload_lengths=OL)),
    "redistribute_halo_positions_reduce_route": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, overload_lengths=OL,
                                                return_positions=True, reduce_route=True)),
    "redistribute_halo_fine": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_position(i.rec, i.pos, overload_lengths=OL,
                                                fine_cells=GFINE)),
    "redistribute_by_cell_number": (
        lambda: (_red(), _In()),
        lambda R, i: R.redistribute_by_cell_number(
            i.rec, torch.arange(N, device="cuda") % 3 - 1)),
    "fine_cell_sort": (
        _local, lambda R, d, p: R.fine_cell_sort(d, p, FINE)),
    "fine_cell_sort_route": (
        _local, lambda R, d, p: R.fine_cell_sort(d, p, FINE, return_route=True)),
    "fine_cell_sort_positions_counted": (
        _local, lambda R, d, p: R.fine_cell_sort(d, p, FINE_BIG, return_positions=True)),
    "fine_cell_sort_counted_route": (
        _local, lambda R, d, p: R.fine_cell_sort(d, p, FINE_BIG, return_route=True)),
    "fine_cell_sort_soa_ids": (
        lambda: _local(soa=True),
        lambda R, d, p: R.fine_cell_sort(
            d, p, FINE, fine_ids=(torch.arange(N, device="cuda") % 512).to(torch.int16))),
    "ghost_cell_sort": (
        _local, lambda R, d, p: R.ghost_cell_sort(d, p, N, GFINE, OL)),
    "ghost_cell_sort_positions_route": (
        _local, lambda R, d, p: R.ghost_cell_sort(d, p, N, GFINE, OL, return_positions=True,
                                                     return_route=True)),
    "unsort": (
        _c_sort_route(FINE), lambda R, s: R.unsort(_vals(N), s)),
    "unsort_counted": (
        _c_sort_route(FINE_BIG), lambda R, s: R.unsort(_vals(N)[0], s)),
    "return_to_source": (
        _c_route(), lambda R, res, route: R.return_to_source(_vals(N), route)),
    "return_to_source_dropped": (
        _c_drop_route, lambda R, route: R.return_to_source(_vals(route.n_local)[1], route)),
    "return_to_source_sort_route": (
        _c_sorted_route, lambda R, route, s: R.return_to_source(_vals(N), route, sort_route=s)),
    "return_to_source_halo": (
        _c_reduce_route,
        lambda R, route: R.return_to_source(_vals(route.n_local + route.n_halo)[0], route)),
}


def _count(name):
    """{profiler kernel: launches} of the case's call (kernels never launched
    are left out)."""
    setup, call = CASES[name]
    args = setup()
    torch.cuda.synchronize()
    _lib.profile_select(None)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        call(*args)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    got = {k: _lib.profile_read(k)[1] for k in _lib.PROFILE_KERNELS}
    _lib.profile_reset()
    return {k: int(c) for k, c in got.items() if c}


# Recorded at 5b5def7 (python -m tests.test_gpu_launch_counts on an MI355X).
EXPECTED = {'fine_cell_sort': {'bin_fine': 1, 'count_ids': 1, 'pack_fine': 1, 'scan': 1},
 'fine_cell_sort_counted_route': {'bin_fine': 1, 'count_ids': 1, 'pack': 1, 'scan': 1},
 'fine_cell_sort_positions_counted': {'bin_fine': 1, 'count_ids': 1, 'pack': 2, 'scan': 1},
 'fine_cell_sort_route': {'bin_fine': 1, 'count_ids': 1, 'pack_fine': 1, 'scan': 1},
 'fine_cell_sort_soa_ids': {'count_ids': 1, 'pack_fine': 4, 'scan': 1},
 'ghost_cell_sort': {'count_ids': 1, 'pack_fine': 1, 'scan': 1},
 'ghost_cell_sort_positions_route': {'count_ids': 1, 'pack_fine': 2, 'scan': 1},
 'partition_by_position': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_by_position_numpy': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_by_position_soa': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_device': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_device_fine': {'bin_fine': 1, 'pack': 1, 'scan': 1},
 'partition_fields_device': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_fields_device_fine': {'bin_fine': 1, 'pack': 1, 'scan': 1},
 'partition_lists_onepass': {'onepass': 1},
 'partition_lists_onepass_fine': {'onepass': 1},
 'partition_lists_soa_default': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_lists_soa_onepass': {'onepass_fields': 1},
 'partition_lists_soa_onepass_fine': {'onepass_fields': 1},
 'partition_lists_soa_twopass_f16': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_lists_twopass_f16': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'partition_lists_twopass_f16_fine': {'bin_fine': 1, 'pack': 1, 'scan': 1},
 'redistribute': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'redistribute_by_cell_number': {'bin_ids': 1, 'pack': 1, 'scan': 1},
 'redistribute_fine': {'bin_fine': 1, 'count_ids': 1, 'pack': 1, 'pack_fine': 1, 'scan': 2},
 'redistribute_fine_soa_positions': {'bin_fine': 1,
                                     'count_ids': 1,
                                     'pack': 1,
                                     'pack_fine': 4,
                                     'scan': 2},
 'redistribute_halo': {'bin_count': 1, 'halo': 1, 'halo_pack': 1, 'pack': 1, 'scan': 2},
 'redistribute_halo_fine': {'bin_count': 1,
                            'count_ids': 1,
                            'halo': 1,
                            'halo_pack': 1,
                            'pack': 1,
                            'pack_fine': 1,
                            'scan': 3},
 'redistribute_halo_positions_reduce_route': {'bin_count': 1,
                                              'halo': 1,
                                              'halo_pack': 1,
                                              'pack': 1,
                                              'scan': 2},
 'redistribute_numpy': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'redistribute_positions': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'redistribute_route': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'redistribute_soa': {'bin_count': 1, 'pack': 1, 'scan': 1},
 'return_to_source': {'unpack': 1},
 'return_to_source_dropped': {'unpack': 1},
 'return_to_source_halo': {'unpack': 1},
 'return_to_source_sort_route': {'unpack': 1, 'unpack_ranked': 1},
 'unpartition_fields_device': {'unpack': 1},
 'unsort': {'unpack_ranked': 1},
 'unsort_counted': {'unpack': 1}}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def test_table_covers_every_case():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_counts(name):
    got = _count(name)
    print(name, got)
    assert got == EXPECTED[name]


def test_partitioner_fine_cells_length_checked():
    """fine_cells shorter than the grid's dimensions: refused before the
    native plan reads dim entries from it (both entry points)."""
    P = _part()
    rec, pos = mgr.synth_wide(64, seed=3)
    with pytest.raises(ValueError, match="fine_cells must have 3 entries"):
        P.partition_lists(rec, pos, fine_cells=[8, 8])
    with pytest.raises(ValueError, match="fine_cells must have 3 entries"):
        P.partition_device(_u8(rec), 36, pos, fine_cells=[8, 8])


if __name__ == "__main__":
    import pprint
    table = {name: _count(name) for name in sorted(CASES)}
    print("EXPECTED = ", end="")
    pprint.pprint(table, width=100, sort_dicts=True)
