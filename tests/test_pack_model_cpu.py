"""The numpy pack model (tests/pack_model.py) checked on the CPU before the
kernel tests trust it: against the C oracle's stable partition, and against
its own tile-range algebra (chunks compose, chunks are disjoint, the tile
offsets bracket every chunk's slots)."""
import numpy as np
import pytest

from oracle import c_oracle
from tests.pack_model import bin_layout, pack_model, tile_offsets_model

SENT = 0xAB


def _case(n, nbins, row_bytes, seed, empty=()):
    rng = np.random.default_rng(seed)
    live = [b for b in range(nbins) if b not in empty] or [0]
    dest = rng.choice(np.asarray(live, dtype=np.int64), size=n)
    rows = rng.integers(0, 256, size=(n, row_bytes), dtype=np.uint8)
    ids = rng.integers(0, 1 << 16, size=n, dtype=np.uint16)
    return dest, rows, ids


@pytest.mark.parametrize("n", [0, 1, 63, 64, 1000])
@pytest.mark.parametrize("nbins,row_bytes,empty", [
    (1, 3, ()), (2, 6, ()), (9, 36, (4,)), (9, 8, (0, 8)), (64, 2, (1, 2, 3)), (300, 12, (299,)),
    (1100, 100, ())])
def test_model_equals_c_oracle(n, nbins, row_bytes, empty):
    dest, rows, ids = _case(n, nbins, row_bytes, 1000 * nbins + n, empty)
    want, offsets = c_oracle.partition(rows, dest, nbins)
    m = pack_model([rows, ids], dest, nbins, tile_rows=64, ids=ids, sentinel=SENT)
    assert np.array_equal(m.bin_start, offsets)
    assert np.array_equal(m.dst[0], want.reshape(n, row_bytes))
    # the ids as a field and as the side field move alike, and with the rows
    want_ids, _ = c_oracle.partition(ids, dest, nbins)
    assert np.array_equal(m.dst[1].view(np.uint16).reshape(-1), want_ids)
    assert np.array_equal(m.ids_dst, m.dst[1])
    assert m.dst_written.all() and m.red[0].shape == (0, row_bytes)


@pytest.mark.parametrize("redirect_bin", [-1, 0, 4, 8])
@pytest.mark.parametrize("drop_bin", [-1, 9])
def test_redirect_and_drop_layout(redirect_bin, drop_bin):
    """dst = the kept, non-redirected bins back to back; red = the redirect bin."""
    n, nbins = 777, 10 if drop_bin >= 0 else 9
    dest, rows, ids = _case(n, nbins, 12, 6 + redirect_bin, empty=(2,))
    m = pack_model([rows], dest, nbins, drop_bin, redirect_bin, 64, ids=ids, sentinel=SENT)
    keep = [b for b in range(nbins) if b not in (drop_bin, redirect_bin)]
    want = np.concatenate([rows[dest == b] for b in keep])
    assert np.array_equal(m.dst[0][:len(want)], want)
    assert (m.dst[0][len(want):] == SENT).all()
    assert np.array_equal(m.dst_written, np.arange(n) < len(want))
    if redirect_bin >= 0:
        assert np.array_equal(m.red[0], rows[dest == redirect_bin])
        assert np.array_equal(m.ids_red.view(np.uint16).reshape(-1), ids[dest == redirect_bin])
        assert m.red_written.all()
    else:
        assert m.red[0].shape[0] == 0


def _splits(T):
    yield [T * c // 4 for c in range(5)]
    yield [0, 0, 1, max(1, T - 2), T]           # an empty chunk and a one-tile chunk
    yield list(range(T + 1))                    # every tile its own chunk
    yield [0, T]


@pytest.mark.parametrize("n,tile_rows", [(1, 64), (63, 64), (64, 64), (5 * 64 + 37, 64),
                                         (5 * 512 + 37, 512)])
@pytest.mark.parametrize("redirect_bin,drop_bin", [(-1, -1), (0, 9), (4, -1), (8, 9)])
def test_chunks_compose_and_offsets_bracket(n, tile_rows, redirect_bin, drop_bin):
    nbins = 10 if drop_bin >= 0 else 9
    dest, rows, ids = _case(n, nbins, 6, n + 7 * (redirect_bin + 1), empty=(3,))
    T = (n + tile_rows - 1) // tile_rows
    whole = pack_model([rows], dest, nbins, drop_bin, redirect_bin, tile_rows, ids=ids,
                       sentinel=SENT)
    counts, bin_start, _ = bin_layout(dest, nbins)
    for bounds in _splits(T):
        offs = tile_offsets_model(dest, nbins, tile_rows, bounds)
        assert np.array_equal(offs[0], bin_start[:nbins])
        assert np.array_equal(offs[-1], bin_start[1:])
        acc = None
        seen_d = np.zeros(n, dtype=bool)
        seen_r = np.zeros(whole.red[0].shape[0], dtype=bool)
        for c in reversed(range(len(bounds) - 1)):
            m = pack_model([rows], dest, nbins, drop_bin, redirect_bin, tile_rows, bounds[c],
                           bounds[c + 1], ids=ids, sentinel=SENT)
            assert not (m.dst_written & seen_d).any() and not (m.red_written & seen_r).any()
            seen_d |= m.dst_written
            seen_r |= m.red_written
            # the chunk's slots, bin by bin, are exactly [offs[c][b], offs[c+1][b])
            want_d = np.zeros(n, dtype=bool)
            want_r = np.zeros(len(seen_r), dtype=bool)
            gap = counts[redirect_bin] if redirect_bin >= 0 else 0
            for b in range(nbins):
                lo, hi = offs[c][b], offs[c + 1][b]
                if b == drop_bin:
                    continue
                if b == redirect_bin:
                    want_r[lo - bin_start[b]:hi - bin_start[b]] = True
                else:
                    shift = gap if (redirect_bin >= 0 and b > redirect_bin) else 0
                    want_d[lo - shift:hi - shift] = True
            assert np.array_equal(m.dst_written, want_d)
            assert np.array_equal(m.red_written, want_r)
            acc = m.over(acc)
        for (name, a), (_, w) in zip(acc.buffers(), whole.buffers()):
            assert np.array_equal(a, w), name
        assert np.array_equal(acc.dst_written, whole.dst_written)
        assert np.array_equal(acc.red_written, whole.red_written)


def test_tile_offsets_model_repeats_and_order():
    dest, _, _ = _case(1000, 5, 1, 3)
    offs = tile_offsets_model(dest, 5, 64, [16, 0, 3, 3, 16])
    assert np.array_equal(offs[0], offs[4]) and np.array_equal(offs[2], offs[3])
    assert np.array_equal(offs[2] - offs[1], np.bincount(dest[:192], minlength=5))


def test_model_refuses_bad_destinations():
    with pytest.raises(ValueError):
        pack_model([np.zeros((3, 4), np.uint8)], [0, 1, 5], 5)
