"""CPU tests of tests/_bucket_ref.py, the numpy restatement of the FAST corner buckets the GPU tests compare against
(tests/test_gpu_buckets.py): the properties the contract in include/svo_abi.h states, on oracle.fast corners."""
import numpy as np
import pytest

from _bucket_ref import bucket, bucket_cells
from conftest import rand_image
from test_gpu_keep_strongest import _strongest

GRIDS = [(16, 16), (40, 24), (7, 5), (1, 1), (1000, 1000)]


@pytest.fixture(scope="module")
def lists(oracle, small_seq):
    out = []
    for seed, (h, w) in enumerate([(64, 80), (97, 131), (128, 416)]):
        out.append((oracle.fast(rand_image(h, w, 20 + seed)), w, h))
    _, frames = small_seq
    for L, _R in frames[:2]:
        out.append((oracle.fast(L), L.shape[1], L.shape[0]))
    assert all(len(k) > 100 for k, _, _ in out)
    return out


def _is_raster_sublist(sub, full):
    """every record of `sub` is a record of `full`, in the same order"""
    key = lambda k: k["y"].astype(np.int64) * 100000 + k["x"].astype(np.int64)
    ks, kf = key(sub), key(full)
    assert np.all(np.diff(ks) > 0)
    pos = np.searchsorted(kf, ks)
    return bool(np.all(pos < len(kf)) and full[pos].tobytes() == sub.tobytes())


@pytest.mark.parametrize("cw,ch", GRIDS)
@pytest.mark.parametrize("k", [1, 2, 5])
def test_bucket_properties(lists, cw, ch, k):
    cut_seen = False
    for kps, w, h in lists:
        got = bucket(kps, w, h, cw, ch, k)
        assert _is_raster_sublist(got, kps)
        cells, cells_got = bucket_cells(kps, w, cw, ch), bucket_cells(got, w, cw, ch)
        pop = np.bincount(cells)
        pop_got = np.bincount(cells_got, minlength=len(pop))
        assert np.array_equal(pop_got, np.minimum(pop, k))        # at most k per cell; a cell with <= k corners loses none
        cut_seen |= bool(np.any(pop > k))
        # what a cell drops is never stronger than what it keeps
        for c in np.flatnonzero(pop > k)[:50]:
            kept = got["response"][cells_got == c]
            allr = np.sort(kps["response"][cells == c])[::-1]
            assert np.array_equal(np.sort(kept)[::-1], allr[:k])
        assert bucket(got, w, h, cw, ch, k).tobytes() == got.tobytes()          # idempotent
        nxt = bucket(kps, w, h, cw, ch, k + 1)
        assert _is_raster_sublist(got, nxt)                                      # survivors at k are survivors at k + 1
    assert cut_seen or (cw, ch) == (1, 1) or k > 1        # (3x3 NMS: a 7 x 5 cell seldom holds more than 4 corners)


@pytest.mark.parametrize("k", [1, 31, 150, 100000])
def test_one_cell_is_keep_strongest(lists, k):
    for kps, w, h in lists:
        assert bucket(kps, w, h, w, h, k).tobytes() == _strongest(kps, k).tobytes()
        assert bucket(kps, w, h, 16384, 16384, k).tobytes() == _strongest(kps, k).tobytes()


def test_ties_go_to_raster_order_and_empty_list():
    kp = np.zeros(6, dtype=[("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                            ("octave", "<i4"), ("class_id", "<i4")])
    kp["x"] = [1, 3, 9, 2, 8, 3]
    kp["y"] = [0, 0, 0, 1, 1, 2]
    kp["response"] = [5, 5, 7, 5, 7, 9]
    got = bucket(kp, 16, 4, 8, 4, 2)                 # cells: x < 8 -> 0 (responses 5, 5, 5, 9), else 1 (7, 7)
    assert got["x"].tolist() == [1, 9, 8, 3] and got["y"].tolist() == [0, 0, 1, 2]
    assert len(bucket(kp[:0], 16, 4, 8, 4, 2)) == 0
