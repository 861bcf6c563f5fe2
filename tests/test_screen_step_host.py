"""The coarse screen's grouped chunk maxima (csrc/screen_kernels.hip), restated in numpy -- no GPU.

In the full chunks the coarse kernel takes one sample per group of CMG steps: the last row at the group's last column minus the
potential of its first.  T does not decrease along a row and the potential grows by hh per column, so the sample bounds
T(j) - pot(j) of every column of its group, and exceeds the best of them by at most (2 CMG - 1) hh."""
import numpy as np
import pytest

import screen_step_ref as ref

PARAMS = [-1.0, -1.0, -16.0, -16.0, 16.0, 0.0]          # open_h, ext_h, open_v, ext_v, dist_offset, dist_min (STRique's)


@pytest.mark.parametrize("cmg", [2, 4])
def test_grouped_samples_bound_the_per_column_rule(cmg):
    rng = np.random.default_rng(40 + cmg)
    sc, hh, v, merge = 512, 512, 16 * 512, 3
    k, n = 24, 5000
    looser = 0
    for trial in range(4):
        classes = rng.uniform(60, 120, k).astype(np.float32)
        vals = np.repeat(rng.uniform(50, 130, n), rng.integers(1, 9, n))[:n].astype(np.float32)          # runs of 1 .. 8 samples
        emb = np.repeat(classes, rng.integers(1, 9, k))
        p = int(rng.integers(500, n - 500 - len(emb)))
        vals[p:p + len(emb)] = emb
        T = ref.last_row(vals, classes, PARAMS, sc, hh, v, merge)
        assert np.all(np.diff(T) >= 0)                       # what the grouped rule rests on
        n_chunks = ((n + 1) // 2 + 63 + 63) // 64
        for lane in (0, (k - 1) // 5, 28, 32 + (k - 1) // 5, 60):
            per_column = ref.chunk_values(T, hh, lane, n_chunks)
            grouped = ref.chunk_values(T, hh, lane, n_chunks, cmg)
            assert np.all(grouped >= per_column), (trial, lane)
            assert np.all(grouped <= per_column + (2 * cmg - 1) * hh), (trial, lane)
            full = np.array([ref.is_full(c, n) for c in range(n_chunks)])
            assert np.array_equal(grouped[~full], per_column[~full])          # the predicated chunks keep the per-column rule
            looser += int((grouped[full] > per_column[full]).sum())
    assert looser > 0


def test_full_chunks_and_their_columns():
    """The full path starts at step 64 and needs 2 (t0s + 64) <= n: 256 columns is the shortest piece with a full chunk."""
    assert not ref.is_full(0, 10000)
    assert [ref.is_full(1, n) for n in (255, 256, 257)] == [False, True, True]
    assert [ref.is_full(2, n) for n in (383, 384, 385, 511)] == [False, True, True, True] and not ref.is_full(3, 511)
    # lane 60 (the last lane of flank B at 145 classes) in chunk 1 of a 256-column piece: columns 9 .. 136, all inside the piece
    assert ref.chunk_columns(1, 60, 256) == (9, 136)
    assert ref.chunk_columns(0, 28, 256) == (1, 72)
