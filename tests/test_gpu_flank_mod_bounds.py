"""flank_mod_bounds_kernel on its own (strq_debug_flank_mod_bounds) against the plain-Python bounds of strique_amd/flank_mod.py: the
hand-written paths of tests/flank_mod_ref.py, stretch lengths around the lane stride (63, 64, 65, 129), 64 groups in one
flank, the first and the last column of the profile as a group's range, more stretches than one workgroup has waves, the decode
status.  Every record is compared exactly."""
import numpy as np
import pytest

from flank_mod_ref import HAND_COLUMN_OF as COLUMN_OF, HAND_PATHS as HAND

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    c = ffi.Context(0)
    yield c
    c.close()


def _want(paths, column_of, groups, status=None):
    from strique_amd import flank_mod
    return [np.array(flank_mod.bounds(None if status is not None and status[f] else p, column_of, g), np.int32).reshape(-1, 3)
            for f, (p, g) in enumerate(zip(paths, groups))]


def _check(ctx, paths, column_of, groups, status=None):
    got = ctx.debug_flank_mod_bounds(paths, column_of, groups, status)
    want = _want(paths, column_of, groups, status)
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and np.array_equal(g, w), (f, g, w)
    return got


def test_hand_written_paths(ctx):
    cases = [(p, r, w) for p, r, w in HAND if p is not None]
    got = _check(ctx, [p for p, _, _ in cases], COLUMN_OF, [r for _, r, _ in cases])          # seven stretches: two workgroups
    for g, (_, _, w) in zip(got, cases):
        assert [tuple(int(v) for v in row) for row in g] == w
    # one at a time, and the decode status: anything but 0 is "no path" for every group
    for p, r, w in cases:
        assert [tuple(int(v) for v in row) for row in _check(ctx, [p], COLUMN_OF, [r])[0]] == w
    p, r, _ = cases[4]
    got = _check(ctx, [p, p, p], COLUMN_OF, [r, r, r], status=[0, 1, 2])
    assert got[0][0, 0] == 0 and (got[1] == [1, -1, -1]).all() and (got[2] == [1, -1, -1]).all()


def _profile_path(rng, n_cols, T):
    """A monotone walk over the match (2 c) and insert (2 c + 1) states of n_cols columns, T observations."""
    cols = np.sort(rng.integers(0, n_cols, T))
    return (2 * cols + (rng.random(T) < 0.2)).astype(np.int32)


@pytest.mark.parametrize("T", [63, 64, 65, 129])
def test_lane_stride_and_tail(ctx, T):
    rng = np.random.Generator(np.random.PCG64(T))
    n_cols = 40
    column_of = np.repeat(np.arange(n_cols), 2)
    paths, groups = [], []
    for k in range(9):
        p = _profile_path(rng, n_cols, T)
        lo = int(column_of[p[0]]); hi = int(column_of[p[-1]])
        # ranges that end on the observation in front of the lane stride, on it and behind it, and the profile's first and last column
        at = [int(column_of[p[t]]) for t in (62, min(63, T - 1), min(64, T - 1), T - 2)]
        groups.append([(0, 0), (n_cols - 1, n_cols - 1), (lo, lo), (hi, hi), (0, n_cols - 1)] + [(c, c) for c in at] + [(max(0, c - 3), c) for c in at])
        paths.append(p)
    got = _check(ctx, paths, column_of, groups)
    assert {int(s) for g in got for s in g[:, 0]} >= {0, 2}
    # a group that holds the very last observation only, and one that holds everything but the first and the last
    p = np.array([0] + [2] * (T - 2) + [4], np.int32)
    got = _check(ctx, [p], [0, 0, 1, 1, 2, 2], [[(2, 2), (1, 1), (0, 0), (0, 2)]])
    assert got[0].tolist() == [[2, -1, -1], [0, 0, T - 1], [2, -1, -1], [2, -1, -1]]


def test_64_groups_in_one_flank(ctx):
    rng = np.random.Generator(np.random.PCG64(64))
    n_cols = 64 * 3
    column_of = np.concatenate([np.repeat(np.arange(n_cols), 2), [-1]])
    groups = [(3 * g, 3 * g + 1) for g in range(64)]          # every third column belongs to nobody
    paths = [_profile_path(rng, n_cols, T) for T in (700, 129, 64, 2000)]
    paths[1][5] = 2 * n_cols                                   # a state without a column
    got = _check(ctx, paths, column_of, [groups] * 4)
    assert all(g.shape == (64, 3) for g in got) and {int(s) for g in got for s in g[:, 0]} >= {0, 3}
    from strique_amd import ffi
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.debug_flank_mod_bounds(paths[:1], column_of, [groups + [(0, 0)]])
    assert e.value.code == ffi.STRQ_ERR_ARG and "64 groups" in str(e.value)
    with pytest.raises(ffi.StriqueHipError) as e:
        ctx.debug_flank_mod_bounds([np.array([2 * n_cols + 1], np.int32)], column_of, [groups])
    assert e.value.code == ffi.STRQ_ERR_ARG


def test_no_groups_and_empty_stretch(ctx):
    got = _check(ctx, [np.array([0, 2, 4], np.int32), np.zeros(0, np.int32)], [0, 0, 1, 1, 2, 2], [[], [(0, 1)]])
    assert got[0].shape == (0, 3) and got[1].tolist() == [[3, -1, -1]]
