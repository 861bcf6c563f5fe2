"""Census of the case lists of tests/test_gpu_conditioning.py (tests/cond_cases.py): every path of the conditioning kernels the
GPU module means to compare is reached by some read -- whatever the alignment of the batch buffer's base is -- and the oracle
has a usable expectation for every read that is not tagged otherwise.  Runs on the host."""
from collections import Counter

import numpy as np
import pytest

import cond_cases as cc


@pytest.fixture(scope="module")
def census(orc, opm):
    batches = cc.all_batches()
    exp = {(b.name, c.name): cc.expected(orc, opm, c) for b in batches for c in b.cases}
    return batches, exp


def test_every_dispatch_class_is_reached_for_every_base_alignment(census):
    batches, exp = census
    for base in range(8):
        seen = Counter()
        for b in batches:
            for i, _, at, rel in cc.compared(b):
                c = b.cases[i]
                seen.update(cc.classify(c, b.dtype, cc.phase(b, at, rel, base), exp[(b.name, c.name)]))
        missing = sorted(cc.required_classes() - set(seen))
        assert not missing, (base, missing)


def test_the_last_sub_batch_starts_at_every_residue(census):
    batches, _ = census
    for dtype, want in ((np.int16, set(range(8))), (np.float64, {0, 1})):
        got = set()
        for b in batches:
            if b.sub and b.dtype == dtype:
                i = cc.compared(b)[0][0]
                assert i > 0 and len(b.cases) - i == b.sub
                got.add(int(cc.offsets(b)[i]) % 8)
                lens = [len(c.signal) for c in b.cases[i:]]
                k = lens.index(0)
                assert lens[k + 1] == 1 and lens[k - 1] > 2 * cc.COND_TILE and lens[k + 2] > 2 * cc.COND_TILE      # empty, one sample, between long reads
        assert got == want


def test_tags_agree_with_the_oracle(census):
    """Untagged: MAD > 0 and every level value finite.  empty_tails: MAD > 0 (levels are compared), no finite level value.
    degenerate: levels undefined -- and only for reads that cannot be anything else: at most two samples, constant, or a NaN."""
    batches, exp = census
    n_degenerate = 0
    for b in batches:
        for c in b.cases:
            e = exp[(b.name, c.name)]
            if "degenerate" in c.tags:
                n_degenerate += 1
                s = c.signal
                assert len(s) <= 2 or np.isnan(s).any() or (s == s[0]).all(), c.name
                assert e.u8 is None and not e.ok, c.name
                continue
            assert e.mad > 0 and e.u8 is not None and len(e.u8) == len(c.signal), c.name
            if "empty_tails" in c.tags:
                assert np.isnan(e.morph).all() and not e.ok, c.name
            else:
                assert np.isfinite(e.morph).all() and e.ok, c.name
    # the listed ones: per int16 edge block the reads of one and two samples, the empty and the one-sample read between long ones,
    # the constant reads, the read with two NaNs, the empty float64 read, and the empty / one-sample reads of the sub-batch runs
    assert n_degenerate == 8 * 2 + 2 + 1 + (2 + 3) + (8 + 2) * 2


def test_a_lone_nan_against_scipy():
    """scipy's medfilt sides with the oracle's medfilt3 (np.sort: NaN last) on the read with one NaN: the median of three drops
    it.  (What scipy's selection makes of two NaNs in a row depends on the order it visits them in; the oracle keeps them.)"""
    import scipy.signal
    from oracle import strique_oracle
    b = [b for b in cc.all_batches() if b.name == "float64_edges"][0]
    s = [c.signal for c in b.cases if c.name == "f/nan"][0]
    flt = scipy.signal.medfilt(s, 3)
    assert np.isnan(s).sum() == 1 and not np.isnan(flt).any() and np.array_equal(flt, strique_oracle.medfilt3(s))
    s = [c.signal for c in b.cases if c.name == "f/nan_pair"][0]
    assert np.isnan(strique_oracle.medfilt3(s)).sum() == 2


def test_special_reads_are_what_their_names_say(census):
    batches, exp = census
    by = {c.name: (c, exp[(b.name, c.name)]) for b in batches for c in b.cases}
    c, e = by["range/extremes"]
    assert e.flt.min() == -32768 and e.flt.max() == 32767
    for bins in (cc.HSTAT_LDS_BINS, cc.HSTAT_LDS_BINS + 1):
        c, e = by["range/bins%d" % bins]
        assert int(e.flt.max()) - int(e.flt.min()) + 1 == bins
    c, e = by["range/step6000"]
    assert "empty_tails" in c.tags
    c, e = by["hist/n%d" % cc.LONG_READ]
    assert len(c.signal) >= 300000
    # truncation against rounding: z * 24 + 127 a few ulps from an integer at (nearly) every sample, on both sides of it
    c, e = by["f/near_integer"]
    z = (e.flt - e.med) / e.mad * 24 + 127
    near = np.abs(z - np.round(z)) < 1e-12
    assert near.sum() >= 2000 and (z[near] < np.round(z[near])).sum() >= 100 and (z[near] >= np.round(z[near])).sum() >= 100
    # neighbouring reads whose edge samples would change the median if they took the zero pad's place
    for b in batches:
        if b.name in ("int16_edges", "int16_leak"):
            for prev, c in zip(b.cases, b.cases[1:]):
                s, p = c.signal.astype(np.int64), prev.signal.astype(np.int64)
                if len(s) >= 3 and len(p) >= 3:
                    assert sorted([p[-1], s[0], s[1]])[1] != sorted([0, s[0], s[1]])[1], c.name
                    assert sorted([p[-2], p[-1], s[0]])[1] != sorted([p[-2], p[-1], 0])[1], prev.name


def test_sizes_stay_modest(census):
    batches, _ = census
    assert sum(len(b.cases) for b in batches) < 2500 and sum(len(c.signal) for b in batches for c in b.cases) < 4000000
