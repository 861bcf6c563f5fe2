"""Census of the case lists of tests/test_gpu_tables.py (tests/table_cases.py): every kind of score table the GPU module means to
compare is reached, the preconditions of every constructed case hold under the host's pow, and what the table kernel has to
report for a case does not depend on how its pow rounds (no entry between the model's two windows).  Runs on the host."""
from collections import Counter

import numpy as np
import pytest

import table_cases as tc


@pytest.fixture(scope="module")
def models(orc):
    cases = tc.all_cases() + tc.batch_b()[:2]
    return cases, {c.name: tc.model_of(c) for c in cases}


def test_every_committed_distance_is_borderline_under_the_c_pow():
    d = tc.BORDERLINE
    assert len(d) == 262 and np.all(np.diff(tc.bits_of(d).astype(np.int64)) > 0) and d[0] > 0 and d[-1] < 10.08
    y, low = tc.c_pow12(d)
    assert np.abs(low).max() <= tc.SURE and 2 * tc.SURE == tc.KERNEL_WINDOW
    assert int(((d >= 0.5) & (d < 8)).sum()) == 7 and int((d < 2.0 ** -20).sum()) == 214
    # a distance that is not on the list is not borderline: the neighbours of one that is
    _, low = tc.c_pow12(tc.f32(tc.bits_of(tc.D_INTERIOR) + 1))
    assert abs(int(low[0])) > tc.GRAY
    for x in (tc.D_CENTRE, tc.D_INTERIOR, tc.D_EDGE):
        assert x in d


def test_every_case_class_is_reached(models):
    cases, mod = models
    kinds = Counter(c.kind for c in cases)
    assert set(kinds) == set("abcdefghi") and kinds["i"] >= 99
    where = Counter(p for c in cases for p in mod[c.name].sure.values())
    assert set(where) == {"centre", "edge", "interior", "duplicate"}, where
    why = Counter(mod[c.name].why for c in cases)
    assert {"", "centre", "edge", "count", "levels"} <= set(why), why
    assert {mod[c.name].packed for c in cases} == {0, 1}
    ks = {len(c.classes) for c in cases}
    assert {1, 2, 128, 157, 158} <= ks


def test_no_case_depends_on_the_rounding_of_the_device_pow(models):
    cases, mod = models
    for c in cases:
        assert mod[c.name].determinate, (c.name, mod[c.name].sure, mod[c.name].gray)


def test_expectations_of_the_constructed_cases(models):
    cases, mod = models
    for c in cases:
        m = mod[c.name]
        for key in ("n_hard", "packed"):
            if key in c.expect:
                assert getattr(m, key) == c.expect[key], (c.name, key, getattr(m, key))
        if "where" in c.expect:
            assert m.where == c.expect["where"], (c.name, m.where)
        if c.kind == "a":
            assert m.n_hard == 0 and m.packed == 1 and not m.sure, c.name
        if c.special is not None and c.kind in "bcde":
            assert c.special in m.sure, c.name
    by = {c.name: (c, mod[c.name]) for c in cases}
    c, m = by["b/interior"]
    assert list(m.sure.items()) == [((70, 47), "interior")]
    c, m = by["c/centre"]
    assert m.best[33] == 120 and m.sure[(33, 120)] == "centre"
    c, m = by["e/64"]
    assert sorted(m.sure) == [(7, q) for q in range(1, 65)] and m.best[7] == 0
    c, m = by["e/65"]
    assert sorted(m.sure) == [(60, q) for q in range(1, 66)] and m.why == "count"


def test_the_clipped_edge_case_sits_on_dist_min(models):
    """Case d: the host's score at the borderline distance IS dist_min (clipped), the float on the other side of the rounding
    boundary gives a score above it -- so the entry ends the band on the host and would lie inside it for a pow that rounds the
    other way."""
    cases, mod = models
    c = [c for c in cases if c.name == "d/edge"][0]
    m = mod[c.name]
    off, dmin = np.float32(c.params[4]), np.float32(c.params[5])
    y, low = tc.c_pow12(np.array([tc.D_EDGE], np.float32))
    x = np.float32(y[0])
    assert 0 < low[0] <= tc.SURE and float(x) > y[0]                       # rounded up: the other candidate is the float below
    x2 = tc.f32(int(tc.bits_of(x)[0]) - 1)
    assert np.float32(off - x) == dmin and np.float32(off - x2) > dmin
    k, q = c.special
    assert m.scores[k, q] == dmin and m.scores[k, q - 1] > dmin and m.er[k] == q and m.sure[(k, q)] == "edge"


def test_packing_edges(models):
    cases, mod = models
    by = {c.name: (c, mod[c.name]) for c in cases}
    c, m = by["f/equal_bits"]
    assert tc.bits_of(c.levels)[100] == tc.bits_of(c.classes)[3] and m.scores[3, 100] == np.float32(16.0) and m.packed == 0
    c, m = by["f/negative_dist_min"]
    assert m.scores.min() == np.float32(-16.0) and (m.scores < 0).any() and m.packed == 0
    c, m = by["f/offset_20"]
    assert m.scores.max() >= 16.0 and m.packed == 0
    # 12.5: entries in [4, 8) with an odd multiple of 2^-21 exist, so this table does not pack either
    c, m = by["f/offset_12.5"]
    st = np.concatenate([m.scores[x, m.el[x]:m.er[x] + 1] for x in range(len(c.classes))])
    assert ((st * 2.0 ** 20) % 1 != 0).any() == (m.packed == 0)


def test_rows_shared_plateaus_and_hosts(models):
    cases, mod = models
    by = {c.name: (c, mod[c.name]) for c in cases}
    c, m = by["g/duplicates"]
    assert list(m.dup[[4, 5, 3, 20, 39]]) == [4, 4, 3, 3, 3]
    c, m = by["g/duplicate_borderline"]
    assert m.sure == {(70, 47): "interior", (90, 47): "duplicate"} and m.n_hard == 1
    for k in (2, 128, 157, 158):
        c, m = by["g/plateaus_k%d" % k]
        lo, hi = int(np.sum(c.levels == 55.0)) - 1, 256 - int(np.sum(c.levels == 125.0))
        assert lo > 10 and hi < 245 and (m.el == lo).any() and (m.er == hi).any(), c.name
    c, m = by["g/constant"]
    assert list(m.el) == [255, 255, 255, 0, 0, 255] and list(m.er) == [255, 255, 255, 0, 0, 255]
    for name in ("h/permuted", "h/nan_level"):
        c, m = by[name]
        assert m.rebuilt and m.why == "levels" and m.n_hard == -1


def test_clamping_into_the_modelled_band_changes_no_score(models):
    """The banding argument itself, on the host: for every case the entry at clamp(level, e_l, e_r) has the bits of the entry at
    the level."""
    cases, mod = models
    for c in cases:
        m = mod[c.name]
        q = np.arange(256)[None, :]
        cl = np.clip(q, m.el[:, None], m.er[:, None])
        got = np.take_along_axis(m.scores, cl, axis=1)
        assert np.array_equal(tc.bits_of(got), tc.bits_of(m.scores)), c.name


def test_the_planted_reads_cross_the_special_entries(orc):
    for c in tc.cases_b() + tc.cases_c() + tc.cases_d() + tc.cases_e() + tc.cases_f()[:1]:
        lv = tc.read_for(c, 3000, 11)
        o = orc.align_overlap(c.levels[lv], tc.flank_of(c), np.array(c.params, np.float32), want_idx=False)
        assert tc.crosses_special(c, lv, o[3]), c.name


def test_sizes_stay_modest(models):
    cases, _ = models
    assert len(cases) < 140 and sum(len(c.classes) for c in cases) < 14000
