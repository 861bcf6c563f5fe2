"""The score tables of the flank DP (csrc/lut_kernels.hip, build_tables) entry by entry against strq_oracle_cell_score, and the
same tables through the DP kernels: borderline entries patched or sent to the host, packed and float32 tables, the switches that
choose between them.  The cases and the host model of what the kernel has to report are in tests/table_cases.py
(tests/test_table_cases_host.py checks them without a GPU).  Everything is compared bit for bit: no tolerance anywhere."""
import numpy as np
import pytest

import table_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(ctx, orc):
    """Every case's table as the library builds it: one hook call per parameter set, and the batch of three of case b."""
    out = {}
    for params, cases in tc.by_params(tc.all_cases()):
        ctx.set_align_params(*params)
        for c, t in zip(cases, ctx.debug_score_tables(np.stack([c.levels for c in cases]), [c.classes for c in cases])):
            out[c.name] = t
    batch = tc.batch_b()
    ctx.set_align_params(*tc.P0)
    out["batch"] = ctx.debug_score_tables(np.stack([c.levels for c in batch]), [c.classes for c in batch])
    return out


def _check_table(case, t):
    m = tc.model_of(case)
    k = len(case.classes)
    got = (t["n_hard"], t["packed"], t["total"], t["entries"], sorted(t["handed"]))
    print(case.name, "n_hard %d packed %d total %d entries %d handed %s" % got, "model", m.n_hard, m.packed, sorted(m.sure.items()))
    assert m.determinate, case.name
    eff, idx = tc.effective(t, k)
    diff = np.argwhere(tc.bits_of(eff) != tc.bits_of(m.scores))
    assert len(diff) == 0, (case.name, [(int(x), int(q), float(eff[x, q]), float(m.scores[x, q]), float(case.classes[x]), float(case.levels[q])) for x, q in diff[:8]])
    assert t["n_hard"] == m.n_hard, (case.name, t["n_hard"], m.n_hard)
    assert t["packed"] == m.packed, (case.name, t["packed"], m.packed)
    if m.n_hard < 0:
        assert t["entries"] == 256 * k and not t["handed"], case.name
        assert np.array_equal(t["band_lo"].astype(np.int64) & 0xFFFFFFFF, (255 << 8) | (np.arange(k) * 256 << 16)), case.name
    else:
        assert t["entries"] == t["total"] and len(t["handed"]) == t["n_hard"], case.name
        want = {e for e, pos in m.sure.items() if pos == "interior"}
        assert want <= set(t["handed"]), (case.name, want, t["handed"])
        for x, q in t["handed"]:                       # only stored entries of rows that are written: first occurrences
            assert m.dup[x] == x and m.el[x] <= q <= m.er[x], (case.name, x, q)
    if t["packed"]:
        fixed = (t["hi16"].astype(np.uint32) << 8) | t["lo8"]
        assert np.array_equal(tc.bits_of((fixed.astype(np.float64) * 2.0 ** -20).astype(np.float32)), tc.bits_of(t["table"][:t["total"]])), case.name
        assert fixed.max() < 1 << 24


@pytest.mark.parametrize("kind", list("abcdefghi"))
def test_every_entry_equals_the_oracle(built, kind):
    """All 256 x k effective entries -- what the forward DP reads for (class, level) after its clamp -- have the bits of
    strq_oracle_cell_score; n_hard, packed and the list handed to the host are the host model's; a table reported as packed
    decodes to its float32 entries."""
    cases = [c for c in tc.all_cases() if c.kind == kind]
    assert cases
    for c in cases:
        _check_table(c, built[c.name])


def test_a_borderline_entry_in_the_last_job_of_a_batch(built):
    """Case b as job 2 of 3 (its read is not read 0): the host re-evaluates with THAT read's level values and patches THAT table."""
    batch = tc.batch_b()
    for c, t in zip(batch, built["batch"]):
        _check_table(c, t)
    assert [t["n_hard"] for t in built["batch"]] == [0, 0, 1] and built["batch"][2]["handed"] == [(70, 47)]
    assert [t["packed"] for t in built["batch"]] == [1, 1, 0]


# ---- the same tables through the DP kernels
def _run(ctx, orc, case, reads, flank=None, levels=None):
    flank = tc.flank_of(case) if flank is None else flank
    levels = case.levels if levels is None else levels
    params = np.array(case.params, np.float32)
    na, m = len(reads), len(flank)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    ctx.set_align_params(*case.params)
    got = ctx.align_batch(np.concatenate(reads), off, np.tile(levels, (na, 1)), np.arange(na, dtype=np.int32),
                          np.tile(flank, na), np.arange(na + 1, dtype=np.int64) * m)
    timing, geo = ctx.last_timing(), ctx.last_geometry()
    from conftest import oracle_map
    want = oracle_map(lambda lv: orc.align_overlap(levels[lv], flank, params, want_idx=False), reads)
    for i, o in enumerate(want):
        assert np.float32(o[0]).tobytes() == np.float32(got[0][i]).tobytes(), (case.name, i, o[0], got[0][i])
        assert (o[4], o[5]) == (int(got[1][i]), int(got[2][i])), (case.name, i)
        assert np.array_equal(o[3], got[3][i * m:(i + 1) * m]), (case.name, i)
    return want, timing, geo


DP_CASES = {c.name: c for c in tc.cases_b() + tc.cases_c() + tc.cases_d() + tc.cases_e() + tc.cases_f()}


@pytest.mark.parametrize("name", sorted(DP_CASES))
def test_best_path_through_the_special_entry(ctx, orc, name):
    """Reads whose best path (the oracle's rec says so) crosses the borderline / unpackable entry: score bits, end and start
    column and rec are the oracle's; the host re-evaluated at least the entries the model counts; the launch ran on float32
    tables, one per CU where the host rebuilt a 145-class table at full width."""
    case = DP_CASES[name]
    m = tc.model_of(case)
    reads = [tc.read_for(case, n, 40 + n) for n in (1500, 3000, 4000)]
    want, timing, geo = _run(ctx, orc, case, reads)
    print(name, "timing[4]", timing[4], geo)
    if case.special is not None:
        for lv, o in zip(reads, want):
            assert tc.crosses_special(case, lv, o[3]), name
    assert timing[4] >= max(m.n_hard, 0) * len(reads), (name, timing[4])
    assert geo["packed"] == m.packed, (name, geo)
    if m.n_hard < 0 and len(case.classes) == 145:
        assert geo["tables_per_cu"] == 1, (name, geo)


def test_borderline_entry_in_the_second_strip_of_a_long_flank(ctx, orc):
    """A flank of 300 classes runs as strips of 128 classes with a table each (class offset job_k0 in every index): the
    borderline entry of case b at class 200, i.e. class 72 of the second strip's table."""
    rng = np.random.default_rng(31)
    lv = tc.cases_b()[0].levels
    cls = rng.uniform(0.5, 9.5, 300).astype(np.float32)
    cls[200] = 0.0
    strip = tc._case("b/strip", "b", tc.P0, lv, cls[128:256], special=(72, 47))
    ms = tc.model(strip.params, strip.levels, strip.classes)
    assert ms.determinate and ms.sure == {(72, 47): "interior"}
    whole = tc.Case("b/long", "b", tc.P0, lv, cls, {}, (200, 47))
    for c3 in (cls[:128], cls[256:]):
        mo = tc.model(tc.P0, lv, c3)
        assert mo.determinate and not mo.sure
    reads = [tc.read_for(whole, n, 50 + n) for n in (3000, 4000)]
    want, timing, geo = _run(ctx, orc, whole, reads)
    for r, o in zip(reads, want):
        assert tc.crosses_special(whole, r, o[3])
    assert timing[4] >= len(reads), timing


def test_the_default_plan_runs_packed_tables_on_a_short_read(ctx, orc):
    """One of the short-read shapes of test_gpu_align.py (k = 145, n = 4000, STRique's parameters): the 24-bit kernel is what the
    default suite runs."""
    case = tc.cases_a()[0]
    _, timing, geo = _run(ctx, orc, case, [tc.read_for(case, 4000, 3)])
    assert geo["packed"] == 1 and timing[4] == 0, geo


@pytest.fixture(scope="module")
def switch_batch(orc):
    """k = 40 and k = 145, n = 30 000: the shapes of test_dist_min_above_dist_offset... / the seam tests, with their oracle results."""
    out = []
    for k, seed in ((40, 61), (145, 62)):
        lv, cl = tc.strique_like(seed, k=k)
        case = tc._case("switch/k%d" % k, "a", tc.P0, lv, cl)
        reads = [tc.read_for(case, 30000, seed + i, plant=i < 3) for i in range(4)]
        out.append((case, reads))
    return out


SWITCHES = [({"STRQ_PACK": "1", "STRQ_SEG": "1"}, {"packed": 1, "waves_per_alignment": 1}),
            ({"STRQ_PACK": "1", "STRQ_SEG": "2"}, {"packed": 1, "waves_per_alignment": 2}),
            ({"STRQ_PACK": "1", "STRQ_SEG": "4"}, {"packed": 1, "waves_per_alignment": 4}),
            ({"STRQ_NO_PACK": "1"}, {"packed": 0}),
            ({"STRQ_TABLES": "1"}, {"tables_per_cu": 1}),
            ({"STRQ_TABLES": "2"}, {"tables_per_cu": 2}),
            ({"STRQ_MAX_WAVES": "4"}, {}),
            ({"STRQ_NO_R14": "1"}, {"rows_per_lane": 15})]


@pytest.mark.parametrize("opts,geometry", SWITCHES, ids=["+".join("%s=%s" % kv for kv in o.items()) for o, _ in SWITCHES])
def test_switches_change_the_geometry_and_no_result(ctx, orc, switch_batch, opts, geometry):
    """The README's claim for STRQ_PACK, STRQ_NO_PACK, STRQ_TABLES, STRQ_MAX_WAVES and STRQ_NO_R14: another kernel instance or
    plan, the oracle's results.  STRQ_OVERLAP=1500 sends the weak alignment (no flank in the read) through the second round."""
    opts = dict(opts, STRQ_OVERLAP="1500")
    try:
        for key, value in opts.items():
            ctx.set_option(key, value)
        for case, reads in switch_batch:
            _, timing, geo = _run(ctx, orc, case, reads)
            print(opts, case.name, geo)
            for key, value in geometry.items():
                if key == "tables_per_cu":
                    assert geo[key] <= value, (opts, case.name, geo)
                elif key == "rows_per_lane":
                    assert len(case.classes) != 145 or geo[key] == value, (opts, case.name, geo)
                else:
                    assert geo[key] == value, (opts, case.name, geo)
    finally:
        for key in opts:
            ctx.set_option(key, None)


def test_generic_path_patches_a_borderline_pair(ctx, orc):
    """strq_align_overlap with more than 256 distinct values in `a` (the generic kernel and its own table): the pair
    (a = 1.354..., b = 0.0) is borderline and lies on the best path."""
    rng = np.random.default_rng(71)
    cls = rng.uniform(-8, 8, 12).astype(np.float32)
    cls[5] = 0.0
    b = np.repeat(cls, 6)
    a = rng.uniform(-9, 9, 2000).astype(np.float32)
    emb = np.repeat(cls, 7) + rng.uniform(-0.2, 0.2, 7 * len(cls)).astype(np.float32)
    emb[35:42] = tc.D_INTERIOR
    a[600:600 + len(emb)] = emb
    assert len(np.unique(a)) > 256
    params = np.array(tc.P0, np.float32)
    ctx.set_align_params(*tc.P0)
    want = orc.align_overlap(a, b, params)
    rec = want[3][30:36]
    assert any(not r & 1 and a[(r >> 1) - 1] == tc.D_INTERIOR for r in rec.tolist())
    got = ctx.align_overlap(a, b)
    assert ctx.last_timing()[4] >= 1
    assert np.float32(want[0]).tobytes() == np.float32(got[0]).tobytes() and (want[4], want[5]) == (got[4], got[5])
    assert np.array_equal(want[3], got[3]) and np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
