"""The score kernels of the variant pass and of the per-unit scores, and the bounds kernels of the variant pass, on their own
(strq_debug_variant_scores / strq_debug_mod_llr_scores / strq_debug_variant_bounds) against tests/passage_cases.py: every compiled
instance, passage lengths around the chunk of the time loop, the two halves of a wave with different lengths and models, more
passages than the grid has waves, missing and out-of-support observations, unusable bounds, and the `bad` outcomes of the bounds
kernels.  Every score is compared bit for bit, -inf included."""
import numpy as np
import pytest

import passage_cases as pc
import variant_ref

pytestmark = pytest.mark.gpu

# The grid of a score launch is capped at 8 workgroups of 4 waves per CU; a wave of a mode 0 instance takes two passages.  An
# MI355X has 256 CUs; the counts below exceed the cap for up to 304.
SLOTS = 8 * 304 * 4

_MODELS = {}


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    c = ffi.Context(0)
    yield c
    c.close()
    _MODELS.clear()


def _variant(ctx, pm, repeat, n_alt):
    """(model id, baked arrays, (lo, hi), image) of a product variant model, registered once."""
    key = ("var", repeat, n_alt)
    if key not in _MODELS:
        from strique_amd import ffi, hmm
        alts = next(a for r, a, _, _ in pc.PRODUCT_VARIANTS if r == repeat)[:n_alt]
        m = hmm.RepeatVariantModel(repeat, alts, pm)
        _MODELS[key] = (ctx.model_create(m.baked), m.baked, (m.model_min, m.model_max), ffi.debug_variant_image(m.baked, n_alt))
    return _MODELS[key]


def _mod(ctx, pm, pm_mod, nt):
    key = ("mod", nt)
    if key not in _MODELS:
        from strique_amd import ffi, hmm
        m = hmm.RepeatModModel(pc.MOD_UNITS[nt], pm, pm_mod)
        _MODELS[key] = (ctx.model_create(m.baked), m.baked, (m.model_min, m.model_max), ffi.debug_mod_llr_image(m.baked))
    return _MODELS[key]


def _crafted(ctx, ne, nb, own=5, copy=3, end=3, tags="var"):
    key = ("crafted", ne, nb, own, copy, end, tags)
    if key not in _MODELS:
        from strique_amd import ffi
        m = pc.crafted_model(np.random.default_rng(1000 * ne + nb), ne, nb, own, copy, end, tags)
        image = ffi.debug_variant_image(m, nb - 1) if tags == "var" else ffi.debug_mod_llr_image(m)
        assert image["rc"] == 0, image["why"]
        _MODELS[key] = (ctx.model_create(m), m, (pc.CRAFT_LO, pc.CRAFT_HI), image)
    return _MODELS[key]


def _instance_model(ctx, pm, mode, nb):
    if (mode, nb) == (0, 4):
        return _crafted(ctx, 32, 4)
    return _variant(ctx, pm, *pc.INSTANCE_MODELS[(mode, nb)])


def _run(ctx, nb, models, xs, ws, tags="var"):
    """One launch over the reads (models[r], xs[r], ws[r]); returns (scores per read, the instance that ran)."""
    ids = [m[0] for m in models]
    if tags == "var":
        return ctx.debug_variant_scores(ids, nb - 1, xs, ws)
    return ctx.debug_mod_llr_scores(ids, xs, ws)


def _compare(got, nb, models, xs, ws, tags="var"):
    """Bit equality with the oracle, read by read; returns the reference."""
    refs = []
    for r, (m, x, w) in enumerate(zip(models, xs, ws)):
        want = pc.reference_scores(m[1], nb, x, w, tags)
        bad = [j for j in range(len(w)) if not pc.same_bits(got[r][j], want[j])]
        assert not bad, (r, bad[:5], got[r][bad[0]], want[bad[0]], pc.usable(w, len(x))[bad[0]])
        refs.append(want)
    return refs


def _instance_read(rng, W, lo, hi):
    lengths = np.concatenate([rng.permutation(pc.instance_lengths(W)) for _ in range(2)])
    return pc.signal(rng, int(lengths.sum()) + 7, lo, hi), pc.bounds_of(lengths), lengths


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,nb", [(m, nb) for m in range(3) for nb in (2, 3, 4)])
def test_every_variant_instance(ctx, pm, orc, mode, nb):
    model = _instance_model(ctx, pm, mode, nb)
    assert (model[3]["mode"], model[3]["n_branch"]) == (mode, nb)
    x, w, lengths = _instance_read(np.random.default_rng(10 * mode + nb), 32 if mode == 0 else 64, *model[2])
    got, ran = _run(ctx, nb, [model], [x], [w])
    assert ran == (mode, nb)
    ref = _compare(got, nb, [model], [x], [w])[0]
    long_ones = np.isfinite(ref[lengths >= 31])
    if (mode, nb) == (0, 4):          # (the crafted model: a window of three observations has a path, a Uniform branch state may shut one)
        assert long_ones.any()
    else:
        assert long_ones.all() and not np.isfinite(ref).all()


@pytest.mark.parametrize("nt,mode", [(7, 0), (15, 1), (31, 2)])
def test_every_mod_llr_instance(ctx, pm, pm_mod, orc, nt, mode):
    model = _mod(ctx, pm, pm_mod, nt)
    assert model[3]["mode"] == mode
    x, w, lengths = _instance_read(np.random.default_rng(nt), 32 if mode == 0 else 64, *model[2])
    got, ran = _run(ctx, 2, [model], [x], [w], "llr")
    assert ran == (mode, 2)
    ref = _compare(got, 2, [model], [x], [w], "llr")[0]
    assert np.isfinite(ref[lengths >= 31]).all() and not np.isfinite(ref).all()


def test_crafted_sizes_and_last_legal_degrees(ctx, orc):
    """Crafted models at the sizes where the lane layout changes and with the last rows of src / src2 / end_src filled."""
    rng = np.random.default_rng(77)
    for ne, nb, own, copy, end in [(32, 4, 8, 4, 8), (33, 3, 5, 4, 3), (64, 3, 8, 4, 8), (65, 2, 7, 3, 3), (128, 4, 8, 4, 8)]:
        model = _crafted(ctx, ne, nb, own, copy, end)
        assert (model[3]["deg"], model[3]["deg2"], model[3]["end_deg"][0]) == (own, copy, end)
        x, w, _ = _instance_read(rng, 32 if ne <= 32 else 64, *model[2])
        got, ran = _run(ctx, nb, [model], [x], [w])
        assert ran == (0 if ne <= 32 else 1 if ne <= 64 else 2, nb)
        assert np.isfinite(_compare(got, nb, [model], [x], [w])[0]).any()
    for ne, own, copy, end in [(1, 3, 3, 1), (32, 8, 4, 8), (64, 8, 4, 8), (128, 8, 4, 8)]:
        model = _crafted(ctx, ne, 2, own, copy, end, "llr")
        x, w, _ = _instance_read(rng, 32 if ne <= 32 else 64, *model[2])
        got, _ = _run(ctx, 2, [model], [x], [w], "llr")
        assert np.isfinite(_compare(got, 2, [model], [x], [w], "llr")[0]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
def _second_model(ctx, nb):
    """A crafted 30-state model with other in-degrees than the first of a mode 0 instance."""
    return _crafted(ctx, 30, nb, 8, 4, 6)


@pytest.mark.parametrize("nb", [2, 3, 4])
def test_halves_of_one_wave(ctx, pm, orc, nb):
    """Mode 0: a wave holds two passages.  (short, long) and (long, short) pairs, an odd number of passages, and two models with
    different deg / deg2 in the two halves."""
    first = _instance_model(ctx, pm, 0, nb)
    rng = np.random.default_rng(nb)
    one = lambda model, n: (model, pc.signal(rng, n, *model[2]), np.array([n - 1], np.int32))
    reads = [one(first, n) for n in (3, 70, 70, 3, 33)]
    got, ran = _run(ctx, nb, *zip(*reads))
    assert ran == (0, nb)
    ref = _compare(got, *([nb] + [list(v) for v in zip(*reads)]))
    assert np.isfinite(ref[1]).any() and np.isfinite(ref[2]).any()
    # bounds inside one read: the halves of a wave are consecutive passages of unequal length
    x = pc.signal(rng, 300, *first[2]); w = pc.bounds_of([3, 70, 70, 3, 33, 64, 5])
    got, _ = _run(ctx, nb, [first], [x], [w])
    _compare(got, nb, [first], [x], [w])
    # two models
    second = _second_model(ctx, nb)
    assert (first[3]["deg"], first[3]["deg2"]) != (second[3]["deg"], second[3]["deg2"])
    reads = [one((first, second)[i % 2], n) for i, n in enumerate((3, 70, 33, 31, 64, 5, 65, 40, 40))]
    reads += [one((second, first)[i % 2], n) for i, n in enumerate((40, 40, 3, 70, 33))]
    got, ran = _run(ctx, nb, *zip(*reads))
    assert ran == (0, nb)
    ref = np.concatenate(_compare(got, *([nb] + [list(v) for v in zip(*reads)])))
    assert np.isfinite(ref).any()


@pytest.mark.parametrize("kind,mode,nb", [("var", 0, 2), ("var", 0, 4), ("var", 1, 3), ("var", 2, 4), ("llr", 0, 2), ("llr", 2, 2)])
def test_more_passages_than_waves(ctx, pm, pm_mod, orc, kind, mode, nb):
    """Every wave of the capped grid takes several passages, one after the other: reads of one tile of 40 short windows each, every
    97th read of a second model.  The expected scores are computed once per (model, tile); every repetition carries the same bits."""
    if kind == "var":
        first = _instance_model(ctx, pm, mode, nb)
        second = _second_model(ctx, nb) if mode == 0 else _crafted(ctx, 64 if mode == 1 else 100, nb, 6, 4, 4)
    else:
        first = _mod(ctx, pm, pm_mod, 7 if mode == 0 else 16)
        second = _crafted(ctx, 32 if mode == 0 else 128, 2, 8, 4, 8, "llr")
    rng = np.random.default_rng(5)
    lengths = np.array([5 + (7 * i) % 16 for i in range(40)])
    w = pc.bounds_of(lengths)
    tiles = [pc.signal(rng, int(lengths.sum()) + 3, *m[2]) for m in (first, second)]
    want = [pc.reference_scores(m[1], nb, x, w, kind) for m, x in zip((first, second), tiles)]
    assert all(len({v.tobytes() for v in t}) > 10 for t in want)          # the windows of a tile differ
    n_reads = (SLOTS * (2 if mode == 0 else 1)) // 40 + 2
    which = [1 if r % 97 == 96 else 0 for r in range(n_reads)]
    got, ran = _run(ctx, nb, [(first, second)[k] for k in which], [tiles[k] for k in which], [w] * n_reads, kind)
    assert ran == (mode, nb) and n_reads * 40 > SLOTS * (2 if mode == 0 else 1)
    wrong = [r for r in range(n_reads) if not pc.same_bits(got[r], want[which[r]])]
    assert not wrong, (len(wrong), wrong[:8])


# ---------------------------------------------------------------------------------------------------------------------------------
def _value_read(rng, lo, hi):
    """A stretch of ten passages of 40 observations with, per passage: nothing, NaN at both hub positions, NaN inside, NaN
    everywhere, a first observation above / below the support, hub observations at (lo, hi) and (hi, lo), nothing, nothing."""
    x = pc.signal(rng, 400, lo, hi); w = pc.bounds_of([40] * 10)
    x[40] = x[79] = np.nan
    x[85:110:5] = np.nan
    x[120:160] = np.nan
    x[160] = np.nextafter(hi, np.inf)
    x[200] = np.nextafter(lo, -np.inf)
    x[240], x[279] = lo, hi
    x[280], x[319] = hi, lo
    return x, w


@pytest.mark.parametrize("mode,nb", [(0, 2), (1, 3), (2, 4)])
def test_variant_values(ctx, pm, orc, mode, nb):
    model = _instance_model(ctx, pm, mode, nb)
    x, w = _value_read(np.random.default_rng(mode), *model[2])
    got, _ = _run(ctx, nb, [model], [x], [w])
    ref = _compare(got, nb, [model], [x], [w])[0]
    assert [bool(np.isfinite(v).all()) for v in ref] == [True, True, True, True, False, False, True, True, True, True]
    assert not np.isfinite(ref[4]).any() and not np.isfinite(ref[5]).any()


@pytest.mark.parametrize("nt", [7, 31])
def test_mod_llr_values(ctx, pm, pm_mod, orc, nt):
    model = _mod(ctx, pm, pm_mod, nt)
    x, w = _value_read(np.random.default_rng(nt), *model[2])
    if nt == 31:          # longer windows for the longest unit: the marks fall inside them, and one first observation outside the support
        w = pc.bounds_of([150, 150]); x[150] = np.nextafter(model[2][1], np.inf)
    got, _ = _run(ctx, 2, [model], [x], [w], "llr")
    ref = _compare(got, 2, [model], [x], [w], "llr")[0]
    if nt == 31:
        assert np.isfinite(ref[0]).all() and not np.isfinite(ref[1]).any()
    else:
        assert [bool(np.isfinite(v).all()) for v in ref] == [True, True, True, True, False, False, True, True, True, True]
        assert not np.isfinite(ref[4]).any() and not np.isfinite(ref[5]).any()


@pytest.mark.parametrize("kind,mode,nb", [("var", 0, 3), ("var", 1, 4), ("var", 2, 2), ("llr", 0, 2), ("llr", 1, 2)])
def test_unusable_bounds(ctx, pm, pm_mod, orc, kind, mode, nb):
    """-1 (a bound nobody wrote), a bound at or behind T, bounds that do not ascend: -inf for every branch of that passage -- and of
    the one behind a bound at or behind T, whose first observation lies outside the stretch -- and nothing else changes."""
    model = _instance_model(ctx, pm, mode, nb) if kind == "var" else _mod(ctx, pm, pm_mod, 7 if mode == 0 else 15)
    x = pc.signal(np.random.default_rng(9), 600, *model[2])
    clean = np.array([79, 159, 239, 319, 399, 479, 559, 599], np.int32)
    w = clean.copy(); w[2] = -1; w[4] = 300; w[6] = 600
    reads = [(model, x, clean), (model, x, w), (model, x, np.array([-1], np.int32)), (model, x, np.array([1 << 30, 79], np.int32)),
             (model, x, np.array([-2, 79], np.int32))]
    got, _ = _run(ctx, nb, *(list(v) for v in zip(*reads)), kind)
    ref = _compare(got, *([nb] + [list(v) for v in zip(*reads)] + [kind]))
    assert np.isfinite(ref[0]).all()
    assert [bool(np.isfinite(v).any()) for v in ref[1]] == [True, True, False, True, False, True, False, False]
    for j in (0, 1):          # passages whose own two bounds are those of the clean read score what they score there
        assert pc.same_bits(got[1][j], got[0][j])
    assert not np.isfinite(np.concatenate(ref[2:4])).any() and not np.isfinite(ref[4]).any()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(ctx, pm):
    """The product model of CGG with three alt units, its hub and branch states, and a decoded stretch with its passages."""
    mid, baked, (lo, hi), _ = _variant(ctx, pm, "CGG", 3)
    br = pc.branches(baked)
    hubs = [int(l) for l in np.flatnonzero(br == pc.HUB)]
    inner = [[int(l) for l in np.flatnonzero(br == b)][:5] for b in range(4)]
    x = pc.signal(np.random.default_rng(4), 701, lo, hi)
    logp, _, status, path = ctx.viterbi(mid, x, want_path=True)
    assert status == 0 and np.isfinite(logp)
    ps = variant_ref.passages(br, path)
    assert len(ps) > 20 and len({p[2] for p in ps}) > 1
    return dict(id=mid, br=br, s0=hubs[0], e0=hubs[1], inner=inner, T=len(x), path=np.asarray(path, np.int32), ps=ps)


def _crafted_paths(chain):
    """Paths whose passages end at observations 62 .. 65, 127, 128 (a hub at the first lane of a round of 64 behind a branch state at
    the last lane of the round before), with lengths that are no multiple of 64."""
    out = []
    for ends, T in [((5, 62, 65, 127, 140), 141), ((20, 63, 128), 129), ((64, 100, 191, 194), 195), ((61, 64, 67, 126, 129), 131)]:
        path = pc.path_with_ends(ends, T, chain["s0"], chain["e0"], chain["inner"])
        ps = variant_ref.passages(chain["br"], path)
        assert [p[1] for p in ps] == list(ends)
        out.append((path, ps))
    return out


def _check_bounds(res, ps):
    assert (res["n"], res["bad_count"], res["bad_write"], res["untouched"]) == (len(ps), 0, 0, True), res
    assert list(res["w"]) == [p[1] for p in ps] and list(res["branch"]) == [p[2] for p in ps]


def test_bounds_scan_route(ctx, chain):
    reads = [(chain["path"], chain["ps"])] + _crafted_paths(chain)
    out = ctx.debug_variant_bounds(chain["id"], 3, [len(p) for p, _ in reads], paths=[p for p, _ in reads])
    for res, (_, ps) in zip(out, reads):
        _check_bounds(res, ps)


def test_bounds_hop_route(ctx, chain):
    reads = [(chain["path"], chain["ps"])] + _crafted_paths(chain)
    recs = [pc.hub_records(len(p), ps) for p, ps in reads]
    out = ctx.debug_variant_bounds(chain["id"], 3, [len(p) for p, _ in reads], recs=[r for r, _ in recs], last=[l for _, l in recs])
    for res, (_, ps) in zip(out, reads):
        _check_bounds(res, ps)


def _is_bad_count(res):
    assert (res["n"], res["bad_count"], res["untouched"]) == (0, 1, True), res


def _is_bad_write(res, n):
    assert (res["n"], res["bad_count"], res["bad_write"], res["untouched"]) == (n, 0, 1, True), res


def test_bounds_scan_route_bad(ctx, chain):
    """What variant_kernels.h names: more passages than `cap`, a branch outside the model's, a write pass that finds another count;
    and a decode without a path with a non-zero cap.  The guard entries behind `cap` stay as they were."""
    path, ps = _crafted_paths(chain)[0]
    T, n = len(path), len(ps)
    dense = np.array([chain["s0"] if t % 2 == 0 else chain["inner"][0][0] for t in range(30)], np.int32)          # 14 passages, cap 11
    alt3 = pc.path_with_ends((5, 20), 21, chain["s0"], chain["e0"], [chain["inner"][3]])
    out = ctx.debug_variant_bounds(chain["id"], 3, [30, T, T, T, T], paths=[dense, path, path, path, path],
                                   status=[0, 0, 0, 1, 1], cap=[-1, n + 1, n - 1, 2, -1])
    _is_bad_count(out[0])
    _is_bad_write(out[1], n); _is_bad_write(out[2], n)
    assert list(out[2]["w"]) == [p[1] for p in ps[:n - 1]]          # the entries below the cap are the first passages
    _is_bad_write(out[3], 0)
    assert (out[4]["n"], out[4]["bad_count"], out[4]["bad_write"], out[4]["untouched"]) == (0, 0, 0, True)          # no path, no cap: nothing to say
    # the same path is fine for the model's four branches and wrong for three
    ok = ctx.debug_variant_bounds(chain["id"], 3, [21], paths=[alt3])[0]
    assert (ok["n"], ok["bad_count"], list(ok["branch"])) == (2, 0, [3, 3])
    _is_bad_count(ctx.debug_variant_bounds(chain["id"], 2, [21], paths=[alt3])[0])


def test_bounds_hop_route_bad(ctx, chain):
    """... and on the records: a record outside (0, T], times that do not descend."""
    path, ps = _crafted_paths(chain)[0]
    T, n = len(path), len(ps)
    rec, last = pc.hub_records(T, ps)
    dense = np.arange(31, dtype=np.uint64); dense[1:] -= 1          # record p points at p - 1: 30 passages in 30 observations, cap 11
    branch4 = rec.copy(); branch4[ps[1][1] + 1] = (4 << 32) | int(rec[ps[1][1] + 1] & 0xFFFFFFFF)
    same = rec.copy(); same[last] = (int(rec[last]) >> 32 << 32) | last          # a record that points at itself
    ahead = rec.copy(); ahead[ps[1][1] + 1] = last                             # ... at a later one
    cases = [(dense, 30, 30, 0, -1), (branch4, T, last, 0, -1), (same, T, last, 0, -1), (ahead, T, last, 0, -1), (rec, T, T + 1, 0, -1)]
    out = ctx.debug_variant_bounds(chain["id"], 3, [c[1] for c in cases], recs=[c[0] for c in cases], last=[c[2] for c in cases])
    for res in out:
        _is_bad_count(res)
    out = ctx.debug_variant_bounds(chain["id"], 3, [T] * 5, recs=[rec] * 5, last=[last, last, last, last, 0],
                                   status=[0, 0, 1, 1, 0], cap=[n + 1, n - 1, 2, -1, -1])
    _is_bad_write(out[0], n); _is_bad_write(out[1], n); _is_bad_write(out[2], 0)
    assert len(out[1]["w"]) == n - 1 and (out[1]["w"] == 0x7F7F7F7F).all()          # the walk is checked before anything is written
    for res in out[3:]:          # no path / no record at all: no passages, and nothing wrong with that
        assert (res["n"], res["bad_count"], res["bad_write"], res["untouched"]) == (0, 0, 0, True)
    assert any(p[2] == 3 for p in ps)          # a chain that is fine for the model's four branches is wrong for three
    _is_bad_count(ctx.debug_variant_bounds(chain["id"], 2, [T], recs=[rec], last=[last])[0])
