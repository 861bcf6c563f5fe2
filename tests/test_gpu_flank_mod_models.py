"""Flank methylation calls at model level on the GPU against tests/flank_mod_ref.py: the segmentation decode of
hmm.FlankProfileModel (strq_viterbi_batch with path -- a 150-nt flank has 290 emitting states, beyond the lane slots), the bounds of
flank_mod_bounds_kernel (strq_debug_flank_mod_bounds) on that path, and (V_base, V_mod) of hmm.SiteModModel through the passage
scorer of the per-unit scores (strq_debug_mod_llr_scores), all three scorer modes.

The reads: the bundled C9orf72 target and the HTT target with their 150-nt flanks, both strands, each synthesised once from the
base table and once from the mCpG table, 6 kb with arrays of 12 / 27 units; int16 for both targets, float64 for C9orf72.  A flank's
stretch is where the alignment of the whole configured flank begins and ends (flank_mod_ref.flank_ranges), normalised and clipped as
the modification pass takes its stretch.  status, u, w and n_columns are compared exactly, v_base and v_mod to the bit.

Ties (flank_mod_ref): a (read, group) pair whose bounds differ between the oracle's in-edge order and the baked model's is compared
with nothing; at most 2 % of the pairs of a parametrisation (tests/test_flank_mod_host.py finds none for the seed in use)."""
import numpy as np
import pytest

import flank_mod_ref as fr

pytestmark = pytest.mark.gpu


class _Arrays(object):
    def __init__(self, model):
        self.__dict__.update(model.baked._asdict()); self.column_of = model.column_of


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    c = ffi.Context(0)
    yield c
    c.close()
    _MODELS.clear()


_MODELS = {}


def _profile(ctx, pm, cfg, flank):
    from strique_amd import hmm
    if ("p", flank) not in _MODELS:
        m = hmm.FlankProfileModel(flank, pm, cfg["HMM"])
        _MODELS[("p", flank)] = (ctx.model_create(m.baked), m)
    return _MODELS[("p", flank)]


def _site(ctx, pm, pm_mod, cfg, seq):
    from strique_amd import hmm
    if ("s", seq) not in _MODELS:
        m = hmm.SiteModModel(seq, pm, pm_mod, cfg["HMM"])
        ne = m.baked.silent_start
        _MODELS[("s", seq)] = (ctx.model_create(m.baked), 0 if ne <= 32 else (1 if ne <= 64 else 2))
    return _MODELS[("s", seq)]


def gpu_call(ctx, pm, pm_mod, cfg, flank, x):
    """[(status, u, w, n_columns, v_base, v_mod)] per group of `flank` on the stretch x, and the scorer modes that ran."""
    from strique_amd import flank_mod
    k = pm.kmer
    gs = flank_mod.check(flank, k)
    if flank_mod.too_long(len(x), len(flank)):
        return [(flank_mod.TOO_LONG, -1, -1, g.n_columns, np.nan, np.nan) for g in gs], set()
    mid, model = _profile(ctx, pm, cfg, flank)
    _, _, status, paths = ctx.viterbi_batch(mid, [x], want_path=True)
    b = ctx.debug_flank_mod_bounds([paths[0]], model.column_of[:model.baked.silent_start], [[(g.c0, g.c1) for g in gs]], status=[int(status[0])])[0]
    V = np.full((len(gs), 2), np.nan)
    by_mode = {}
    for j, g in enumerate(gs):
        if b[j, 0] == flank_mod.SCORED:
            sid, mode = _site(ctx, pm, pm_mod, cfg, flank_mod.site_sequence(flank, g, k))
            by_mode.setdefault(mode, []).append((j, sid))
    for mode, items in by_mode.items():
        xs = [x[b[j, 1]:b[j, 2] + 1] for j, _ in items]
        got, launched = ctx.debug_mod_llr_scores([sid for _, sid in items], xs, [np.array([len(s) - 1], np.int32) for s in xs])
        assert launched == (mode, 2)
        for (j, _), v in zip(items, got):
            V[j] = v[0]
    return [(int(b[j, 0]), int(b[j, 1]), int(b[j, 2]), g.n_columns, V[j, 0], V[j, 1]) for j, g in enumerate(gs)], set(by_mode)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.mark.parametrize("names,as_int16", [(("c9orf72", "htt"), True), (("c9orf72",), False)])
def test_calls_equal_the_reference(ctx, pm, pm_mod, tables, cfg, targets, names, as_int16):
    from strique_amd import flank_mod
    cases, opm, opm_mod = fr.cases(tables, cfg, targets, names, as_int16)
    pairs = ties = scored = 0
    modes = set()
    for c in cases:
        for which, flank, b, e, x in c["flanks"]:
            what = (c["target"], c["strand"], c["table"], which)
            mid, model = _profile(ctx, pm, cfg, flank)
            assert model.baked.silent_start == 2 * (len(flank) - pm.kmer + 1) == 290
            ref = fr.call(x, flank, opm, opm_mod, cfg["HMM"], alt=_Arrays(model))
            got, ran = gpu_call(ctx, pm, pm_mod, cfg, flank, x)
            modes |= ran
            assert len(got) == len(ref) == len(flank_mod.groups(flank, pm.kmer)), what
            for r, g in zip(ref, got):
                pairs += 1
                if r["tie"]:
                    ties += 1
                    continue
                assert g[:4] == (r["status"], r["u"], r["w"], r["n_columns"]), (what, r, g)
                assert _bits(g[4:]) == _bits([r["v_base"], r["v_mod"]]), (what, r, g)
                scored += r["status"] == fr.SCORED
    print("flank-mod models: %d pairs, %d ties, %d scored, modes %s" % (pairs, ties, scored, sorted(modes)))
    assert ties <= fr.TIE_CAP * pairs and scored >= 0.75 * pairs
    assert modes == {0, 1, 2} if "htt" in names else modes >= {0, 2}


def test_edge_skipped_and_too_long(ctx, pm, pm_mod, opm, opm_mod, cfg, targets):
    """A flank that starts with CG (edge), a stretch synthesised with a group's CG deleted (skipped), a stretch above 64 L (too_long,
    nothing decoded), and a flank without CG (no groups)."""
    from strique_amd import flank_mod, synth
    rng = np.random.Generator(np.random.PCG64(11))
    table = synth.KmerTable(pm)

    def signal(seq):
        x = synth.make_signal(rng, table, seq.encode(), as_int16=False)
        return np.clip(x, min(opm.model_min, opm_mod.model_min), max(opm.model_max, opm_mod.model_max))

    flank = "CGTTAGCATTGACTTAGGCATCGATTTGACCATAGGTACCATTAGCAGTCG"          # CG at 0, at 21 and at L - 2 (one column: the last)
    assert flank_mod.sites(flank) == [0, 21, len(flank) - 2]
    for x, want in ((signal(flank), [fr.EDGE, fr.SCORED, fr.EDGE]),
                    (signal(flank[:-2]), [fr.EDGE, fr.SCORED, fr.SKIPPED]),          # the last group's CG deleted: its one k-mer is gone
                    (np.resize(signal(flank), 64 * len(flank) + 1), [fr.TOO_LONG] * 3)):
        ref = fr.call(x, flank, opm, opm_mod, cfg["HMM"], alt=_Arrays(_profile(ctx, pm, cfg, flank)[1]))
        got, _ = gpu_call(ctx, pm, pm_mod, cfg, flank, x)
        assert [r["status"] for r in ref] == want and not any(r["tie"] for r in ref), ref
        for r, g in zip(ref, got):
            assert g[:4] == (r["status"], r["u"], r["w"], r["n_columns"]) and _bits(g[4:]) == _bits([r["v_base"], r["v_mod"]]), (r, g)
    assert gpu_call(ctx, pm, pm_mod, cfg, "ATTAGCATTGACTTAGGCAT", signal("ATTAGCATTGACTTAGGCAT")) == ([], set())
