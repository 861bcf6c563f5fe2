"""The edge images of the variant pass and of the per-unit scores (strq_debug_variant_image / strq_debug_mod_llr_image), interpreted
on the CPU (passage_cases.interpret_image), against the oracle's Viterbi on the masked copies of the model, to the bit -- product
models of every compiled instance and crafted ones at the sizes and in-degrees where the image changes shape; the refusals of the
two builders; and the conditions that keep these cases from checking nothing.  No GPU."""
import numpy as np
import pytest

import passage_cases as pc


def _variant(pm, repeat, alts):
    from strique_amd import hmm
    m = hmm.RepeatVariantModel(repeat, alts, pm)
    return m.baked, (m.model_min, m.model_max)


def _mod(pm, pm_mod, unit):
    from strique_amd import hmm
    m = hmm.RepeatModModel(unit, pm, pm_mod)
    return m.baked, (m.model_min, m.model_max)


def _check_windows(image, baked, nb, rng, lo, hi, tags):
    """interpret_image == reference_scores on every window of host_windows; returns {window name: reference scores}."""
    ref = {}
    for name, x in pc.host_windows(rng, lo, hi):
        want = pc.reference_scores(baked, nb, x, [len(x) - 1], tags)[0]
        got = pc.interpret_image(image, nb, x, tags)
        assert pc.same_bits(got, want), (name, got, want)
        ref[name] = want
    return ref


def _check_alive(ref, unit_nt, dual=False):
    """What the reference itself must show, so that the comparison above is none of -inf with -inf.  (The two branches of a dual
    model are the same profile over two pore models: a window has a path in both or in neither, so there the short windows are
    asked to differ from each other, where those of a variant model -- an alt branch spans m + 1 units -- differ inside a window.)"""
    for n in pc.LONG:
        assert np.isfinite(ref["len%d" % n]).all(), n
    for n in (1, 2):
        assert not np.isfinite(ref["len%d" % n]).any(), n
    if dual:
        short = [np.isfinite(ref["len%d" % n]) for n in (3, 4, 5, 8)]
        assert all(f.all() or not f.any() for f in short) and (unit_nt > 6 or any(f.all() for f in short))
    elif unit_nt <= 6:
        assert any(np.isfinite(ref["len%d" % n]).any() and not np.isfinite(ref["len%d" % n]).all() for n in (3, 4, 5, 8))
    for name in ("outside_hi", "outside_lo"):
        assert not np.isfinite(ref[name]).any(), name
    for name in ("nan5", "ends_lo_hi", "ends_hi_lo"):
        assert np.isfinite(ref[name]).all(), name


@pytest.mark.parametrize("case", pc.product_variant_cases(), ids=lambda c: "%s_%d" % (c[0], len(c[1])))
def test_product_variant_images(pm, orc, case):
    from strique_amd import ffi
    repeat, alts, ne, (mode, nb) = case
    baked, (lo, hi) = _variant(pm, repeat, alts)
    assert baked.silent_start == ne
    image = ffi.debug_variant_image(baked, len(alts))
    assert image["rc"] == 0 and (image["mode"], image["n_branch"], image["n_emit"]) == (mode, nb, ne)
    ref = _check_windows(image, baked, nb, np.random.default_rng(ne), lo, hi, "var")
    _check_alive(ref, len(repeat))


def test_every_variant_instance_has_a_product_model_but_one():
    have = {inst for _, _, _, inst in pc.product_variant_cases()}
    assert have == {(m, nb) for m in range(3) for nb in (2, 3, 4)} - {(0, 4)}
    assert set(pc.INSTANCE_MODELS) == have


@pytest.mark.parametrize("nt", sorted(pc.MOD_UNITS))
def test_product_mod_llr_images(pm, pm_mod, orc, nt):
    from strique_amd import ffi
    baked, (lo, hi) = _mod(pm, pm_mod, pc.MOD_UNITS[nt])
    assert baked.silent_start == 2 + 4 * nt
    image = ffi.debug_mod_llr_image(baked)
    assert image["rc"] == 0 and image["mode"] == pc.MOD_MODES[nt]
    ref = _check_windows(image, baked, 2, np.random.default_rng(nt), lo, hi, "llr")
    _check_alive(ref, nt, dual=True)


# (ne, nb, own_deg, copy_deg, end_deg): the sizes at which the lane layout changes, (mode 0, NB 4), the last legal in-degrees
CRAFTED = [(32, 4, 5, 3, 3), (6, 4, 3, 3, 2), (32, 2, 6, 3, 4), (33, 3, 5, 4, 3), (64, 4, 5, 3, 5), (65, 2, 7, 3, 3), (128, 3, 5, 3, 3),
           (64, 3, 8, 4, 8), (128, 4, 8, 4, 8), (32, 4, 8, 4, 8)]


def _check_crafted(image, m, nb, tags, seed):
    ref = _check_windows(image, m, nb, np.random.default_rng(seed), pc.CRAFT_LO, pc.CRAFT_HI, tags)
    finite = np.array([np.isfinite(v) for v in ref.values()])
    assert finite.any() and not finite.all()          # some windows have a path, the shortest have none
    assert all(np.isfinite(ref["len%d" % n]).all() for n in (64, 129, 200))
    assert not np.isfinite(ref["len1"]).any()


@pytest.mark.parametrize("shape", CRAFTED, ids=lambda s: "-".join(str(v) for v in s))
def test_crafted_variant_images(orc, shape):
    from strique_amd import ffi
    ne, nb, own, copy, end = shape
    m = pc.crafted_model(np.random.default_rng(ne * 100 + nb), ne, nb, own, copy, end)
    image = ffi.debug_variant_image(m, nb - 1)
    assert image["rc"] == 0, image["why"]
    assert (image["mode"], image["n_branch"]) == (0 if ne <= 32 else 1 if ne <= 64 else 2, nb)
    if ne >= 32:          # the degrees asked for were reached, and the image says so
        assert (m.degrees["own"], m.degrees["copy"], m.degrees["end"]) == (own, copy, end)
        assert image["deg"] == own and image["deg2"] == copy and image["end_deg"][0] == end
    _check_crafted(image, m, nb, "var", ne)


@pytest.mark.parametrize("shape", [(1, 2, 3, 3, 1), (32, 2, 5, 3, 3), (33, 2, 5, 3, 3), (64, 2, 8, 4, 8), (65, 2, 5, 3, 3), (128, 2, 8, 4, 8)],
                         ids=lambda s: "-".join(str(v) for v in s))
def test_crafted_mod_llr_images(orc, shape):
    from strique_amd import ffi
    ne, nb, own, copy, end = shape
    m = pc.crafted_model(np.random.default_rng(ne * 100 + 7), ne, nb, own, copy, end, tags="llr")
    image = ffi.debug_mod_llr_image(m)
    assert image["rc"] == 0, image["why"]
    assert image["mode"] == (0 if ne <= 32 else 1 if ne <= 64 else 2)
    if ne >= 32:
        assert image["deg"] == own and image["deg2"] == copy and image["end_deg"][0] == end
    ref = _check_windows(image, m, 2, np.random.default_rng(ne), pc.CRAFT_LO, pc.CRAFT_HI, "llr")
    assert all(np.isfinite(ref["len%d" % n]).all() for n in (64, 129, 200))


REFUSALS = [((129, 3, 5, 3, 3), "at most 128 emitting states"), ((64, 3, 9, 4, 8), "more than 8 in-edges"),
            ((64, 3, 8, 5, 8), "more than 4 in-edges inside one branch"), ((64, 3, 8, 4, 9), "end state"), ((1, 2, 3, 3, 1), "no state of branch")]


@pytest.mark.parametrize("shape,text", REFUSALS, ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_variant_image_refusals(shape, text):
    from strique_amd import ffi
    ne, nb, own, copy, end = shape
    m = pc.crafted_model(np.random.default_rng(5), ne, nb, own, copy, end)
    if ne in (64, 129):
        assert (m.degrees["own"], m.degrees["copy"], m.degrees["end"]) == (own, copy, end)
    image = ffi.debug_variant_image(m, nb - 1)
    assert image["rc"] == 1 and image["why"].startswith("variants: ") and text in image["why"], image


@pytest.mark.parametrize("shape,text", REFUSALS[:4], ids=lambda v: v if isinstance(v, str) else "-".join(str(x) for x in v))
def test_mod_llr_image_refusals(shape, text):
    from strique_amd import ffi
    ne, _, own, copy, end = shape
    m = pc.crafted_model(np.random.default_rng(6), ne, 2, own, copy, end, tags="llr")
    if ne == 64:
        assert (m.degrees["own"], m.degrees["copy"], m.degrees["end"]) == (own, copy, end)
    image = ffi.debug_mod_llr_image(m)
    assert image["rc"] == 1 and image["why"].startswith("mod-llr: ") and text in image["why"], image


def test_variant_image_other_refusals(pm):
    """alt counts outside 1 .. 3, a tag beyond the alt branches, missing tags: each with its reason."""
    from strique_amd import ffi
    baked, _ = _variant(pm, "CGG", ["AGG", "CAG"])
    assert "between 1 and 3 alt units" in ffi.debug_variant_image(baked, 0)["why"]
    assert "between 1 and 3 alt units" in ffi.debug_variant_image(baked, 4)["why"]
    assert "state tags of a variant model with 1 alt units" in ffi.debug_variant_image(baked, 1)["why"]
    assert "no state of branch 3" in ffi.debug_variant_image(baked, 3)["why"]
    assert "no state tags" in ffi.debug_variant_image(pc.as_model(baked, tag=None), 2)["why"]


def test_reference_marks_unusable_bounds(pm, orc):
    """-inf for every branch where not 0 <= u_j <= w_j < T, and only there."""
    baked, (lo, hi) = _variant(pm, "CGG", ["AGG"])
    x = pc.signal(np.random.default_rng(3), 200, lo, hi)
    w = np.array([39, 79, -1, 99, 90, 130, 200, 199], np.int32)
    V = pc.reference_scores(baked, 2, x, w)
    assert [bool(np.isfinite(v).all()) for v in V] == [True, True, False, True, False, True, False, False]
    assert pc.same_bits(V[3], pc.reference_scores(baked, 2, x[:100], [99])[0])
