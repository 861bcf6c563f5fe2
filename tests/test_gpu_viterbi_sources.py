"""The Viterbi kernels on the window sources of the detect pipeline: int16 or float64 samples and a per-window map
x' = clip((s - c1) / h1 * h2 + c2, lo, hi), through strq_debug_viterbi_sourced.  For such windows the kernels choose, once per
window, between two instantiations of their time loop -- the branch-free emission code when [lo, hi] lies inside every Uniform
emission's support and c1, h1 are numbers, the general code otherwise (the one every plain float64 window takes).  The model-level
tests of tests/test_gpu_viterbi_modes.py see only the second; here the same checks run on the first, and the two are compared bit
by bit.

The cases and both references: tests/vit_mode_cases.py (sourced_windows); tests/test_vit_mode_cases_host.py checks without a GPU
that they land where they claim, that the predicate is what each window claims and that the windows exercise marks, hub and unit
chains and ties.  Every comparison is exact."""
import numpy as np
import pytest

import vit_mode_cases as vc
from test_gpu_viterbi_modes import G2_OPTIONS, _check_window, _g2_unit_numbering, options

pytestmark = pytest.mark.gpu

KINDS = (vc.VIT_SRC_I16_AFFINE, vc.VIT_SRC_F64_AFFINE)
KIND_NAMES = {vc.VIT_SRC_I16_AFFINE: "int16", vc.VIT_SRC_F64_AFFINE: "float64"}


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


@pytest.fixture(scope="module")
def src_cases(pm, pm_mod, cfg):
    return vc.sourced_cases(pm, pm_mod, cfg)


@pytest.fixture(scope="module")
def models(ctx, src_cases):
    """case name -> (model id, plan), registered on first use."""
    from strique_amd import ffi
    made = {}

    def get(name):
        if name not in made:
            c = src_cases[name]
            mid = ctx.model_create(c.baked)
            if c.g2:
                assert ctx.last_positions_rc == 0, ctx.last_positions_error
            made[name] = (mid, ffi.debug_viterbi_plan(c.baked))
        return made[name]
    return get


def _sourced_launch(ctx, mid, mode, kind, sws, expect_shape, what):
    res = ctx.debug_viterbi_sourced(mid, mode, kind, [sw.samples for sw in sws], [sw.consts for sw in sws])
    assert res["launched"] == expect_shape, what + (res["launched"], expect_shape)
    return res


def _same_bits(got, want, sws, mode, what):
    """Two launches over the same windows, window by window: every raw result and every record byte."""
    for i, sw in enumerate(sws):
        w = what + (sw.label,)
        assert got["status"][i] == want["status"][i] and np.float64(got["logp"][i]).tobytes() == np.float64(want["logp"][i]).tobytes(), w
        if sw.label.startswith("nopath"):
            assert got["status"][i] == 1, w
            continue
        assert got["counted"][i] == want["counted"][i] and got["dbg"][i].tobytes() == want["dbg"][i].tobytes(), w + (got["dbg"][i], want["dbg"][i])
        if mode in (vc.VIT_HUB, vc.VIT_UNIT):
            assert got["records"][i].tobytes() == want["records"][i].tobytes(), w
        else:
            assert got["records"][i] is None and want["records"][i] is None, w


def _run_case(ctx, orc, c, mid, mode, shape, kmap, what):
    """Both source kinds of the case's windows in one launch each: against references A and B (the checks of
    test_gpu_viterbi_modes), and against the launch of the plain float64 window x_prime -- the general instantiation -- bit by bit.
    Returns the results by kind."""
    out = {}
    for kind in KINDS:
        sws = [sw for sw in vc.sourced_windows(c) if sw.kind == kind]
        if not sws:
            continue
        w = what + (KIND_NAMES[kind],)
        res = _sourced_launch(ctx, mid, mode, kind, sws, shape, w)
        for i, sw in enumerate(sws):
            _check_window(orc, c, mode, vc.ref_label(sw), sw.x_prime, res, i, kmap)
        plain = ctx.debug_viterbi_mode(mid, mode, [sw.x_prime for sw in sws])
        assert plain["launched"] == shape, w
        _same_bits(res, plain, sws, mode, w)
        out[kind] = (sws, res)
    return out


@pytest.mark.parametrize("name", vc.SOURCED_NAMES)
def test_sourced_windows_against_both_references_and_the_plain_launch(ctx, orc, src_cases, models, name):
    from strique_amd import ffi
    c = src_cases[name]
    mid, plan = models(name)
    assert {sw.fast for sw in vc.sourced_windows(c)} >= {True}
    for mode in c.modes:
        if mode == vc.VIT_BACKPTR:          # (back-pointer launches belong to strq_viterbi_batch: plain float64 windows only)
            continue
        what = (name, vc.MODE_NAMES[mode])
        if not c.g2:
            _run_case(ctx, orc, c, mid, mode, plan["shape"], (0, 1), what)
            continue
        # STRique's flanked models: the register-resident kernel under every exchange level and wave count, then the lane row
        kmap = _g2_unit_numbering(c.baked)
        first = _run_case(ctx, orc, c, mid, mode, ffi.VIT_SHAPE_G2, kmap, what)
        for opts in G2_OPTIONS:
            with options(ctx, opts):
                run = _run_case(ctx, orc, c, mid, mode, ffi.VIT_SHAPE_G2, kmap, what + (str(opts),))
            for kind, (sws, res) in run.items():
                _same_bits(res, first[kind][1], sws, mode, what + (str(opts), "against the default"))
        with options(ctx, {"STRQ_VIT_NO_G2": 1}):
            lane = _run_case(ctx, orc, c, mid, mode, plan["shape"], (0, 1), what + ("NO_G2",))
        assert ctx.get_option("STRQ_VIT_NO_G2") == "" and ctx.get_option("STRQ_VIT_G2_LDS") == ""
        for kind, (sws, res) in lane.items():
            for i, sw in enumerate(sws):          # (the payload of a unit decode names the counted states in the kernel's own numbering)
                if not sw.label.startswith("nopath"):
                    assert np.float64(res["logp"][i]).tobytes() == np.float64(first[kind][1]["logp"][i]).tobytes(), what + (sw.label,)
                    assert res["counted"][i] == first[kind][1]["counted"][i], what + (sw.label,)


@pytest.mark.parametrize("name", vc.BOUNDARY_NAMES)
def test_mark_boundaries_exact_on_int16_samples(ctx, src_cases, models, name):
    c = src_cases[name]
    mid, plan = models(name)
    sws = vc.sourced_windows(c)
    res = _sourced_launch(ctx, mid, vc.VIT_MARK, vc.VIT_SRC_I16_AFFINE, sws, plan["shape"], (name,))
    got = [(int(d[0]), int(d[1]), int(k), int(s)) for d, k, s in zip(res["dbg"], res["counted"], res["status"])]
    assert got == [(enter, leave, leave - enter, 0) for enter, leave in vc.BOUNDARY_TIMES], got


@pytest.mark.parametrize("name", vc.WIDE_NAMES)
def test_tract_payload_on_int16_windows(ctx, src_cases, name):
    """The wide-payload count launch over sourced windows: counters and log-probability against both references of
    tests/tract_ref.py on x_prime, and equal to strq_viterbi_tracts on x_prime."""
    import tract_ref as tr
    from strique_amd import ffi
    from test_gpu_tracts import spread
    c = src_cases[name]
    bk = c.baked
    K = 3 if int((np.asarray(bk.count_inc)[:bk.silent_start] == 1).sum()) >= 3 else 2
    tract_of = spread(bk, K)
    mid = ctx.model_create(bk)
    ctx.model_set_tracts(mid, K, tract_of)
    plan = ffi.debug_viterbi_plan(bk)
    sws = [sw for sw in vc.sourced_windows(c) if sw.label in ("i16_T65", "i16_T333")]
    assert len(sws) == 2 and all(sw.fast for sw in sws)
    res = ctx.debug_viterbi_sourced(mid, vc.VIT_COUNT, vc.VIT_SRC_I16_AFFINE, [sw.samples for sw in sws], [sw.consts for sw in sws], tracts=True)
    assert res["launched"] == plan["shape"], (name, res["launched"], plan)
    plain = ctx.viterbi_tracts(mid, [sw.x_prime for sw in sws])
    seen = np.zeros(K, bool)
    for i, sw in enumerate(sws):
        a = tr.decode_a(bk, tract_of, K, sw.x_prime)
        b = tr.decode_b(bk, tract_of, K, sw.x_prime)
        seen |= np.array(a[1]) > 0
        what = (name, sw.label, float(res["logp"][i]), [int(v) for v in res["tract_counts"][i]], a, b)
        assert a[1:] == b[1:] and np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and a[2] == 0, what          # (the references agree)
        assert int(res["status"][i]) == 0 and [int(v) for v in res["tract_counts"][i]] == a[1] + [0] * (3 - K), what
        assert np.float64(res["logp"][i]).tobytes() == np.float64(a[0]).tobytes(), what
        assert np.float64(plain[0][i]).tobytes() == np.float64(res["logp"][i]).tobytes() and np.array_equal(plain[1][i], res["tract_counts"][i]), what
    assert seen.sum() >= 2, (name, seen)          # the windows count in more than one field of the payload


@pytest.mark.parametrize("name", ["wide_row2_multi", "wide_row7_ss", "wide_general", "flanked_c9orf72", "dual_ggcccc"])
def test_window_in_a_ragged_sourced_batch_equals_the_window_alone(ctx, src_cases, models, name):
    """Seventy int16 windows of random lengths (so most start at an odd sample), every one with its own map and both values of the
    predicate where the case has them: windows 0, 33 and 69 give the bits they give alone."""
    c = src_cases[name]
    mid, plan = models(name)
    rng = np.random.default_rng(5)
    pool = [sw for sw in vc.sourced_windows(c) if sw.kind == vc.VIT_SRC_I16_AFFINE and len(sw.samples) >= 3]
    samples, consts = [], []
    for i in range(70):
        sw = pool[i % len(pool)]
        samples.append(sw.samples[:int(rng.integers(3, min(len(sw.samples), 400) + 1))]); consts.append(sw.consts)
    off = np.cumsum([0] + [len(s) for s in samples])
    assert sum(int(o) % 2 for o in off[:-1]) >= 10
    for mode in c.modes:
        if mode == vc.VIT_BACKPTR:
            continue
        batch = ctx.debug_viterbi_sourced(mid, mode, vc.VIT_SRC_I16_AFFINE, samples, consts)
        for i in (0, 33, 69):
            alone = ctx.debug_viterbi_sourced(mid, mode, vc.VIT_SRC_I16_AFFINE, [samples[i]], [consts[i]])
            assert alone["launched"] == batch["launched"]
            for k in ("logp", "counted", "status", "dbg"):
                assert alone[k][0].tobytes() == batch[k][i].tobytes(), (name, vc.MODE_NAMES[mode], i, k)
            if batch["records"][i] is not None:
                assert alone["records"][0].tobytes() == batch["records"][i].tobytes(), (name, vc.MODE_NAMES[mode], i)


def test_what_the_hook_refuses(ctx, src_cases, models):
    from strique_amd import ffi
    c = src_cases["wide_row2_ss"]
    mid, _ = models("wide_row2_ss")
    sw = next(sw for sw in vc.sourced_windows(c) if sw.label == "i16_T63")
    f64 = next(sw for sw in vc.sourced_windows(c) if sw.label == "f64_T65")
    c1, h1, h2, c2, lo, hi = sw.consts

    def refused(code, mid_, mode, kind, samples, consts, **kw):
        with pytest.raises(ffi.StriqueHipError) as ei:
            ctx.debug_viterbi_sourced(mid_, mode, kind, [samples], [consts], **kw)
        assert ei.value.code == code, (ei.value, mode, kind, consts)

    for kind in (0, 3, -1):          # (0: plain float64 windows have a hook of their own)
        refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, kind, sw.samples, sw.consts)
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, sw.kind, sw.samples, (c1, 0.0, h2, c2, lo, hi))
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, sw.kind, sw.samples, (c1, h1, h2, c2, hi, lo))
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, sw.kind, sw.samples, (c1, h1, h2, c2, np.nan, hi))
    bad = f64.samples.copy(); bad[17] = np.nan          # a missing sample under constants that are numbers: never launched
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, f64.kind, bad, f64.consts)
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_COUNT, sw.kind, sw.samples, sw.consts, tracts=True)          # no tracts set
    refused(ffi.STRQ_ERR_ARG, mid, vc.VIT_BACKPTR, sw.kind, sw.samples, sw.consts)
    # no launch of the mode: exactly where strq_debug_viterbi_mode says so
    for name, mode in (("wide_row6_ss", vc.VIT_UNIT), ("wide_row0_ss", vc.VIT_HUB), ("wide_general", vc.VIT_UNIT), ("wide_general", vc.VIT_HUB),
                       ("boundary_ss", vc.VIT_HUB)):
        m, _ = models(name)
        w = vc.sourced_windows(src_cases[name])[2]
        refused(ffi.STRQ_ERR_UNSUPPORTED, m, mode, w.kind, w.samples[:50], w.consts)
        with pytest.raises(ffi.StriqueHipError) as ei:
            ctx.debug_viterbi_mode(m, mode, [w.x_prime[:50]])
        assert ei.value.code == ffi.STRQ_ERR_UNSUPPORTED
    # the launch that follows is what it was
    res = ctx.debug_viterbi_sourced(mid, vc.VIT_COUNT, sw.kind, [sw.samples], [sw.consts])
    assert res["status"][0] == 0


def test_every_kernel_instance_is_launched_with_the_predicate_true(ctx, src_cases, models, capsys):
    """One short window per case and mode whose clip range lies inside every Uniform support: together the sourced cases launch
    every (shape, single-stage, mode) the table of vit_model.h has an instance for, on the branch-free code.  The list goes to the log."""
    from strique_amd import ffi
    launched = set()
    for name in vc.SOURCED_NAMES:
        c = src_cases[name]
        mid, plan = models(name)
        sw = next(sw for sw in vc.sourced_windows(c) if sw.fast and len(sw.samples) >= 40 and not sw.label.startswith("nopath"))
        assert vc.predicate(c.baked, sw.consts), (name, sw.label)
        one = sw._replace(samples=sw.samples[:40])
        for mode in c.modes:
            if mode == vc.VIT_BACKPTR:
                continue
            if c.g2:
                launched.add((_sourced_launch(ctx, mid, mode, one.kind, [one], ffi.VIT_SHAPE_G2, (name, mode))["launched"], mode))
                with options(ctx, {"STRQ_VIT_NO_G2": 1}):
                    launched.add((_sourced_launch(ctx, mid, mode, one.kind, [one], plan["shape"], (name, mode))["launched"], mode))
            else:
                launched.add((_sourced_launch(ctx, mid, mode, one.kind, [one], plan["shape"], (name, mode))["launched"], mode))
    with capsys.disabled():
        print("\nViterbi launches on sourced windows, predicate true (row, single-stage, mode):")
        for shape, mode in sorted(launched):
            print("  row %d  ss %d  %s" % (shape & ~ffi.VIT_SHAPE_SS, 1 if shape & ffi.VIT_SHAPE_SS else 0, vc.MODE_NAMES[mode]))
    want = set()
    for row, modes in vc.ROW_MODES.items():
        for mode in modes:
            if mode != vc.VIT_BACKPTR:
                want |= {(row, mode)} if row >= ffi.VIT_SHAPE_CSR else {(row, mode), (row | ffi.VIT_SHAPE_SS, mode)}
    assert not (want - launched), sorted(want - launched)
