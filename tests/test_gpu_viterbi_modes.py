"""The MARK, HUB and UNIT decodes (and COUNT beside them) of every Viterbi kernel shape, one launch at a time through
strq_debug_viterbi_mode, against the two references of tests/vit_mode_cases.py: the shape that ran is the planned one, the
log-probability has the oracle's bits, counts, marks and hop chains equal reference A (the oracle's path) entry by entry, and every
record a live state wrote equals reference B (the DP that carries the payloads).  Every comparison is exact.
tests/test_vit_mode_cases_host.py checks, without a GPU, that the cases land where they claim and exercise what they claim."""
import numpy as np
import pytest

import vit_mode_cases as vc

pytestmark = pytest.mark.gpu

# the register-resident kernel: exchange levels and waves per workgroup, then the lane row of the same model
G2_OPTIONS = [{"STRQ_VIT_G2_LDS": l} for l in (0, 1, 2)] + [{"STRQ_VIT_G2_WAVES": w} for w in (4, 8, 12)]


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


@pytest.fixture(scope="module")
def all_cases(pm, pm_mod, cfg):
    return vc.cases(pm, pm_mod, cfg)


@pytest.fixture(scope="module")
def models(ctx, all_cases):
    """case name -> (model id, plan), registered on first use."""
    from strique_amd import ffi
    made = {}

    def get(name):
        if name not in made:
            c = all_cases[name]
            mid = ctx.model_create(c.baked)
            if c.g2:
                assert ctx.last_positions_rc == 0, ctx.last_positions_error
            made[name] = (mid, ffi.debug_viterbi_plan(c.baked))
        return made[name]
    return get


class options(object):
    """Context options for the length of a with block; the entries are removed afterwards."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, None)


def _g2_unit_numbering(bk):
    """The register-resident kernel numbers the two counted states by the slot that holds them -- the match-type one (the broadcast
    source of the match-type states) writes record 0, the insert-type one record 1 (vit_model.h: VitModel::g2_unit) -- where the lane
    kernels number them by ascending state.  k of the references -> k of that kernel."""
    us = vc.unit_states(bk)
    kmap = tuple(int(bk.pos_kind[s]) for s in us)
    assert sorted(kmap) == [0, 1]
    return kmap


def _check_window(orc, c, mode, label, x, res, i, kmap=(0, 1)):
    """Window i of a launch of `mode` against A and B; kmap: how the kernel that ran numbers the two counted states."""
    what = (c.name, vc.MODE_NAMES[mode], label)
    a = vc.reference_a(orc, c, label, x)
    logp, counted, status, dbg = res["logp"][i], int(res["counted"][i]), int(res["status"][i]), [int(v) for v in res["dbg"][i]]
    if a["path"] is None:
        assert status == 1 and logp == -np.inf, what
        return
    assert np.float64(logp).tobytes() == np.float64(a["logp"]).tobytes() and status == 0, what + (logp, a["logp"], status)
    assert dbg[2] == 0 and dbg[3] == 0, what
    if mode == vc.VIT_COUNT:
        assert counted == a["counted"] and dbg[:2] == [0, 0], what + (counted, a["counted"], dbg)
        return
    if mode == vc.VIT_MARK:
        assert (counted, dbg[0], dbg[1]) == (a["counted"], a["enter"], a["leave"]), what + (counted, dbg, a["counted"], a["enter"], a["leave"])
        return
    b = vc.reference_b(c, label, x)
    rec = res["records"][i]
    if mode == vc.VIT_HUB:
        assert dbg[0] == (a["hub"][-1][0] if a["hub"] else 0) and dbg[1] == 0, what + (dbg, a["hub"][-3:])
        assert vc.hub_chain(dbg[0], rec) == a["hub"], what
        assert len(rec) == len(x) + 1 and rec[0] == 0, what          # no state emits at time 0
        live = b["hub_live"]
        assert np.array_equal(rec[live], b["hub_rec"][live]), what + (np.nonzero(rec[live] != b["hub_rec"][live])[0][:5],)
    else:
        chain = [(t, kmap[k]) for t, k in a["unit"]]
        assert dbg[0] == (((chain[-1][0] + 1) << 1 | chain[-1][1]) if chain else 0) and dbg[1] == 0 and counted == 0, what + (dbg, chain[-3:])
        assert vc.unit_chain(dbg[0], rec) == chain, what
        assert rec.shape == (len(x), 2), what
        for k in (0, 1):
            live = b["unit_live"][:, k]; want = b["unit_rec"][live, k]
            want = np.where(want == 0, 0, (want & ~np.uint32(1)) | np.where(want & 1, kmap[1], kmap[0]).astype(np.uint32)).astype(np.uint32)
            assert np.array_equal(rec[live, kmap[k]], want), what + (k,)


def _launch(ctx, mid, mode, xs, expect_shape, what):
    res = ctx.debug_viterbi_mode(mid, mode, xs)
    assert res["launched"] == expect_shape, what + (res["launched"], expect_shape)
    return res


@pytest.mark.parametrize("name", vc.CASE_NAMES)
def test_modes_against_both_references(ctx, orc, all_cases, models, name):
    from strique_amd import ffi
    c = all_cases[name]
    mid, plan = models(name)
    labels = [l for l, _ in c.windows]; xs = [x for _, x in c.windows]
    for mode in c.modes:
        what = (name, vc.MODE_NAMES[mode])
        if mode == vc.VIT_BACKPTR:
            # the back-pointer instance of the row, through strq_viterbi_batch: the oracle's path itself
            lg, cg, sg, paths = ctx.viterbi_batch(mid, xs, want_path=True)
            for i, (label, x) in enumerate(c.windows):
                a = vc.reference_a(orc, c, label, x)
                if a["path"] is None:
                    assert sg[i] == 1 and lg[i] == -np.inf, what + (label,)
                    continue
                assert np.float64(lg[i]).tobytes() == np.float64(a["logp"]).tobytes() and sg[i] == 0 and cg[i] == a["counted"], what + (label,)
                assert np.array_equal(paths[i], a["path"]), what + (label,)
            continue
        if not c.g2:
            res = _launch(ctx, mid, mode, xs, plan["shape"], what)
            for i, (label, x) in enumerate(c.windows):
                _check_window(orc, c, mode, label, x, res, i)
            continue
        # STRique's flanked models: the register-resident kernel under every exchange level and wave count, then the lane row
        first = _launch(ctx, mid, mode, xs, ffi.VIT_SHAPE_G2, what)
        runs = [("default", first)]
        for opts in G2_OPTIONS:
            with options(ctx, opts):
                runs.append((str(opts), _launch(ctx, mid, mode, xs, ffi.VIT_SHAPE_G2, what + (opts,))))
        with options(ctx, {"STRQ_VIT_NO_G2": 1}):
            runs.append(("lane row", _launch(ctx, mid, mode, xs, plan["shape"], what + ("NO_G2",))))
        assert ctx.get_option("STRQ_VIT_NO_G2") == "" and ctx.get_option("STRQ_VIT_G2_LDS") == ""
        kmap = _g2_unit_numbering(c.baked)
        ok = [i for i, l in enumerate(labels) if not l.startswith("nopath")]
        for tag, res in runs:
            lane = tag == "lane row"
            for i, (label, x) in enumerate(c.windows):
                _check_window(orc, c, mode, label, x, res, i, (0, 1) if lane else kmap)
            # identical to the first run; the payload of a unit decode names the counted states in the kernel's own numbering
            keys = ("logp", "counted", "status") if lane and mode == vc.VIT_UNIT else ("logp", "counted", "status", "dbg")
            for k in keys:
                assert first[k][ok].tobytes() == res[k][ok].tobytes(), what + (tag, k)


@pytest.mark.parametrize("name", ["boundary_ss", "boundary_multi", "boundary_csr"])
def test_mark_boundaries_exact(ctx, all_cases, models, name):
    """The first tagged emission and the first emission behind it at 4095, 4096, 4097 and 8192: where the packed payload of the
    lane and general kernels splits the enter time into 12 + 10 bits."""
    c = all_cases[name]
    mid, plan = models(name)
    res = _launch(ctx, mid, vc.VIT_MARK, [x for _, x in c.windows], plan["shape"], (name,))
    got = [(int(d[0]), int(d[1]), int(k), int(s)) for d, k, s in zip(res["dbg"], res["counted"], res["status"])]
    assert got == [(enter, leave, leave - enter, 0) for enter, leave in vc.BOUNDARY_TIMES], got


@pytest.mark.parametrize("name", ["row2_multi", "row7_ss", "general", "flanked_c9orf72", "dual_ggcccc"])
def test_window_in_a_ragged_batch_equals_the_window_alone(ctx, all_cases, models, name):
    c = all_cases[name]
    mid, plan = models(name)
    rng = np.random.default_rng(5)
    pool = [x for l, x in c.windows if len(x) >= 3]
    xs = []
    for i in range(70):
        x = pool[i % len(pool)]
        xs.append(x[:int(rng.integers(3, min(len(x), 400) + 1))])
    for mode in c.modes:
        if mode == vc.VIT_BACKPTR:
            continue
        batch = ctx.debug_viterbi_mode(mid, mode, xs)
        for i in (0, 33, 69):
            alone = ctx.debug_viterbi_mode(mid, mode, [xs[i]])
            assert alone["launched"] == batch["launched"]
            for k in ("logp", "counted", "status", "dbg"):
                assert alone[k][0].tobytes() == batch[k][i].tobytes(), (name, vc.MODE_NAMES[mode], i, k)
            if batch["records"][i] is not None:
                assert alone["records"][0].tobytes() == batch["records"][i].tobytes(), (name, vc.MODE_NAMES[mode], i)


def test_modes_the_library_does_not_launch_are_refused(ctx, all_cases, models):
    from strique_amd import ffi
    for name, mode in (("row6_ss", vc.VIT_UNIT), ("row0_ss", vc.VIT_HUB), ("general", vc.VIT_UNIT), ("general", vc.VIT_HUB), ("boundary_ss", vc.VIT_HUB)):
        mid, _ = models(name)
        with pytest.raises(ffi.StriqueHipError) as ei:
            ctx.debug_viterbi_mode(mid, mode, [all_cases[name].windows[2][1]])
        assert ei.value.code == ffi.STRQ_ERR_UNSUPPORTED, (name, mode)
    mid, _ = models("row6_ss")
    with pytest.raises(ffi.StriqueHipError) as ei:
        ctx.debug_viterbi_mode(mid, vc.VIT_BACKPTR, [all_cases["row6_ss"].windows[2][1]])
    assert ei.value.code == ffi.STRQ_ERR_ARG


def test_every_kernel_instance_is_launched(ctx, all_cases, models, capsys):
    """One short window per case and mode: the shape that runs is the planned one, and together the cases launch every
    (shape, single-stage, mode) the table of vit_model.h has an instance for.  The list goes to the log."""
    from strique_amd import ffi
    launched = set()
    for name in vc.CASE_NAMES:
        c = all_cases[name]
        mid, plan = models(name)
        x = next(x for l, x in c.windows if not l.startswith("nopath"))[:40]
        for mode in c.modes:
            if mode == vc.VIT_BACKPTR:
                continue
            if c.g2:
                launched.add((_launch(ctx, mid, mode, [x], ffi.VIT_SHAPE_G2, (name, mode))["launched"], mode))
                with options(ctx, {"STRQ_VIT_NO_G2": 1}):
                    launched.add((_launch(ctx, mid, mode, [x], plan["shape"], (name, mode))["launched"], mode))
            else:
                launched.add((_launch(ctx, mid, mode, [x], plan["shape"], (name, mode))["launched"], mode))
    with capsys.disabled():
        print("\nViterbi launches (row, single-stage, mode):")
        for shape, mode in sorted(launched):
            print("  row %d  ss %d  %s" % (shape & ~ffi.VIT_SHAPE_SS, 1 if shape & ffi.VIT_SHAPE_SS else 0, vc.MODE_NAMES[mode]))
    want = set()
    for row, modes in vc.ROW_MODES.items():
        for mode in modes:
            if mode != vc.VIT_BACKPTR:
                want |= {(row, mode)} if row >= ffi.VIT_SHAPE_CSR else {(row, mode), (row | ffi.VIT_SHAPE_SS, mode)}
    assert not (want - launched), sorted(want - launched)
