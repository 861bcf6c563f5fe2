"""The shared host code of the re-decode passes on the GPU: what the window-batch preamble of the standalone HMM entry points refuses,
and the traced re-decode (state statistics, tract positions) on pieces that hold windows of two kernel shapes -- six reads with the two
targets interleaved (the state statistics take them in read order, so the tasks of a piece are not in the order of its windows; the
tract positions take them as the tract decode grouped them) -- at the default budget, at a budget of exactly
two windows' back-pointers and at one that leaves the longest window out.  Expected values: tests/state_stats_ref.py and
tests/tract_pos_ref.py on the product's baked arrays, bit for bit; the pieces, launches and peak bytes from the piece rule written out
below (a piece takes windows in input order while their 16-byte-rounded back-pointers fit the budget; per piece one sort,
one decode and one traceback per kernel shape, and one consumer kernel)."""
import ctypes

import numpy as np
import pytest

import state_stats_ref as ssr
import tract_pos_cases as tpc
import tract_pos_ref as tpr
import tract_ref as tr
import vit_mode_cases as vc
from conftest import oracle_map

pytestmark = pytest.mark.gpu

LONG_UNIT = "GGCCCCTTAGCA"          # a 12-nt unit: its flanked model has more emitting slots per lane than a 3- or 6-nt unit's


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


# ---- argument refusals -------------------------------------------------------------------------------------------------------------
def _viterbi_batch(ctx, mid, x, off):
    from strique_amd import ffi
    n = len(off) - 1
    x = np.ascontiguousarray(x, np.float64); off = np.ascontiguousarray(off, np.int64)
    logp = np.zeros(n); counted = np.zeros(n, np.int64); status = np.full(n, -1, np.int32)
    rc = ctx._lib.strq_viterbi_batch(ctx._h, ctypes.c_int32(mid), ctypes.c_int64(n), ffi._ptr(x), ffi._ptr(off), ffi._ptr(logp), ffi._ptr(counted),
                                     ffi._ptr(status), None)
    return rc, ctx._lib.strq_last_error(ctx._h).decode(), logp, counted, status


def test_viterbi_batch_refuses_offsets_that_decrease_or_start_below_zero(ctx, pm, cfg):
    from strique_amd import ffi, hmm
    repeat, prefix, suffix = cfg["repeat"]["c9orf72"][3:6]
    m = hmm.FlankedRepeatModel(repeat.upper(), prefix[-50:].upper(), suffix[:50].upper(), pm, cfg["HMM"])
    mid = ctx.model_create(m.baked)
    x = np.linspace(-1.0, 1.0, 8)
    for off in ([0, 5, 3], [-1, 4]):
        rc, msg, _, _, status = _viterbi_batch(ctx, mid, x, off)
        assert rc == ffi.STRQ_ERR_ARG and msg == "bad argument (x_off must not decrease)", (off, rc, msg)
        assert (status == -1).all()          # nothing was decoded
    # the context decodes as before: the same windows through the raw entry and through the wrapper
    rc, _, logp, counted, status = _viterbi_batch(ctx, mid, x, [0, 5, 8])
    assert rc == ffi.STRQ_OK
    wl, wc, ws, _ = ctx.viterbi_batch(mid, [x[:5], x[5:]])
    assert logp.tobytes() == np.asarray(wl, np.float64).tobytes() and np.array_equal(counted, wc) and np.array_equal(status, ws) and set(status.tolist()) <= {0, 1}


def test_entries_refuse_a_null_context():
    from strique_amd import ffi
    lib = ffi.load_library()
    x = np.zeros(4); logp = np.zeros(1); counted = np.zeros(1, np.int64); status = np.zeros(1, np.int32)
    kind = np.zeros(4, np.int32)
    assert lib.strq_viterbi(None, ctypes.c_int32(0), ffi._ptr(x), ctypes.c_int64(4), ffi._ptr(logp), ffi._ptr(counted), ffi._ptr(status), None) == ffi.STRQ_ERR_ARG
    assert lib.strq_model_set_positions(None, ctypes.c_int32(0), ffi._ptr(kind), ffi._ptr(kind)) == ffi.STRQ_ERR_ARG
    off = np.array([0, 4], np.int64)
    assert lib.strq_viterbi_batch(None, ctypes.c_int32(0), ctypes.c_int64(1), ffi._ptr(x), ffi._ptr(off), ffi._ptr(logp), ffi._ptr(counted), ffi._ptr(status), None) == ffi.STRQ_ERR_ARG


# ---- two kernel shapes in one piece ------------------------------------------------------------------------------------------------
def bp_bytes(T, n_states):
    return ((T + 1) * n_states * 2 + 15) & ~15


def pieces_of(sizes, shapes, budget, order):
    """The piece rule of the traced re-decode on the windows in the order the pass hands them in: (status per window, windows traced,
    launches, peak bytes of a piece).  A window over the budget alone is left out (status 2)."""
    status = [2 if s > budget else 0 for s in sizes]
    kept = [i for i in order if not status[i]]
    launches = peak = 0
    at = 0
    while at < len(kept):
        end, total = at, 0
        while end < len(kept) and total + sizes[kept[end]] <= budget:
            total += sizes[kept[end]]; end += 1
        launches += 3 * len({shapes[i] for i in kept[at:end]}) + 1
        peak = max(peak, total)
        at = end
    return status, len(kept), launches, peak


def budgets_of(sizes, order):
    """None (the default), exactly the first two windows' back-pointers, and 16 bytes short of the largest window."""
    two, short = sizes[order[0]] + sizes[order[1]], max(sizes) - 16
    assert max(sizes) <= two and sorted(sizes)[-2] <= short          # the first leaves no window out, the second exactly one
    return [None, two, short]


def backptr_shape(baked):
    from strique_amd import ffi
    plan = ffi.debug_viterbi_plan(baked)
    assert vc.VIT_BACKPTR in plan["modes"]
    return plan["shapes"][vc.VIT_BACKPTR]


@pytest.fixture(scope="module")
def stats_case(pm, opm, orc, cfg):
    """Six int16 reads of 3.5 kb, c9orf72 and a target with a 12-nt unit in turn, the last one with the longest array: per read
    the item, the oracle's row, the reference statistics on the product's flanked model, the window's back-pointer bytes and shape."""
    from strique_amd import hmm, synth
    table = synth.KmerTable(pm)
    prefix, suffix = cfg["repeat"]["c9orf72"][4:6]
    repeats = {"c9orf72": cfg["repeat"]["c9orf72"][3], "long12": LONG_UNIT}
    jobs = []
    for k, (name, strand, units) in enumerate((("c9orf72", "+", 5), ("long12", "+", 4), ("c9orf72", "-", 7), ("long12", "-", 6), ("c9orf72", "+", 9), ("long12", "+", 10))):
        sig = synth.make_read(table, 9, 5200 + k, 3500, (repeats[name], prefix, suffix), units, strand=strand, as_int16=True)[0]
        R, P, S = repeats[name].upper(), prefix[-50:].upper(), suffix[:50].upper()
        if strand == "-":
            R, P, S = ssr.revcomp(R), ssr.revcomp(S), ssr.revcomp(P)
        model = hmm.FlankedRepeatModel(R, P, S, pm, cfg["HMM"])
        tc = orc.classifier(repeats[name], prefix, suffix, strand, opm, None, cfg["HMM"])
        jobs.append(((name, sig, strand), tc, model))

    def one(job):
        item, tc, model = job
        row, x = ssr.oracle_window(orc, opm, cfg, tc, item[1])
        assert x is not None, (item[0], item[2], row)
        ref = ssr.reference(orc, model.baked, x)
        assert ref[2] == 0, (item[0], item[2])
        return item, row, ref, bp_bytes(len(x), model.baked.n_states), backptr_shape(model.baked)

    return repeats, (prefix, suffix), oracle_map(one, jobs)


def test_state_stats_of_two_kernel_shapes_in_one_piece(pm, cfg, stats_case):
    from strique_amd.counter import repeatCounter
    repeats, (prefix, suffix), reads = stats_case
    items = [r[0] for r in reads]; sizes = [r[3] for r in reads]; shapes = [r[4] for r in reads]
    assert len(set(shapes)) == 2 and shapes[0] != shapes[1] and sizes.index(max(sizes)) == 5          # the shapes alternate with the targets
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in sorted(repeats):
        rc.add_target(name, repeats[name], prefix, suffix)
    order = list(range(6))          # the pass takes the decoded reads in read order
    for budget in budgets_of(sizes, order):
        want_status, windows, launches, peak = pieces_of(sizes, shapes, budget if budget else 8 << 30, order)
        rc.ctx.set_option("STRQ_STATE_STATS_WS_BYTES", "" if budget is None else str(budget))
        try:
            got = rc.state_stats_batch(items)
            info = rc.ctx.last_state_stats()
            status, stats = rc.ctx.batch_fetch_state_stats(with_status=True)
        finally:
            rc.ctx.set_option("STRQ_STATE_STATS_WS_BYTES", "")
        print("state-stats, budget", budget, info, "want", (windows, launches, peak))
        assert status.tolist() == want_status, budget
        assert (info["windows"], info["launches"], info["bp_bytes"]) == (windows, launches, peak), (budget, info)
        if budget is None:
            assert launches == 7 and peak == sum(sizes)          # one piece: (sort, decode, traceback) per shape, one statistics kernel
        for i, ((row, st), (_, orow, ref, _, _)) in enumerate(zip(got, reads)):
            assert tuple(row[:6]) == tuple(orow[:6]), (budget, i)
            if want_status[i]:
                assert st is None and stats[i] is None, (budget, i)
            else:
                assert ssr.same_rows(st, ref[3:]) and ssr.same_rows(stats[i], ref[3:]), (budget, i)


@pytest.fixture(scope="module")
def tracts_case(pm, opm, orc, cfg):
    """Six reads of the two compound loci in turn on 50-nt flanks (compound models on lane kernels of two shapes), the last one with
    by far the longest array: per read the item, the oracle's row, the reference record on the product's compound model, the window's
    back-pointer bytes and shape."""
    from strique_amd import hmm, synth, tracts
    table = synth.KmerTable(pm)
    full_p, full_s = tpc.full_flanks(cfg)
    prefix, suffix = full_p[-50:], full_s[:50]
    params = orc.align_params(cfg["align"])
    plan = [("htt_like", "+", (12, 7)), ("cnbp_like", "+", (9, 6, 11)), ("htt_like", "-", (5, 9)), ("cnbp_like", "-", (6, 10, 7)), ("htt_like", "+", (8, 8)),
            ("cnbp_like", "+", (16, 12, 14))]
    jobs = []
    for i, (target, strand, planted) in enumerate(plan):
        sig = tpc.pipeline_signal(table, cfg, i, target, strand, planted, "read")
        un, li = tracts.strand_definition(*tr.LOCI[target], strand)
        p, s = (prefix, suffix) if strand == "+" else (ssr.revcomp(suffix), ssr.revcomp(prefix))
        cm = hmm.CompoundRepeatModel(un, li, p, s, pm, cfg["HMM"])
        tc = orc.classifier(tpc.FLANKED_REPEAT[target], prefix, suffix, strand, opm, None, cfg["HMM"])
        jobs.append(((target, sig, strand), tc, cm))

    def one(job):
        item, tc, cm = job
        row, b, x = tpr.window(item[1], tc, opm, params)
        rec = tpr.record_on(cm.baked, cm.tract_of, cm.n_tracts, list(cm.count_bias), item[2], b, x)
        assert rec is not None, (item[0], item[2], row)
        return item, row, rec, bp_bytes(len(x), cm.baked.n_states), backptr_shape(cm.baked)

    return (prefix, suffix), oracle_map(one, jobs)


def test_tract_positions_of_two_kernel_shapes_in_one_piece(pm, cfg, tracts_case):
    from strique_amd.counter import repeatCounter
    (prefix, suffix), reads = tracts_case
    items = [r[0] for r in reads]; sizes = [r[3] for r in reads]; shapes = [r[4] for r in reads]
    assert len(set(shapes)) == 2 and shapes[0] != shapes[1] and sizes.index(max(sizes)) == 5
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name in sorted(tr.LOCI):
        rc.add_target(name, tpc.FLANKED_REPEAT[name], prefix, suffix, tracts=tr.LOCI[name])
    rc.set_tracts(True, positions=True)
    # the pass takes its windows as the tract decode had its tasks: by ascending kernel shape, in read order within a shape (group_items)
    order = sorted(range(6), key=lambda i: (shapes[i], i))
    for budget in budgets_of(sizes, order):
        want_status, windows, launches, peak = pieces_of(sizes, shapes, budget if budget else 8 << 30, order)
        rc.ctx.set_option("STRQ_TRACT_POS_WS_BYTES", None if budget is None else str(budget))
        try:
            got = rc.detect_batch(items, records=True)
            info = rc.ctx.last_tract_positions()
        finally:
            rc.ctx.set_option("STRQ_TRACT_POS_WS_BYTES", None)
        print("tract positions, budget", budget, info, "want", (windows, launches, peak))
        assert (info["windows"], info["launches"], info["bp_bytes"]) == (windows, launches, peak), (budget, info)
        if budget is None:
            assert launches == 7 and peak == sum(sizes)          # one piece: (sort, decode, traceback) per shape, one scan kernel
        for i, (d, (_, orow, rec, _, _)) in enumerate(zip(got, reads)):
            assert tuple(d.row[:6]) == tuple(orow[:6]), (budget, i)
            assert d.tracts is not None and tuple(d.tracts[0]) == tuple(rec[0]) and np.float64(d.tracts[1]).tobytes() == np.float64(rec[1]).tobytes(), (budget, i)
            if want_status[i]:
                assert d.tracts[2] is None, (budget, i)
            else:
                assert d.tracts[2] is not None and tpr.same_positions(d.tracts[2], rec[2]), (budget, i)
