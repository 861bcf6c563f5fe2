"""State posteriors on the GPU (strq_forward_state_stats, strq_set_state_posteriors, repeatCounter.state_stats_batch(posterior=True),
`calibrate --posterior`) against tests/posterior_ref.py: log-space forward-backward in np.longdouble (the reference R) over the
oracle's UN-BAKED graphs, emitting states matched to the baked order by name.

Tolerance (the project's rule for a linear-space kernel against a log-space float64 run, tests/test_gpu_confidence.py; measured inside
the test, never taken from the code under test): per quantity q of log_lik, w, wx, wxx let E_q be the largest distance of the float64
run of the restatement from R over the cases of the test, the distance being |a - R| / max(1, |R|).  The GPU value must lie within
16 E_q of R, and never tighter than 4 ulp of R.

Measured on an MI355X over the windows of test_model_level_against_the_reference (the test prints them with -s):
    E_q                     log_lik 4.19e-14   w 2.71e-10   wx 2.68e-10   wxx 2.68e-10
    largest GPU distance    log_lik 3.43e-16   w 4.92e-14   wx 4.67e-14   wxx 4.45e-14
and in the pipeline on the two planted reads against R (E_q of the read itself): w 1.93e-10 and 3.50e-10, GPU distance 4.1e-14 and 8.2e-14.

Kernel instances (VIT_FWD_SHAPES), asserted with strq_debug_viterbi_plan: the four flanked models with 20 nt flanks and the three-state
model run on instance 1 (rows 2 and 1 of VIT_SHAPES), the flanked model with 50 nt flanks -- the size the pipeline decodes with -- on
instance 0 (row 7), the random model of 260 emitting and 130 silent states -- silent edges outside the chains, several rounds of the
silent phase -- on instance 2 (row 4).  Every instance is reached.
"""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest

import state_stats_ref as ssr
from conftest import oracle_tc
from forward_ref import sample_window
from posterior_ref import counted_occupancy, emitting_names, posterior_ref

pytestmark = pytest.mark.gpu

LEAVE = 0.05          # leave_repeat of the sampled models: a random walk then counts 3 ... 60 units, not ~500
FWD_OF_ROW = {0: 0, 1: 1, 2: 1, 3: 2, 4: 2, 5: 0, 6: 1, 7: 0}          # the `fwd` column of VIT_SHAPES
Q = ("log_lik", "w", "wx", "wxx")


def _dist(g, r):
    g, r = np.asarray(g, np.longdouble), np.asarray(r, np.longdouble)
    return float(np.max(np.abs(g - r) / np.maximum(1, np.abs(r)))) if g.size else 0.0


def _bound(E, r):
    """16 E_q, never tighter than 4 ulp of R (in the units of the distance)."""
    r = np.abs(np.asarray(r, np.float64))
    ulp4 = float(np.max(4 * np.spacing(r) / np.maximum(1, r))) if r.size else 0.0
    return max(16 * float(E), ulp4)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same(a, b):
    """log_lik, status, w, wx, wxx of two calls: the same bits."""
    return all(np.array_equal(_bits(x), _bits(y)) if np.asarray(x).dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def _ws_bytes(T, n_emit):
    return (T * ((n_emit + 63) // 64) * 64 * 8 + 4 * T + 15) & ~15


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


def _cut(x, L):
    """L observations of a sampled window: its head and its tail (both flanks stay in)."""
    return np.concatenate([x[:(L + 1) // 2], x[len(x) - L // 2:]]) if L < len(x) else x


def _tiny_model():
    """Two Normal states and a Uniform one, every one reachable from start and leading to end: a path exists at T = 1."""
    from strique_amd import hmm
    g = hmm.Graph()
    a = g.add_state("a", hmm.NORMAL, (80.0, 2.0)); b = g.add_state("b", hmm.NORMAL, (100.0, 3.0)); u = g.add_state("u", hmm.UNIFORM, (40.0, 160.0))
    for s, p in ((a, .5), (b, .3), (u, .2)):
        g.add_transition(g.start, s, p)
    for s in (a, b, u):
        for t, p in ((a, .3), (b, .3), (u, .2)):
            g.add_transition(s, t, p if s != t else p + .1)
        g.add_transition(s, g.end, .1)
    return hmm.bake(g, count_states=(b,))


@pytest.fixture(scope="module")
def cases(ctx, pm, opm, cfg, targets, orc):
    """Every (model, window) of the model-level tests with R, the float64 run and the GPU pass -- computed once, never changed.
    `prep`: the graph the reference runs on (the oracle's un-baked net; the baked arrays themselves for the two models that are
    no flanked nets); `idx`: the reference's emitting state of every baked one."""
    from oracle import hmm_oracle as ho
    from strique_amd import ffi, hmm
    from test_gpu_viterbi import _random_model
    hcfg = dict(cfg["HMM"], leave_repeat=LEAVE)
    rc = orc.revcomp
    out = []
    for mi, (name, strand, flank, config) in enumerate((("c9orf72", "+", 20, hcfg), ("c9orf72", "-", 20, hcfg), ("fmr1", "+", 20, hcfg),
                                                        ("gcg", "+", 20, {"leave_repeat": LEAVE}), ("c9orf72", "+", 50, hcfg))):
        repeat, prefix, suffix = targets["fmr1" if name == "gcg" else name]
        r, p, s = ("GCG" if name == "gcg" else repeat).upper(), prefix[-flank:].upper(), suffix[:flank].upper()
        if strand == "-":
            r, p, s = rc(r), rc(s), rc(p)
        net, _, offset = ho.flanked_net(r, p, s, opm, config)
        prep = ho.prepare(net)
        baked = hmm.FlankedRepeatModel(r, p, s, pm, config).baked
        if name == "gcg":
            assert offset != 0          # the repeat is shorter than the k-mer
        on, bn = emitting_names(prep), emitting_names(baked)
        assert sorted(on) == sorted(bn)
        out.append({"label": "%s%s/%d" % (name, strand, flank), "prep": prep, "baked": baked, "idx": np.array([on.index(nm) for nm in bn]), "fwd": 0 if flank == 50 else 1,
                    "rng": np.random.default_rng(9000 + mi), "long_flanks": flank == 50})
    tiny = _tiny_model()
    out.append({"label": "tiny", "prep": tiny, "baked": tiny, "idx": np.arange(tiny.silent_start), "fwd": 1, "rng": np.random.default_rng(9100), "long_flanks": False})
    rnd = _random_model(np.random.default_rng(760), 260, 130, True)
    inc = rnd.count_inc.copy(); inc[260:] = 0
    rnd = rnd._replace(count_inc=inc)
    out.append({"label": "random", "prep": rnd, "baked": rnd, "idx": np.arange(260), "fwd": 2, "rng": np.random.default_rng(9200), "long_flanks": False})
    for mi, m in enumerate(out):
        plan = ffi.debug_viterbi_plan(m["baked"])
        assert plan["csr"] == 0 and FWD_OF_ROW[plan["row"]] == m["fwd"], (m["label"], plan["row"])
        m["mid"] = ctx.model_create(m["baked"])
        prep, rng = m["prep"], m["rng"]
        if m["label"] == "random":          # (no walk from start to end worth sampling: uniform noise over the range of its levels)
            base = rng.uniform(55, 125, 150)
        elif m["label"] == "tiny":          # (a walk ends after ten observations: levels of its states, seven observations each)
            base = np.repeat(rng.choice([80.0, 100.0, 130.0], 22), 7)[:150] + rng.normal(0, 1.5, 150)
        else:
            lo_T, hi_T = (500, 900) if m["long_flanks"] else (140, 400)          # (a walk through 50 nt flanks emits more than 500 observations)
            base, _ = sample_window(prep, rng)
            while not lo_T <= len(base) <= hi_T:          # (the restatement costs a millisecond per observation in longdouble)
                base, _ = sample_window(prep, rng)
        tmin = next(T for T in range(1, 60) if posterior_ref(prep, np.full(T, np.nan), np.float64)[1] == 0)          # the shortest length with a path
        wins = [("T%d" % L, _cut(base, L)) for L in (0, 1, 2, tmin - 1, tmin, 63, 64, 65, 127, 128, 129)]          # every model, every instance
        wins.append(("sampled", base))
        wins.append(("all-nan", np.full(77, np.nan)))
        nans = base.copy(); nans[[0, len(base) // 3, len(base) - 1]] = np.nan
        wins.append(("nan-first-middle-last", nans))
        outside = base.copy(); outside[len(base) // 2] = opm.model_max + 1.5          # no insert (Uniform) can emit it; the Normals still can
        wins.append(("outside", outside))
        if mi == 0:
            long_x, v = sample_window(prep, np.random.default_rng(77), visits_exactly=80)
            assert 2500 <= len(long_x) <= 3500 and v >= 80, (len(long_x), v)
            wins.append(("long", long_x))
        m["wins"] = wins
    for m in out:          # one after the other: the restatement is a loop of small numpy calls, which threads only slow down
        m["R"] = [posterior_ref(m["prep"], x, np.longdouble) for _, x in m["wins"]]
        m["F"] = [posterior_ref(m["prep"], x, np.float64) for _, x in m["wins"]]
        m["gpu"] = ctx.forward_state_stats(m["mid"], [w for _, w in m["wins"]])
    return out


def _errors(cases):
    """E_q over all cases: float64 run of the restatement against R."""
    E = [0.0] * 4
    for m in cases:
        for r_, f_ in zip(m["R"], m["F"]):
            assert r_[1] == f_[1]
            if r_[1] == 0:
                for q, k in enumerate((0, 2, 3, 4)):
                    E[q] = max(E[q], _dist(f_[k], r_[k]))
    return E


def test_model_level_against_the_reference(cases):
    E = _errors(cases)
    worst = [0.0] * 4
    n_paths = n_none = 0
    for m in cases:
        ll, status, w, wx, wxx = m["gpu"]
        ne = m["baked"].silent_start
        assert w.shape == wx.shape == wxx.shape == (len(m["wins"]), ne) and w.dtype == np.float64
        for k, ((wname, x), r_) in enumerate(zip(m["wins"], m["R"])):
            tag = (m["label"], wname)
            assert status[k] == r_[1], tag
            if r_[1] != 0:          # no path: -inf and +0.0 rows exactly
                assert ll[k] == -np.inf and not _bits(w[k]).any() and not _bits(wx[k]).any() and not _bits(wxx[k]).any(), tag
                n_none += 1
                continue
            n_paths += 1
            got = (ll[k], w[k], wx[k], wxx[k])
            want = (r_[0], r_[2][m["idx"]], r_[3][m["idx"]], r_[4][m["idx"]])
            for q in range(4):
                d = _dist(got[q], want[q])
                worst[q] = max(worst[q], d)
                assert d <= _bound(E[q], want[q]), (tag, Q[q], d, _bound(E[q], want[q]))
            # sum_s gamma_t(s) = 1: the rows hold the observations that are numbers
            assert abs(w[k].sum() - np.count_nonzero(~np.isnan(x))) <= len(x) * 2.0 ** -40, tag
            assert (w[k] >= 0).all() and not np.isnan(wx[k]).any() and not np.isnan(wxx[k]).any(), tag
    print("E_q (float64 restatement vs longdouble): " + "  ".join("%s %.3g" % (n, e) for n, e in zip(Q, E)))
    print("largest GPU distance:                    " + "  ".join("%s %.3g" % (n, e) for n, e in zip(Q, worst)))
    assert n_none >= 3 * 5 and n_paths >= 7 * 7          # T = 0 .. 2 of every flanked model have no path



def test_long_window_underflows_a_double_many_times_over(cases):
    """~3000 observations: the likelihood is far below the smallest double, so the exponents of both halves have to combine."""
    m = cases[0]
    k = [n for n, _ in m["wins"]].index("long")
    ll, status, w, _, _ = m["gpu"]
    assert status[k] == 0 and ll[k] < 5 * np.log(np.finfo(np.float64).tiny)
    assert abs(w[k].sum() - len(m["wins"][k][1])) <= len(m["wins"][k][1]) * 2.0 ** -40


def test_agrees_with_the_forward_pass(cases, ctx):
    """GPU against GPU on the windows without NaN: log_lik, and the occupancy of the counted states against the visits_mean of
    strq_forward_batch with c0 = 0, within the bounds of the reference comparison: max(16 E_q, 4 ulp).  E of the mean: the float64
    restatement of the same quantity, the counted occupancy."""
    E = _errors(cases)
    checked = 0
    for m in cases:
        ll, status, w, _, _ = m["gpu"]
        pick = [k for k, (_, x) in enumerate(m["wins"]) if not np.isnan(x).any()]
        xs = [m["wins"][k][1] for k in pick]
        fll, fmean, _, fstatus = ctx.forward_batch(m["mid"], xs, np.zeros(len(xs), np.int64))
        counted = np.asarray(m["baked"].count_inc[:m["baked"].silent_start]) != 0
        Em = max([_dist(counted_occupancy(m["prep"], f_[2]), counted_occupancy(m["prep"], r_[2])) for r_, f_ in zip(m["R"], m["F"]) if r_[1] == 0] + [0.0])
        for j, k in enumerate(pick):
            tag = (m["label"], m["wins"][k][0])
            assert status[k] == fstatus[j], tag
            if status[k] != 0:
                assert fll[j] == -np.inf and ll[k] == -np.inf
                continue
            r_ = m["R"][k]
            assert _dist(ll[k], fll[j]) <= _bound(E[0], r_[0]), tag
            want = counted_occupancy(m["prep"], r_[2])
            assert abs(w[k][counted].sum() - fmean[j]) / max(1.0, abs(float(want))) <= _bound(Em, want), tag
            checked += 1
    assert checked >= 7 * 10


def test_the_same_bits_alone_together_reversed_and_in_pieces(cases, ctx):
    m = cases[0]
    names = [n for n, _ in m["wins"]]
    five = [names.index(n) for n in ("sampled", "T129", "nan-first-middle-last", "T64", "outside")]
    xs = [m["wins"][k][1] for k in five]
    base = tuple(a[five] for a in m["gpu"])
    together = ctx.forward_state_stats(m["mid"], xs)
    assert _same(together, base)
    back = ctx.forward_state_stats(m["mid"], xs[::-1])
    assert _same(tuple(a[::-1] for a in back), base)
    for j, x in enumerate(xs):
        assert _same(ctx.forward_state_stats(m["mid"], [x]), tuple(a[j:j + 1] for a in base)), j
    # five windows in three pieces: at most two of the three large ones fit a piece
    ne = m["baked"].silent_start
    size = sorted(_ws_bytes(len(x), ne) for x in xs)
    budget = size[-1] + size[-2]
    assert size[-1] + size[-2] + size[-3] > budget and size[0] + size[1] + size[2] > size[-3]
    ctx.set_option("STRQ_STATE_POST_WS_BYTES", str(budget))
    try:
        pieces = ctx.forward_state_stats(m["mid"], xs)
    finally:
        ctx.set_option("STRQ_STATE_POST_WS_BYTES", "")
    assert _same(pieces, base)


def test_a_window_over_the_budget(cases, ctx):
    """Status 4, zero rows and the likelihood it has anyway; its neighbours do not change by a bit."""
    m = cases[0]
    names = [n for n, _ in m["wins"]]
    pick = [names.index(n) for n in ("T129", "long", "sampled")]
    xs = [m["wins"][k][1] for k in pick]
    base = tuple(a[pick] for a in m["gpu"])
    ne = m["baked"].silent_start
    budget = _ws_bytes(len(xs[1]), ne) - 16
    assert budget >= _ws_bytes(len(xs[0]), ne) + _ws_bytes(len(xs[2]), ne)
    ctx.set_option("STRQ_STATE_POST_WS_BYTES", str(budget))
    try:
        ll, status, w, wx, wxx = ctx.forward_state_stats(m["mid"], xs)
    finally:
        ctx.set_option("STRQ_STATE_POST_WS_BYTES", "")
    assert status.tolist() == [0, 4, 0]
    assert np.array_equal(_bits(ll), _bits(base[0])) and np.isfinite(ll[1])
    assert not _bits(w[1]).any() and not _bits(wx[1]).any() and not _bits(wxx[1]).any()
    for j in (0, 2):
        assert _same((w[j], wx[j], wxx[j]), (base[2][j], base[3][j], base[4][j]))


def test_models_without_a_forward_kernel_are_refused(ctx):
    from strique_amd import ffi
    from test_gpu_viterbi import _random_model
    big = ctx.model_create(_random_model(np.random.default_rng(1), 600, 300, False))
    with pytest.raises(ffi.StriqueHipError, match="no lane layout") as ei:
        ctx.forward_state_stats(big, [np.full(5, 90.0)])
    assert ei.value.code == ffi.STRQ_ERR_UNSUPPORTED


# ---- pipeline ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(tables, cfg):
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    table, _ = ssr.planted_table(tables, repeat)
    reads = ssr.planted_reads(table, (repeat, prefix, suffix))
    # int16 and float64 reads: both affine sources
    items = [("c9orf72", np.asarray(sig) if r % 3 else np.asarray(sig).astype(np.float64), strand) for r, (sig, strand, _) in enumerate(reads)]
    assert {np.asarray(s).dtype for _, s, _ in items} == {np.dtype(np.int16), np.dtype(np.float64)}
    return items


@pytest.fixture(scope="module")
def counter(pm, cfg):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    rc.add_target("c9orf72", *cfg["repeat"]["c9orf72"][3:6])
    return rc


@pytest.fixture(scope="module")
def planted_refs(planted, orc, opm, cfg, targets):
    """Per planted read: the oracle's row and the window its decode saw, the float64 run of the restatement on the oracle's full-size
    un-baked model of the strand, and for the first two reads (one of each strand) R.  Computed once, never changed."""
    out = []
    for k, (name, sig, strand) in enumerate(planted):
        tc = oracle_tc(orc, opm, targets, name, strand, cfg["HMM"])
        row, x = ssr.oracle_window(orc, opm, cfg, tc, sig)
        assert x is not None
        out.append({"row": row, "x": x, "prep": tc["hmm"], "F": posterior_ref(tc["hmm"], x, np.float64),
                    "R": posterior_ref(tc["hmm"], x, np.longdouble) if k < 2 else None})
    return out


@pytest.fixture(scope="module")
def pipeline(counter, planted):
    """The six planted reads with the switch on, one read per sub-batch: state_stats_batch runs the four int16 reads and the two
    float64 reads as a device batch each, of four and of two sub-batches."""
    counter.ctx.set_option("STRQ_SUBBATCH_READS", "1")
    try:
        got = counter.state_stats_batch(planted, posterior=True)
        info = counter.ctx.last_state_posteriors()
    finally:
        counter.ctx.set_option("STRQ_SUBBATCH_READS", None)
    return got, info


def test_pipeline_rows_do_not_change_and_records_equal_the_model_level_call(counter, planted, pipeline, planted_refs):
    got, info = pipeline
    plain = counter.detect_batch(planted)
    assert [r for r, _ in got] == plain and all(r[0] > 0 for r in plain)          # every read decodes
    assert all(st is not None for _, st in got)
    assert info["windows"] > 0 and info["launches"] >= 3 and info["ws_bytes"] > 0 and info["ms"] > 0
    # the window the oracle derives, through the model-level call: the same bits
    for (name, sig, strand), (row, st), ref in zip(planted, got, planted_refs):
        x = ref["x"]
        assert tuple(row[:6]) == tuple(ref["row"][:6])
        model = counter.targets[name][0 if strand == "+" else 1].repeatHMM
        ll, status, w, wx, wxx = counter.ctx.forward_state_stats(model.model_id, [x])
        assert status[0] == 0
        assert _same((st[0], st[1], st[2], np.float64(st[3])), (w[0], wx[0], wxx[0], np.float64(ll[0]))), (name, strand)
        assert len(st[0]) == model.baked.silent_start and abs(st[0].sum() - len(x)) <= len(x) * 2.0 ** -40
    # two reads (one of each strand) against R on the oracle's full-size un-baked model
    for k in (0, 1):
        name, _, strand = planted[k]
        r_, f_ = planted_refs[k]["R"], planted_refs[k]["F"]
        baked = counter.targets[name][0 if strand == "+" else 1].repeatHMM.baked
        on, bn = emitting_names(planted_refs[k]["prep"]), emitting_names(baked)
        idx = np.array([on.index(nm) for nm in bn])
        st = got[k][1]
        for q, (g, kk) in enumerate(((st[3], 0), (st[0], 2), (st[1], 3), (st[2], 4))):
            want = r_[kk] if kk == 0 else r_[kk][idx]
            E = _dist(f_[kk], r_[kk])
            assert _dist(g, want) <= _bound(E, want), (k, Q[q], _dist(g, want), E)
            print("read %d %s: E %.3g, GPU distance %.3g" % (k, Q[q], E, _dist(g, want)))


def test_pipeline_switch_off_refuses_a_scan_and_launches_nothing(counter, planted, pipeline):
    from strique_amd import ffi
    ctx = counter.ctx
    assert counter.detect_batch(planted[:2]) == [r for r, _ in pipeline[0][:2]]
    assert ctx.last_state_posteriors() == {"ms": 0.0, "windows": 0, "launches": 0, "ws_bytes": 0.0}
    with pytest.raises(ffi.StriqueHipError, match=r"the last batch ran without state posteriors \(strq_set_state_posteriors\)"):
        ctx.batch_fetch_state_posteriors()
    ctx.set_state_posteriors(True)
    try:
        with pytest.raises(ffi.StriqueHipError, match=r"state-posteriors: not available in a scan \(strq_scan_set\)") as ei:
            counter.scan_batch([sig for _, sig, _ in planted[1:3]], min_score=3.0)
        assert ei.value.code == ffi.STRQ_ERR_ARG
    finally:
        ctx.set_state_posteriors(False)
    assert counter.detect_batch(planted[:2]) == [r for r, _ in pipeline[0][:2]]          # (and the scan mode is off again)


def test_pipeline_budget(counter, planted, pipeline):
    """STRQ_STATE_POST_WS_BYTES below the longest window of the int16 batch: that read has status 2 and no record, the others keep
    their bits; more pieces, a smaller peak."""
    got, whole = pipeline
    ints = [i for i, (_, sig, _) in enumerate(planted) if np.asarray(sig).dtype == np.int16]
    its = [planted[i] for i in ints]
    ne = counter.targets["c9orf72"][0].repeatHMM.baked.silent_start
    T = [int(round(got[i][1][0].sum())) for i in ints]
    longest = int(np.argmax(T))
    budget = _ws_bytes(sorted(T)[-1], ne) - 16
    assert budget >= _ws_bytes(sorted(T)[-2], ne)
    counter.ctx.set_option("STRQ_STATE_POST_WS_BYTES", str(budget))
    try:
        again = counter.state_stats_batch(its, posterior=True)
        status, stats = counter.ctx.batch_fetch_state_posteriors(with_status=True)
        info = counter.ctx.last_state_posteriors()
    finally:
        counter.ctx.set_option("STRQ_STATE_POST_WS_BYTES", "")
    assert status.tolist() == [2 if k == longest else 0 for k in range(len(its))]
    assert 0 < info["ws_bytes"] <= budget
    for k, i in enumerate(ints):
        assert again[k][0] == got[i][0]
        if k == longest:
            assert again[k][1] is None and stats[k] is None
        else:
            assert _same(again[k][1][:3] + (np.float64(again[k][1][3]),), got[i][1][:3] + (np.float64(got[i][1][3]),))


# ---- calibrate ---------------------------------------------------------------------------------------------------------------------
def test_calibrate_posterior_end_to_end(workdir, tables, cfg, orc, pm, planted_refs):
    """The six planted-shift c9orf72 reads through `calibrate --posterior`: the rows of --stats agree with pool_posterior / estimate
    over the float64 reference's records within the bound propagated to the mean, |d mean| <= 16 E max(1, |mean|); --out round-trips
    untouched k-mers exactly; the same command without the flag writes the bytes of the hard pass.  E is an estimate from the two reads
    that have a longdouble run (one of each strand), applied to rows pooled over all six; n_reads and `updated` are not compared
    where the restatement's own value lies within 1e-6 of the threshold that decides them."""
    import h5write
    from strique_amd import calibrate, cli, hmm
    from strique_amd.pore_model import pore_model
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    target = (repeat, prefix, suffix)
    planted_tab, _ = ssr.planted_table(tables, repeat)
    reads = ssr.planted_reads(planted_tab, target)
    named, sam = [], ["@HD\tVN:1.0"]
    for i, (sig, strand, _) in enumerate(reads):
        rid = "%08d-0000-4000-8000-%012d" % (i, i)
        named.append((rid, sig))
        sam.append("\t".join([rid, "16" if strand == "-" else "0", chrom, str(b - 3000), "60", "12S6000M5S", "*", "0", "0", "ACGT", "*"]))
    bulk = workdir / "bulk"; bulk.mkdir()
    (bulk / "batch_0.fast5").write_bytes(h5write.multi_read_fast5(named))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(bulk)])
    (bulk / "reads.fofn").write_text(buf.getvalue())
    (workdir / "aln.sam").write_text("\n".join(sam) + "\n")
    base = ["calibrate", str(bulk / "reads.fofn"), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"), "--config", str(workdir / "STRique.json"),
            "--algn", str(workdir / "aln.sam"), "--min-score", "3.0", "--min-obs", "200", "--batch", "4"]
    out, stats = workdir / "soft.model", workdir / "soft.tsv"
    cli.main(base + ["--out", str(out), "--stats", str(stats), "--posterior"])
    pm0 = pore_model(str(workdir / "r9_4_450bps.model"))
    # the float64 reference's records: the oracle's window, the restatement on the oracle's un-baked model of the strand (the shipped
    # table is the recorded one: the windows and models of planted_refs)
    shipped = (planted_tab[0], np.array(tables["base_mean"], np.float64), planted_tab[2])
    assert pm0.model_dict == pm.model_dict
    R, P, S = repeat.upper(), prefix[-50:].upper(), suffix[:50].upper()
    models = {"+": hmm.FlankedRepeatModel(R, P, S, pm, cfg["HMM"]), "-": hmm.FlankedRepeatModel(ssr.revcomp(R), ssr.revcomp(S), ssr.revcomp(P), pm, cfg["HMM"])}
    assert all(ref["row"][1] >= 3.0 and ref["row"][2] >= 3.0 for ref in planted_refs)
    E = max(_dist(ref["F"][q], ref["R"][q]) for ref in planted_refs[:2] for q in (2, 3, 4))
    records = []
    for (sig, strand, _), ref in zip(reads, planted_refs):
        m = models[strand]
        on, bn = emitting_names(ref["prep"]), emitting_names(m.baked)
        idx = np.array([on.index(nm) for nm in bn])
        records.append((m.state_kmers(), ref["F"][2][idx], ref["F"][3][idx], ref["F"][4][idx]))
    means, want = calibrate.estimate(calibrate.pool_posterior(records), pm0, 200)
    rows = calibrate.parse(stats.read_text())
    assert stats.read_text().splitlines()[0].split("\t")[2] == "exp_obs"
    by = {r[0]: r for r in rows}
    # per k-mer: its (read, state) entries -- every entry of the GPU lies within 16 E max(1, |entry|) of the restatement's -- and how
    # close a read's share comes to the one expected observation that decides n_reads
    entries, margin = {}, {}
    for what, w, _, _ in records:
        share = {}
        for (_, _, kmer), wi in zip(what, w):
            if kmer is not None:
                entries[kmer] = entries.get(kmer, 0) + 1
                share[kmer] = share.get(kmer, 0.0) + float(wi)
        for kmer, v in share.items():
            margin[kmer] = min(margin.get(kmer, 1.0), abs(v - 1.0))
    checked = 0
    for kmer, n_reads, W, mean, sd, t_mean, t_stdv, delta, upd in want:
        if W < 1.0:          # (no expected observation: nothing to estimate, and W > 0 itself may hang on rounding)
            continue
        g = by[kmer]
        assert abs(g[2] - W) <= 16 * E * entries[kmer] * max(1.0, W), (kmer, g[2], W)
        assert abs(g[3] - mean) <= 16 * E * max(1.0, abs(mean)), (kmer, g[3], mean, E)
        assert g[5:7] == (t_mean, t_stdv) and g[7] == g[3] - t_mean
        if margin[kmer] > 1e-6:
            assert g[1] == n_reads, kmer
        if abs(W - 200) > 1e-6:
            assert g[8] == upd, kmer
        checked += 1
    assert checked >= len(means) >= 6
    back = pore_model(str(out))
    updated = {r[0] for r in rows if r[8]}
    assert list(back.model_dict) == list(pm0.model_dict) and len(updated) >= 6
    for kmer, (mean, stdv) in pm0.model_dict.items():
        if kmer in updated:
            assert back.model_dict[kmer] == (by[kmer][3], stdv)
        else:
            assert back.model_dict[kmer] == (mean, stdv)          # exact: repr floats
    # without the flag: the bytes of the hard pass, which tests/test_gpu_state_stats.py pins to the reference statistics
    hard_out, hard_stats = workdir / "hard.model", workdir / "hard.tsv"
    cli.main(base + ["--out", str(hard_out), "--stats", str(hard_stats)])
    _, hrecords, _ = ssr.reference_records(orc, cfg, shipped, target, reads)
    hmeans, hrows = calibrate.estimate(calibrate.pool(hrecords), pm0, 200)
    hwant = workdir / "want.model"
    calibrate.write_model(str(hwant), pm0, hmeans)
    assert hard_out.read_bytes() == hwant.read_bytes() and hard_stats.read_bytes() == calibrate.format(hrows).encode()
    print("calibrate --posterior: E %.3g, %d k-mers updated (hard pass: %d)" % (E, len(updated), len(hmeans)))


from test_cli_end_to_end import workdir  # noqa: E402,F401  (model, config and repeat files in a temporary directory)
