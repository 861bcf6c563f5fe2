"""Count confidence on the GPU: strq_forward_batch, detect_batch(..., confidence=True) and `count --confidence` against the numpy
restatement of the definition in tests/forward_ref.py, run in np.longdouble (the reference R) over the oracle's UN-BAKED graphs.

Tolerance (set by the issue that asked for the feature, measured inside the test, never taken from the code under test): for each
quantity q let E_q be the largest distance of forward_ref's float64 run from R over the cases of the test -- relative for log_lik,
absolute for mean and sd.  The GPU value must lie within 16 E_q of R, and never tighter than 4 ulp of R's value.

Measured on an MI355X over the 91 windows of test_forward_batch_against_the_reference (the test prints them with -s):
    E_q                                   log_lik 5.42e-14 (relative)   mean 4.33e-09   sd 1.25e-06
    largest GPU distance, c0 NULL or 0    log_lik 2.03e-16              mean 9.19e-12   sd 1.01e-08
    largest GPU distance, c0 = Viterbi    log_lik 2.03e-16              mean 2.88e-12   sd 1.13e-08
(the restatement takes its moments about zero in log space: on the 320-unit window its own longdouble run carries ~1e-8 in the sd).
"""
import numpy as np
import pytest

from conftest import oracle_map, oracle_tc
from forward_ref import forward_ref, sample_window

pytestmark = pytest.mark.gpu

LEAVE = 0.05          # leave_repeat of the sampled models: a random walk then counts 3 ... 60 units, not ~500


def _dist(g, r, relative):
    g, r = np.longdouble(g), np.longdouble(r)
    d = abs(g - r)
    return d / abs(r) if relative else d


def _bound(E, r, relative):
    """16 E_q, never tighter than 4 ulp of R's value (as a float64)."""
    ulp4 = 4 * np.longdouble(np.spacing(abs(np.float64(r))))
    return max(16 * np.longdouble(E), ulp4 / abs(np.longdouble(r)) if relative else ulp4)


@pytest.fixture(scope="module")
def ctx():
    from strique_amd import ffi
    return ffi.Context(0)


def _cut(x, L):
    """L observations of a sampled window: its head and its tail (both flanks stay in)."""
    return np.concatenate([x[:(L + 1) // 2], x[len(x) - L // 2:]]) if L < len(x) else x


@pytest.fixture(scope="module")
def cases(ctx, pm, opm, cfg, targets, orc):
    """Every (model, window) of the model-level tests with R, the float64 run, the Viterbi decode and the GPU forward pass for
    c0 = NULL, 0 and the Viterbi visits -- computed once."""
    from oracle import hmm_oracle as ho
    from strique_amd import hmm
    hcfg = dict(cfg["HMM"], leave_repeat=LEAVE)
    rc = orc.revcomp
    specs = []
    for name, strand, flank, config in (("c9orf72", "+", 20, hcfg), ("c9orf72", "-", 20, hcfg), ("fmr1", "+", 20, hcfg), ("htt", "+", 20, hcfg),
                                        ("gcg", "+", 20, {"leave_repeat": LEAVE}), ("c9orf72", "+", 50, hcfg)):
        repeat, prefix, suffix = targets["fmr1" if name == "gcg" else name]
        repeat = "GCG" if name == "gcg" else repeat
        r, p, s = repeat.upper(), prefix[-flank:].upper(), suffix[:flank].upper()
        if strand == "-":
            r, p, s = rc(r), rc(s), rc(p)
        specs.append(("%s%s/%d" % (name, strand, flank), r, p, s, config))
    out = []
    for mi, (label, r, p, s, config) in enumerate(specs):
        net, _, offset = ho.flanked_net(r, p, s, opm, config)
        prep = ho.prepare(net)
        mid = ctx.model_create(hmm.FlankedRepeatModel(r, p, s, pm, config).baked)
        rng = np.random.default_rng(9000 + mi)
        base, _ = sample_window(prep, rng)
        while not 140 <= len(base) <= 400:          # (the restatement costs a millisecond per observation in longdouble)
            base, _ = sample_window(prep, rng)
        lo, hi = opm.model_min, opm.model_max
        tmin = next(T for T in range(1, 40) if forward_ref(prep, np.full(T, np.nan), np.float64)[3] == 0)
        wins = [("T%d" % L, _cut(base, L)) for L in (0, 1, 2, tmin - 1, tmin, 63, 64, 65, 127, 128, 129)]
        wins.append(("sampled", base))
        wins.append(("all-nan", np.full(77, np.nan)))
        one_nan = base.copy(); one_nan[len(base) // 3] = np.nan
        wins.append(("one-nan", one_nan))
        outside = base.copy(); outside[len(base) // 2] = hi + 1.5          # no insert (Uniform) can emit it; the Normals still can
        wins.append(("outside", outside))
        if mi == 0:
            long_x, v = sample_window(prep, np.random.default_rng(77), visits_exactly=320)
            assert 10000 <= len(long_x) <= 12000 and v >= 200, (len(long_x), v)
            wins.append(("long", long_x))
        if mi == 3:
            assert offset != 0          # the repeat is shorter than the k-mer
        out.append({"label": label, "prep": prep, "mid": mid, "wins": wins})
    jobs = [(m, k) for m in range(len(out)) for k in range(len(out[m]["wins"]))]
    R = oracle_map(lambda j: forward_ref(out[j[0]]["prep"], out[j[0]]["wins"][j[1]][1], np.longdouble), jobs)
    F = oracle_map(lambda j: forward_ref(out[j[0]]["prep"], out[j[0]]["wins"][j[1]][1], np.float64), jobs)
    for m in out:
        m["R"], m["F"] = [], []
    for (mi, k), r_, f_ in zip(jobs, R, F):
        out[mi]["R"].append(r_); out[mi]["F"].append(f_)
    for m in out:
        xs = [w for _, w in m["wins"]]
        m["vit"] = ctx.viterbi_batch(m["mid"], xs)
        visits = np.where(m["vit"][2] == 0, m["vit"][1], 0)
        m["gpu"] = {"null": ctx.forward_batch(m["mid"], xs), "zero": ctx.forward_batch(m["mid"], xs, np.zeros(len(xs), np.int64)),
                    "viterbi": ctx.forward_batch(m["mid"], xs, visits)}
    return out


def _errors(cases):
    """E_q over all cases: float64 run of the restatement against R."""
    E = [0, 0, 0]
    for m in cases:
        for r_, f_ in zip(m["R"], m["F"]):
            assert r_[3] == f_[3]
            if r_[3] == 0:
                for q in range(3):
                    E[q] = max(E[q], _dist(f_[q], r_[q], q == 0))
    return E


def test_forward_batch_against_the_reference(cases):
    E = _errors(cases)
    worst = {k: [0, 0, 0] for k in ("null", "zero", "viterbi")}
    n_paths = n_none = 0
    for m in cases:
        for key, (ll, mean, var, status) in m["gpu"].items():
            for k, ((wname, x), r_) in enumerate(zip(m["wins"], m["R"])):
                tag = (m["label"], wname, key)
                if r_[3] != 0:          # no path: status and the -inf / NaN pattern exactly
                    assert status[k] == 1 and ll[k] == -np.inf and np.isnan(mean[k]) and np.isnan(var[k]), tag
                    n_none += 1
                    continue
                n_paths += 1
                assert status[k] == 0 and np.isfinite(ll[k]), tag
                got = (ll[k], mean[k], np.sqrt(var[k]))
                for q in range(3):
                    d = _dist(got[q], r_[q], q == 0)
                    worst[key][q] = max(worst[key][q], d)
                    assert d <= _bound(E[q], r_[q], q == 0), (tag, "log_lik mean sd".split()[q], float(d), float(_bound(E[q], r_[q], q == 0)), got[q], r_[q])
    print("E_q (float64 restatement vs longdouble): log_lik %.3g (relative), mean %.3g, sd %.3g" % tuple(float(e) for e in E))
    for key, w in worst.items():
        print("largest GPU distance, c0 = %-8s: log_lik %.3g (relative), mean %.3g, sd %.3g" % ((key,) + tuple(float(e) for e in w)))
    assert n_none >= 3 * 6 * 3 and n_paths >= 3 * 6 * 8          # T = 0, 1, 2 (at least) of every model have no path


def test_inequalities_and_range(cases):
    E = _errors(cases)
    for m in cases:
        vlogp, _, vstatus, _ = m["vit"]
        for key, (ll, mean, var, status) in m["gpu"].items():
            for k, (wname, x) in enumerate(m["wins"]):
                tag = (m["label"], wname, key)
                assert (status[k] == 0) == (vstatus[k] == 0), tag          # a best path exists exactly when any path does
                if status[k] != 0:
                    continue
                assert ll[k] >= vlogp[k] - float(_bound(E[0], ll[k], True)) * abs(ll[k]), tag
                assert 0.0 <= mean[k] <= len(x), tag
                assert var[k] >= 0.0 and not np.isnan(np.sqrt(var[k])), tag


def test_rescale_interval_and_batch_composition_do_not_change_a_bit(cases, ctx):
    """A power of two scales exactly: rescaling every 4th or 7th step gives the bits of rescaling every step, the long window
    included; so does running a window alone instead of in its batch."""
    m = cases[0]
    xs = [w for _, w in m["wins"]]
    visits = np.where(m["vit"][2] == 0, m["vit"][1], 0)
    base = m["gpu"]["viterbi"]
    for every in ("4", "7"):
        ctx.set_option("STRQ_FWD_RESCALE_EVERY", every)
        try:
            got = ctx.forward_batch(m["mid"], xs, visits)
        finally:
            ctx.set_option("STRQ_FWD_RESCALE_EVERY", None)
        for a, b in zip(got, base):
            assert a.tobytes() == b.tobytes(), every
    k = [n for n, _ in m["wins"]].index("sampled")
    alone = ctx.forward_batch(m["mid"], [xs[k]], visits[k:k + 1])
    assert all(a[0].tobytes() == b[k].tobytes() for a, b in zip(alone, base))
    again = ctx.forward_batch(m["mid"], xs, visits)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, base))


@pytest.mark.parametrize("ne,ns,multi", [(40, 10, False), (64, 20, True), (130, 40, True), (260, 130, True)])
def test_random_models_every_lane_layout(ctx, ne, ns, multi):
    """Models without layout hints, with silent edges outside the chains (several rounds of the silent phase) and up to four silent
    slots per lane, against the restatement on the same baked arrays; models the lane layouts do not cover are refused."""
    from strique_amd import ffi
    from test_gpu_viterbi import _random_model
    rng = np.random.default_rng(500 + ne)
    baked = _random_model(rng, ne, ns, multi)
    inc = baked.count_inc.copy(); inc[ne:] = 0
    baked = baked._replace(count_inc=inc)
    mid = ctx.model_create(baked)
    xs = [rng.uniform(55, 125, T) for T in (1, 7, 64, 150)]
    ll, mean, var, status = ctx.forward_batch(mid, xs, ctx.viterbi_batch(mid, xs)[1])
    for k, x in enumerate(xs):
        r_ = forward_ref(baked, x, np.longdouble)
        f_ = forward_ref(baked, x, np.float64)
        assert status[k] == r_[3]
        if r_[3] == 0:
            got = (ll[k], mean[k], np.sqrt(var[k]))
            for q in range(3):
                assert _dist(got[q], r_[q], q == 0) <= _bound(_dist(f_[q], r_[q], q == 0), r_[q], q == 0), (k, q, got[q], r_[q])
    if ne == 260:
        big = ctx.model_create(_random_model(rng, 600, 300, False))
        with pytest.raises(ffi.StriqueHipError, match="no lane layout") as ei:
            ctx.forward_batch(big, xs[:1])
        assert ei.value.code == ffi.STRQ_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
def _pipeline_items(pm, targets):
    from strique_amd import synth
    table = synth.KmerTable(pm)
    items = []
    for k, (name, strand, n) in enumerate((("c9orf72", "+", 31), ("c9orf72", "-", 12), ("fmr1", "+", 45), ("fmr1", "-", 20))):
        items.append((name, synth.make_read(table, 9, 4100 + k, 5000, targets[name], n, strand=strand, as_int16=True)[0], strand))
    rng = np.random.default_rng(3)
    items.insert(1, ("c9orf72", rng.integers(200, 800, 6000).astype(np.int16), "-"))          # no flank: the gate fails
    items.insert(3, ("fmr1", np.full(5000, 300, np.int16), "+"))                              # constant: not normalised
    return items


def _same_conf(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array(x).tobytes() == np.array(y).tobytes())
                                    for x, y in zip(a, b))


def test_detect_batch_confidence(gpu_counter, pm, opm, cfg, orc, targets):
    rc = gpu_counter
    items = _pipeline_items(pm, targets)
    plain = rc.detect_batch(items)
    got = rc.detect_batch(items, confidence=True)
    assert [r for r, _ in got] == plain                                   # the rows do not change
    confs = [c for _, c in got]
    decoded = [c is not None for c in confs]
    assert decoded == [True, confs[1] is not None, True, False, True, True] and (confs[1] is not None or plain[1][0] == 0)
    assert sum(decoded) >= 4
    # the window the oracle derives, through the model-level call: the same bits
    tcs = [oracle_tc(orc, opm, targets, n, s, cfg["HMM"]) for n, _, s in items]
    params = orc.align_params(cfg["align"])
    refs = []
    for (name, sig, strand), tc, row, conf in zip(items, tcs, plain, confs):
        if conf is None:
            refs.append(None); continue
        _, info = orc.detect(sig, tc, opm, params)
        x = orc.condition(np.asarray(sig), opm)[3][info["prefix_begin"]:info["suffix_end"]]
        ptc = rc._classifier_for(name, strand)
        bias = ptc.repeatHMM.count_bias
        ll, mean, var, status = rc.ctx.forward_batch(ptc.repeatHMM.model_id, [x], [row[0] - bias])
        assert status[0] == 0
        assert np.array(conf).tobytes() == np.array([ll[0], float(bias) + mean[0], np.sqrt(var[0])]).tobytes(), (name, strand)
        assert conf[0] >= row[3] - 1e-9 * abs(row[3]) and abs(conf[1] - row[0]) < 5 * max(conf[2], 1.0)
        refs.append((tc, x, bias))
    # two of the reads against R on the oracle's full-size un-baked model
    two = [k for k, r in enumerate(refs) if r is not None][:2]
    R = oracle_map(lambda k: forward_ref(refs[k][0]["hmm"], refs[k][1], np.longdouble), two)
    F = oracle_map(lambda k: forward_ref(refs[k][0]["hmm"], refs[k][1], np.float64), two)
    for k, r_, f_ in zip(two, R, F):
        want = (r_[0], r_[1] + refs[k][2], r_[2])
        for q in range(3):
            E = _dist(f_[q], r_[q], q == 0)
            assert _dist(confs[k][q], want[q], q == 0) <= _bound(E, want[q], q == 0), (k, q, confs[k][q], want[q], float(E))
    # every route: the same bits, rows and unit positions
    units = rc.detect_batch(items, units=True)
    for key, value in (("STRQ_SERIAL", "1"), ("STRQ_SUBBATCH_READS", "2"), (None, None), (None, None)):
        if key:
            rc.ctx.set_option(key, value)
        try:
            again = rc.detect_batch(items, confidence=True)
        finally:
            if key:
                rc.ctx.set_option(key, None)          # the entry removed, not set to "unset": the counter is the session's, and later tests switch through the environment
        assert [r for r, _ in again] == plain and _same_conf([c for _, c in again], confs), key
    both = rc.detect_batch(items, units=True, confidence=True)
    assert [r for r, _, _ in both] == plain and _same_conf([c for _, _, c in both], confs)
    assert all((p is None and q is None) or np.array_equal(p, q) for (_, p, _), (_, q) in zip(both, units))
    info = rc.ctx.last_confidence()
    assert info["windows"] == sum(decoded) and info["no_path"] == 0 and info["ms"] > 0 and info["max_exponent"] > 100
    # off again: no forward pass, and fetching its results is an error
    from strique_amd import ffi
    assert rc.detect_batch(items) == plain
    with pytest.raises(ffi.StriqueHipError) as ei:
        rc.ctx.batch_fetch_confidence()
    assert ei.value.code == ffi.STRQ_ERR_ARG


def test_count_confidence_on_the_bundled_read(workdir):
    """`count --confidence` on tests/golden/c9orf72.{fast5,sam}: the count TSV is byte-identical to a run without the flag; one
    confidence row, whose count and log_p are the TSV's."""
    from strique_amd import cli
    from test_cli_end_to_end import _index
    fofn = workdir / "data" / "reads.fofn"
    fofn.write_text(_index(workdir))
    base = [str(fofn), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"),
            "--config", str(workdir / "STRique.json"), "--algn", str(workdir / "data" / "c9orf72.sam")]
    plain, with_conf, conf = workdir / "plain.tsv", workdir / "with.tsv", workdir / "conf.tsv"
    cli.main(["count"] + base + ["--out", str(plain)])
    cli.main(["count"] + base + ["--out", str(with_conf), "--confidence", str(conf)])
    assert with_conf.read_bytes() == plain.read_bytes()
    rows = plain.read_text().splitlines()[1:]
    crows = cli.parse_confidence(open(conf))
    assert len(crows) == len(rows) == 1
    f = rows[0].split("\t")
    rid, target, strand, count, log_p, c = crows[0]
    assert (rid, target, strand, str(count)) == tuple(f[:4]) and conf.read_text().splitlines()[1].split("\t")[4] == f[6]
    assert c is not None
    print("bundled read: count %d log_p %r log_lik %r count_mean %r count_sd %r" % (count, log_p, c[0], c[1], c[2]))
    assert c[0] >= log_p
    assert abs(c[1] - count) < 5 * max(c[2], 1.0)


from test_cli_end_to_end import workdir  # noqa: E402,F401  (the bundled fast5 / SAM / model files in a temporary directory)
