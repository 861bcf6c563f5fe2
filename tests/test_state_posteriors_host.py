"""State posteriors without a device: the tests' reference (tests/posterior_ref.py) against brute-force path enumeration and against
the identities of the rule (strique_amd/state_posteriors.py), the host side of `calibrate --posterior`, its command line, and the ABI."""
import ctypes
import math
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from forward_ref import forward_ref, sample_window
from posterior_ref import brute_force, counted_occupancy, emitting_names, posterior_ref

LEAVE = 0.05


# ---- the reference against brute force ---------------------------------------------------------------------------------------------
def _toy():
    """A two-state loop A -> (silent mid) -> B -> A with a Uniform insert I: emitting A, B, I = 0, 1, 2; silent start, mid, end = 3, 4, 5."""
    A, B, I, START, MID, END = range(6)
    edges = [(START, A, .7), (START, I, .3), (A, A, .2), (A, MID, .5), (A, I, .2), (A, END, .1), (MID, B, .9), (MID, END, .1),
             (B, A, .5), (B, B, .2), (B, END, .3), (I, I, .3), (I, A, .4), (I, B, .3)]
    ins = {l: sorted((k, p) for k, d, p in edges if d == l) for l in range(6)}
    in_ptr, in_src, in_logp = [0], [], []
    for l in range(6):
        for k, p in ins[l]:
            in_src.append(k); in_logp.append(math.log(p))
        in_ptr.append(len(in_src))
    sig = (2.0, 3.0)
    return SimpleNamespace(n_states=6, silent_start=3, start=START, end=END, in_ptr=np.array(in_ptr), in_src=np.array(in_src),
                           in_logp=np.array(in_logp), emis_kind=np.array([1, 1, 2]), emis_a=np.array([80.0, 100.0, 60.0]),
                           emis_b=np.array([1 / (2 * sig[0] ** 2), 1 / (2 * sig[1] ** 2), 120.0]),
                           emis_c=np.array([-math.log(sig[0] * math.sqrt(2 * math.pi)), -math.log(sig[1] * math.sqrt(2 * math.pi)), -math.log(60.0)]),
                           count_inc=np.array([0, 1, 0, 0, 0, 0]), names=["A", "B", "I", "start", "mid", "end"])


@pytest.mark.parametrize("x", [[], [81.0], [79.0, 101.5], [82.0, 99.0, 78.5], [80.5, 97.0, 110.0, 84.0], [81.0, 103.0, 79.0, 100.0, 99.0],
                               [81.0, float("nan"), 79.0, 100.0], [float("nan")] * 3, [81.0, 150.0, 99.0], [150.0, 81.0], [81.0, 20.0, 99.0, 80.0, 130.0]],
                         ids=lambda x: "T%d" % len(x))
def test_reference_equals_path_enumeration(x):
    """Every start -> end path of the toy net that emits T <= 5 observations, among them a missing one and ones no Uniform can emit
    (150 and 130 lie above the insert's support, 20 below it): w, wx, wxx and log_lik to 1e-12 relative, both dtypes."""
    toy = _toy()
    want = brute_force(toy, x)
    for dtype in (np.longdouble, np.float64):
        got = posterior_ref(toy, x, dtype)
        assert got[1] == want[1]
        if want[1]:
            assert got[0] == -np.inf and not got[2].any() and not got[3].any() and not got[4].any()
            continue
        assert abs(float(got[0]) - want[0]) <= 1e-12 * max(1.0, abs(want[0]))
        for g, w in zip(got[2:], want[2:]):
            assert np.all(np.abs(np.asarray(g, np.float64) - w) <= 1e-12 * np.maximum(1.0, np.abs(w))), (dtype, g, w)
    assert want[1] == (0 if len(x) else 1)          # start does not reach end without an emission


def test_product_rule_equals_the_reference_on_the_toy_net():
    from strique_amd import state_posteriors as sp
    toy = _toy()
    for x in ([81.0, 103.0, 79.0, 100.0, 99.0], [81.0, float("nan"), 150.0, 100.0], []):
        got, want = sp.state_posteriors(toy, x), posterior_ref(toy, x, np.longdouble)
        assert got[1] == want[1]
        if want[1] == 0:
            assert abs(got[0] - float(want[0])) <= 1e-12 * abs(float(want[0]))
            for g, w in zip(got[2:], want[2:]):
                assert np.all(np.abs(g - np.asarray(w, np.float64)) <= 1e-12 * np.maximum(1.0, np.abs(np.asarray(w, np.float64))))


# ---- the identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", [("c9orf72", "+"), ("c9orf72", "-"), ("fmr1", "+"), ("gcg", "+")])
def test_identities_on_the_flanked_models(pm, opm, cfg, targets, orc, name, strand):
    """sum_s w = the observations that are numbers; on a window without NaN the counted states hold E[v | x], forward_ref's mean.
    The product's rule on the baked model (matched by state name) gives the reference's rows."""
    from oracle import hmm_oracle as ho
    from strique_amd import hmm, state_posteriors as sp
    hcfg = {"leave_repeat": LEAVE} if name == "gcg" else dict(cfg["HMM"], leave_repeat=LEAVE)
    repeat, prefix, suffix = targets["fmr1" if name == "gcg" else name]
    r, p, s = ("GCG" if name == "gcg" else repeat).upper(), prefix[-20:].upper(), suffix[:20].upper()
    if strand == "-":
        r, p, s = orc.revcomp(r), orc.revcomp(s), orc.revcomp(p)
    prep = ho.prepare(ho.flanked_net(r, p, s, opm, hcfg)[0])
    rng = np.random.default_rng(31)
    x, _ = sample_window(prep, rng)
    while not 140 <= len(x) <= 400:
        x, _ = sample_window(prep, rng)
    ll, status, w, wx, wxx = posterior_ref(prep, x, np.longdouble)
    fll, fmean, _, fstatus = forward_ref(prep, x, np.longdouble)
    assert status == fstatus == 0 and abs(ll - fll) <= 1e-15 * abs(fll)
    assert abs(w.sum() - len(x)) <= 1e-12 * len(x)
    assert abs(counted_occupancy(prep, w) - fmean) <= 1e-9 * max(1.0, float(fmean))
    holes = x.copy(); holes[[0, len(x) // 2, len(x) - 1]] = np.nan
    w2 = posterior_ref(prep, holes, np.longdouble)[2]
    assert abs(w2.sum() - (len(x) - 3)) <= 1e-12 * len(x)
    baked = hmm.FlankedRepeatModel(r, p, s, pm, hcfg).baked
    on, bn = emitting_names(prep), emitting_names(baked)
    assert sorted(on) == sorted(bn)
    idx = [on.index(nm) for nm in bn]
    got = sp.state_posteriors(baked, x)
    F = posterior_ref(prep, x, np.float64)
    assert got[1] == 0 and abs(got[0] - float(ll)) <= 1e-12 * abs(float(ll))
    for g, f, r_ in zip(got[2:], F[2:], (w, wx, wxx)):
        E = float(np.max(np.abs(f - r_) / np.maximum(1, np.abs(r_))))
        assert float(np.max(np.abs(g - r_[idx]) / np.maximum(1, np.abs(r_[idx])))) <= 16 * max(E, 1e-15)


# ---- the host side of calibrate ----------------------------------------------------------------------------------------------------
WHAT = [("prefix", "match", "AAAAAC"), ("prefix", "insert", None), ("repeat", "match", "GGCCCC"), ("repeat", "match", "GCCCCG"),
        ("repeat", "dummy", None), ("suffix", "match", "GGCCCC"), ("suffix", "match", "TTTTTT")]


def _records(seed, n_reads=7):
    rng = np.random.default_rng(seed)
    recs = []
    for r in range(n_reads):
        w = rng.uniform(0, 50, len(WHAT)) * (rng.random(len(WHAT)) < 0.8)
        w[6] = 0.0                                         # a k-mer nobody ever sees
        wx = w * rng.normal(90, 30, len(WHAT)) * (1 + 1e-9 * rng.normal(size=len(WHAT)))
        wxx = w * np.abs(rng.normal(8500, 1000, len(WHAT)))
        recs.append((WHAT, w, wx, wxx))
    return recs


def test_pool_posterior_does_not_depend_on_order(pm):
    from strique_amd import calibrate
    recs = _records(3)
    base = calibrate.pool_posterior(recs)
    assert list(base) == sorted(base) == ["AAAAAC", "GCCCCG", "GGCCCC"]          # inserts, dummies and unseen k-mers: not pooled
    assert base["GGCCCC"][1] == math.fsum([float(w[2]) for _, w, _, _ in recs] + [float(w[5]) for _, w, _, _ in recs])
    assert base["AAAAAC"][2] == math.fsum(float(s[0]) for _, _, s, _ in recs)
    text = calibrate.format(calibrate.estimate(base, pm, 1)[1], posterior=True)
    order = list(range(len(recs)))
    for seed in range(5):
        random.Random(seed).shuffle(order)
        again = calibrate.pool_posterior([recs[i] for i in order])
        assert again == base and calibrate.format(calibrate.estimate(again, pm, 1)[1], posterior=True) == text
    with pytest.raises(ValueError):
        calibrate.pool_posterior([(WHAT, np.zeros(3), np.zeros(3), np.zeros(3))])


def test_n_reads_counts_reads_with_one_expected_observation():
    from strique_amd import calibrate
    def rec(a, b):          # GGCCCC sits in two states: together they decide
        w = np.zeros(len(WHAT)); w[2], w[5] = a, b
        return (WHAT, w, w * 97.0, w * 97.0 * 97.0)
    pooled = calibrate.pool_posterior([rec(0.5, 0.49), rec(0.5, 0.5), rec(1.0, 0.0), rec(0.0, 0.99), rec(3.0, 4.0)])
    assert list(pooled) == ["GGCCCC"]
    n_reads, W, S, Q = pooled["GGCCCC"]
    assert n_reads == 3 and W == math.fsum([0.5, 0.49, 0.5, 0.5, 1.0, 0.99, 3.0, 4.0])
    assert calibrate.pool_posterior([rec(0.0, 0.0)]) == {}


def test_estimate_on_expected_observations(pm):
    from strique_amd import calibrate
    t_mean = pm.model_dict["GGCCCC"][0]
    for W, updated in ((199.99999999999997, 0), (200.0, 1), (200.5, 1)):
        pooled = {"GGCCCC": (5, W, W * 95.25, W * (95.25 ** 2 + 4.0))}
        means, rows = calibrate.estimate(pooled, pm, 200)
        kmer, n_reads, N, mean, sd, tm, ts, delta, upd = rows[0]
        assert (upd, "GGCCCC" in means) == (updated, bool(updated)) and N == W and n_reads == 5
        assert mean == (W * 95.25) / W and abs(sd - 2.0) < 1e-6 and tm == t_mean and delta == mean - t_mean


def test_stats_files_round_trip_with_both_headers(pm):
    from strique_amd import calibrate
    rows = calibrate.estimate(calibrate.pool_posterior(_records(9)), pm, 1)[1]
    text = calibrate.format(rows, posterior=True)
    assert text.splitlines()[0].split("\t") == calibrate.STATS_HEADER_POSTERIOR == ["kmer", "n_reads", "exp_obs", "mean", "sd", "table_mean", "table_stdv", "delta", "updated"]
    back = calibrate.parse(text)
    assert back == rows and all(isinstance(r[2], float) for r in back) and calibrate.format(back, posterior=True) == text
    hard = [(r[0], r[1], int(r[2]) + 1) + r[3:] for r in rows]
    htext = calibrate.format(hard)
    assert htext.splitlines()[0].split("\t") == calibrate.STATS_HEADER and calibrate.format(hard, posterior=False) == htext
    assert calibrate.parse(htext) == hard and all(isinstance(r[2], int) for r in calibrate.parse(htext))
    with pytest.raises(ValueError):
        calibrate.parse(text.replace("exp_obs", "observations"))


# ---- the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message,env", [
    (["--posterior", "--min-obs", "200"], "calibrate needs --min-score S", {}),
    (["--posterior", "--min-score", "5"], "calibrate needs --min-obs N", {}),
    (["--posterior", "--min-score", "5", "--min-obs", "200", "--mod_model", "m.model"], "calibrate cannot be combined with --mod_model", {}),
    (["--posterior", "--min-score", "5", "--min-obs", "200", "--scan"], "calibrate cannot be combined with --scan", {}),
    (["--posterior", "--min-score", "5", "--min-obs", "200"], "calibrate runs in a single process", {"WORLD_SIZE": "2", "RANK": "0"}),
])
def test_calibrate_posterior_refusals(capsys, tmp_path, monkeypatch, extra, message, env):
    from strique_amd import cli
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        cli.main(["calibrate", str(tmp_path / "reads.fofn"), str(tmp_path / "m.model"), str(tmp_path / "repeat.tsv"), "--out", str(tmp_path / "o.model")] + extra)
    assert e.value.code == 2
    assert ": error: " + message in capsys.readouterr().err
    assert not (tmp_path / "o.model").exists()


def test_calibrate_reads_routes_the_keyword():
    """Without the flag the counter is called exactly as before -- no keyword at all; with it, posterior=True, and the records carry
    the three rows (the log-likelihood stays behind)."""
    from strique_amd import cli
    calls = []
    model = SimpleNamespace(state_kmers=lambda: WHAT)

    class OldCounter(object):
        targets = {"t": (SimpleNamespace(repeatHMM=model), SimpleNamespace(repeatHMM=model))}

        def state_stats_batch(self, items):          # the signature of the parent: a keyword would be a TypeError
            calls.append("hard")
            return [((7, 5.0, 5.0, -1.0, 0, 0, "-"), (np.ones(7, np.int64), np.ones(7), np.ones(7))), ((7, 1.0, 5.0, -1.0, 0, 0, "-"), None)]

    class NewCounter(OldCounter):
        def state_stats_batch(self, items, posterior=False):
            calls.append(posterior)
            return [((7, 5.0, 5.0, -1.0, 0, 0, "-"), (np.full(7, .5), np.ones(7), np.ones(7), -123.0)), ((7, 5.0, 2.0, -1.0, 0, 0, "-"), (np.ones(7),) * 3 + (-1.0,))]

    items = [("t", np.zeros(4), "+"), ("t", np.zeros(4), "-")]
    hard = cli.calibrate_reads(items, OldCounter(), 3.0)
    soft = cli.calibrate_reads(items, NewCounter(), 3.0, posterior=True)
    assert calls == ["hard", True]
    assert len(hard) == 1 and len(hard[0]) == 4 and hard[0][1].dtype == np.int64
    assert len(soft) == 1 and len(soft[0]) == 4 and soft[0][0] is WHAT and soft[0][1][0] == .5          # the second read: a flank score below min_score


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported():
    from strique_amd import ffi
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    lib = ffi.load_library()
    for name in ("strq_forward_state_stats", "strq_set_state_posteriors", "strq_batch_fetch_state_posteriors", "strq_last_state_posteriors"):
        assert re.search(r"\bint %s\s*\(strq_ctx\* ctx" % name, header), name
        assert getattr(lib, name) is not None
    lib.strq_abi_version.restype = ctypes.c_int
    assert lib.strq_abi_version() == 13
    for method in ("forward_state_stats", "set_state_posteriors", "batch_fetch_state_posteriors", "last_state_posteriors"):
        assert callable(getattr(ffi.Context, method))
