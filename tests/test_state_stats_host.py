"""State statistics and calibration without a GPU: the header against the library's exports, argument errors, what every emitting
state of the flanked model stands for, the pooling and estimation rule, the files, the refusals of `calibrate`, and the CPU check --
one round of re-estimation on reads made from a shifted table, with the reference statistics of tests/state_stats_ref.py."""
import ctypes
import io
import math
import os
import random
import re

import numpy as np
import pytest

import state_stats_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("strq_viterbi_state_stats", "strq_set_state_stats", "strq_batch_fetch_state_stats", "strq_last_state_stats")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_exports_agree_on_the_new_symbols():
    from strique_amd import build, ffi
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    declared = set(re.findall(r"\b(strq_[a-z_0-9]+)\s*\(", header))
    handle = ctypes.CDLL(build.LIB)
    for name in NEW_SYMBOLS:
        assert name in declared and getattr(handle, name) is not None
    for method in ("set_state_stats", "batch_fetch_state_stats", "last_state_stats", "viterbi_state_stats"):
        assert callable(getattr(ffi.Context, method))
    handle.strq_abi_version.restype = ctypes.c_int
    assert handle.strq_abi_version() == 13          # the entries are additive


def test_null_context_is_an_argument_error():
    from strique_amd import build, ffi
    lib = ctypes.CDLL(build.LIB)
    out = (ctypes.c_double * 4)()
    off = (ctypes.c_int64 * 2)()
    assert lib.strq_set_state_stats(None, ctypes.c_int32(1)) == ffi.STRQ_ERR_ARG
    assert lib.strq_last_state_stats(None, out) == ffi.STRQ_ERR_ARG
    assert lib.strq_batch_fetch_state_stats(None, off, None, None, None, ctypes.c_int64(0), None) == ffi.STRQ_ERR_ARG
    assert lib.strq_viterbi_state_stats(None, ctypes.c_int32(0), ctypes.c_int64(0), None, None, None, None, None, None, None, None) == ffi.STRQ_ERR_ARG


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def test_rule_order_nan_and_unvisited_states():
    from strique_amd import state_stats
    x = np.array([1e16, 1.0, np.nan, -1e16, 3.0, 0.1, 0.2, 0.3, -0.0])
    path = np.array([0, 0, 0, 0, 2, 2, 2, 2, 3])
    n, s, q = state_stats.state_stats(x, path, 5)
    assert n.dtype == np.int64 and s.dtype == q.dtype == np.float64
    assert n.tolist() == [3, 0, 4, 1, 0] and int(n.sum()) == len(x) - 1
    assert s[0] == (1e16 + 1.0) + -1e16 and s[0] != 1.0          # ascending t: the 1.0 is lost to rounding, as the rule says
    assert s[2] == ((3.0 + 0.1) + 0.2) + 0.3 and q[2] == ((9.0 + 0.1 * 0.1) + 0.2 * 0.2) + 0.3 * 0.3
    for a in (s, q):
        assert ssr.bits(a)[[1, 3, 4]].tolist() == [0, 0, 0]          # +0.0 bits: never visited, and +0.0 + -0.0
    assert ssr.same_rows((n, s, q), ssr.rule(x, path, 5))
    with pytest.raises(ValueError):
        state_stats.state_stats(x, np.full(len(x), 5), 5)
    with pytest.raises(ValueError):
        state_stats.state_stats(x, path[:-1], 5)


# ---- what a state stands for -------------------------------------------------------------------------------------------------------
def _models(pm, cfg):
    from strique_amd import hmm
    out = []
    for name in ("c9orf72", "fmr1"):
        repeat, prefix, suffix = cfg["repeat"][name][3:6]
        R, P, S = repeat.upper(), prefix[-50:].upper(), suffix[:50].upper()
        out.append((name, "+", R, P, S)); out.append((name, "-", ssr.revcomp(R), ssr.revcomp(S), ssr.revcomp(P)))
    P, S = cfg["repeat"]["c9orf72"][4][-50:].upper(), cfg["repeat"]["c9orf72"][5][:50].upper()
    out.append(("gcg", "+", "GCG", P, S))
    return [(name, strand, R, P, S, hmm.FlankedRepeatModel(R, P, S, pm, cfg["HMM"])) for name, strand, R, P, S in out]


def test_state_kmers_against_the_state_names(pm, cfg):
    from strique_amd import hmm
    k = pm.kmer
    for name, strand, R, P, S, m in _models(pm, cfg):
        what = m.state_kmers()
        names = m.baked.names[:m.baked.silent_start]
        assert len(what) == len(names) == m.baked.silent_start
        units = -(-k // len(R))
        seqs = {"prefix": P + (R * units)[:-1], "repeat": hmm.extend_repeat(R, k)[0], "suffix": R * units + S}
        n_match = 0
        for state, (section, kind, kmer) in zip(names, what):
            assert state.startswith(section), (name, strand, state)
            tail = state[len(section):]
            if tail.startswith("dummy"):
                assert (kind, kmer) == ("dummy", None) and section == "repeat"
            elif tail.endswith("i"):
                assert (kind, kmer) == ("insert", None)
            else:
                assert tail.endswith("m") and kind == "match"
                c = int(tail[:-1])
                assert kmer == seqs[section][c:c + k] and len(kmer) == k, (name, strand, state)
                # the emission of the state is that k-mer's level
                assert m.baked.emis_a[names.index(state)] == pm.model_dict[kmer][0]
                n_match += 1
        assert n_match == sum(len(s) - k + 1 for s in seqs.values())
        assert sum(kind == "dummy" for _, kind, _ in what) == 2


# ---- pool, estimate, the files -----------------------------------------------------------------------------------------------------
def _records(seed, n_reads=7):
    rng = np.random.default_rng(seed)
    what = [("prefix", "match", "AAAAAC"), ("prefix", "insert", None), ("repeat", "match", "GGCCCC"), ("repeat", "match", "GCCCCG"),
            ("repeat", "dummy", None), ("suffix", "match", "GGCCCC"), ("suffix", "match", "TTTTTT")]
    recs = []
    for r in range(n_reads):
        n = rng.integers(0, 50, len(what)).astype(np.int64)
        n[6] = 0                                           # a k-mer nobody ever sees
        s = rng.normal(90, 30, len(what)) * n * (1 + 1e-9 * rng.normal(size=len(what)))
        q = np.abs(rng.normal(8500, 1000, len(what))) * n
        s[n == 0] = 0.0; q[n == 0] = 0.0
        recs.append((what, n, s, q))
    return recs


def test_pool_does_not_depend_on_order_or_batching(pm):
    from strique_amd import calibrate
    recs = _records(3)
    base = calibrate.pool(recs)
    assert list(base) == sorted(base) == ["AAAAAC", "GCCCCG", "GGCCCC"]          # inserts, dummies and unseen k-mers: not pooled
    assert base["GGCCCC"][1] == sum(int(n[2]) + int(n[5]) for _, n, _, _ in recs)
    text = calibrate.format(calibrate.estimate(base, pm, 1)[1])
    order = list(range(len(recs)))
    for seed in range(5):
        random.Random(seed).shuffle(order)
        again = calibrate.pool([recs[i] for i in order])
        assert again == base and calibrate.format(calibrate.estimate(again, pm, 1)[1]).encode() == text.encode()
    # re-batched: pooling the records of two halves one after the other is pooling them all
    assert calibrate.pool(recs[4:] + recs[:4]) == base
    # S is the exactly rounded sum of the per-(read, state) sums
    assert base["AAAAAC"][2] == math.fsum(float(s[0]) for _, n, s, _ in recs if n[0]) and base["AAAAAC"][0] == sum(1 for _, n, _, _ in recs if n[0])


def test_estimate_honours_min_obs(pm):
    from strique_amd import calibrate
    pooled = calibrate.pool(_records(5))
    big = min(v[1] for v in pooled.values()) + 1
    means, rows = calibrate.estimate(pooled, pm, big)
    assert [r[0] for r in rows] == list(pooled)
    for kmer, n_reads, N, mean, sd, t_mean, t_stdv, delta, updated in rows:
        assert updated == (1 if N >= big else 0) == (1 if kmer in means else 0)
        assert mean == pooled[kmer][2] / N and delta == mean - t_mean and (t_mean, t_stdv) == pm.model_dict[kmer]
        assert sd == max(0.0, pooled[kmer][3] / N - mean * mean) ** 0.5
    assert 0 < len(means) < len(rows)
    assert calibrate.estimate(pooled, pm, 10 ** 9)[0] == {}
    with pytest.raises(ValueError):
        calibrate.estimate(pooled, pm, 0)


def test_model_and_stats_files_round_trip(pm, tmp_path):
    from strique_amd import calibrate
    from strique_amd.pore_model import pore_model
    pooled = calibrate.pool(_records(9))
    means, rows = calibrate.estimate(pooled, pm, 1)
    path = tmp_path / "new.model"
    calibrate.write_model(str(path), pm, means)
    back = pore_model(str(path))
    assert list(back.model_dict) == list(pm.model_dict)          # every k-mer, input order
    for kmer, (mean, stdv) in pm.model_dict.items():
        assert back.model_dict[kmer] == (means.get(kmer, mean), stdv)          # exact: repr floats
    assert sum(back.model_dict[k] != pm.model_dict[k] for k in pm.model_dict) == len(means) == 3
    text = calibrate.format(rows)
    assert text.splitlines()[0].split("\t") == calibrate.STATS_HEADER == ["kmer", "n_reads", "n_obs", "mean", "sd", "table_mean", "table_stdv", "delta", "updated"]
    assert calibrate.parse(text) == rows and calibrate.format(calibrate.parse(text)) == text
    for bad in ("x\ty\n", text + "GGCCCC\t1\n"):
        with pytest.raises(ValueError):
            calibrate.parse(bad)


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message,env", [
    (["--min-obs", "200"], "calibrate needs --min-score S", {}),
    (["--min-score", "5"], "calibrate needs --min-obs N", {}),
    (["--min-score", "5", "--min-obs", "200", "--mod_model", "m.model"], "calibrate cannot be combined with --mod_model", {}),
    (["--min-score", "5", "--min-obs", "200", "--scan"], "calibrate cannot be combined with --scan", {}),
    (["--min-score", "5", "--min-obs", "200"], "calibrate runs in a single process", {"WORLD_SIZE": "2", "RANK": "0"}),
])
def test_calibrate_refusals(capsys, tmp_path, monkeypatch, extra, message, env):
    from strique_amd import cli
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit) as e:
        cli.main(["calibrate", str(tmp_path / "reads.fofn"), str(tmp_path / "m.model"), str(tmp_path / "repeat.tsv"), "--out", str(tmp_path / "o.model")] + extra)
    assert e.value.code == 2
    assert ": error: " + message in capsys.readouterr().err
    assert not (tmp_path / "o.model").exists()


# ---- the CPU check -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c9orf72", "fmr1"])
def test_one_round_halves_a_planted_level_error(orc, tables, cfg, name):
    """Six clean 8 kb reads made from a table whose repeat k-mers (both strands) are shifted by U[-3, 3] pA, decoded with the shipped
    table: one round of pool / estimate (min_obs 200) on the reference statistics at least halves the table's mean absolute error over
    the planted k-mers, and the six counts are exact under the new table.  Measured: c9orf72 1.605 -> 0.493 pA (max 2.968 -> 1.502;
    GGCCCC and GCCCCG, table levels 96.96 and 98.14, keep 1.5 and 1.1 pA: hard assignment between two neighbours at almost one
    level), fmr1 1.646 -> 0.343 pA."""
    from strique_amd import calibrate
    from strique_amd.pore_model import pore_model
    target = tuple(cfg["repeat"][name][3:6])
    planted, shift = ssr.planted_table(tables, target[0])
    truth = pore_model(table=planted).model_dict
    reads = ssr.planted_reads(planted, target)
    shipped = (planted[0], np.array(tables["base_mean"], np.float64), planted[2])
    pm0 = pore_model(table=shipped)
    rows0, records, _ = ssr.reference_records(orc, cfg, shipped, target, reads)
    assert len(records) == 6
    means, stats = calibrate.estimate(calibrate.pool(records), pm0, 200)
    err = lambda table: np.array([abs(table[k] - truth[k][0]) for k in shift])
    before = err({k: v[0] for k, v in pm0.model_dict.items()})
    after = err({k: means.get(k, v[0]) for k, v in pm0.model_dict.items()})
    print("%s: mean abs error %.3f -> %.3f pA, max %.3f -> %.3f; count - planted before %s" %
          (name, before.mean(), after.mean(), before.max(), after.max(), [r[0] - u for r, (_, _, u) in zip(rows0, reads)]))
    assert abs(before.mean() - np.mean([abs(v) for v in shift.values()])) < 1e-9
    assert after.mean() <= 0.5 * before.mean()
    new_table = (planted[0], np.array([means.get(k, m) for k, m in zip(planted[0], shipped[1])]), planted[2])
    rows1, _, _ = ssr.reference_records(orc, cfg, new_table, target, reads)
    assert [r[0] for r in rows1] == [u for _, _, u in reads]
