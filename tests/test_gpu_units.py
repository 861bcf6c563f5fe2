"""Repeat-unit positions on the GPU (strq_set_units, repeatCounter.detect_batch(..., units=True), `count --units`) against the
oracle's Viterbi path: [prefix_begin + t for t, s in enumerate(path) if count_inc[s]] (STRique.py:374-378,433-441)."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import oracle_map, oracle_tc

pytestmark = pytest.mark.gpu

_RNG = np.random.default_rng(4242)
_NT = lambda n: "".join(_RNG.choice(list("ACGT"), n))
# repeat units of 2, 5 and 12 nt next to the bundled 6 (c9orf72) and 3 (FMR1, HTT); a 70 nt unit has no lane layout
# (names of their own: conftest.oracle_tc caches the oracle classifiers by target name for the whole session)
# (general kernel: the back-pointer route)
CUSTOM = {"units_di": ("CA", _NT(150), _NT(150)), "units_penta": ("ATTCT", _NT(150), _NT(150)), "units_dodeca": ("CCCCGCCCCGCG", _NT(150), _NT(150)),
          "units_vntr70": (_NT(70), _NT(150), _NT(150))}


@pytest.fixture(scope="module")
def all_targets(targets):
    out = dict(targets)
    out.update(CUSTOM)
    return out


@pytest.fixture(scope="module")
def counter(pm, cfg, all_targets):
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    for name, (repeat, prefix, suffix) in all_targets.items():
        rc.add_target(name, repeat, prefix, suffix)
    return rc


def oracle_units(orc, opm, cfg, tc, sig):
    """(row, positions or None) of the oracle: its detect() and the path of the same window."""
    row, info = orc.detect(sig, tc, opm, orc.align_params(cfg["align"]))
    pb, se = info["prefix_begin"], info["suffix_end"]
    if not (pb < se and row[1] > 0.0 and row[2] > 0.0):
        return row, None
    fltn = orc.condition(np.asarray(sig), opm)[3]
    _, path, _ = orc.viterbi(tc["hmm"], fltn[pb:se])
    if path is None:
        return row, None
    return row, np.array([pb + t for t, s in enumerate(path) if tc["hmm"].count_inc[s]], np.int64)


def _items(pm, all_targets, names, seed, total=(3500, 6000), nrep=(4, 60), as_int16=None):
    from strique_amd import synth
    table = synth.KmerTable(pm)
    rng = np.random.default_rng(seed)
    items = []
    for k, name in enumerate(names):
        for strand in "+-":
            unit = all_targets[name][0]
            nt = int(rng.integers(*total))
            n = min(int(rng.integers(*nrep)), max(3, (nt - 2400) // len(unit)))
            i16 = (k % 2 == 0) if as_int16 is None else as_int16
            items.append((name, synth.make_read(table, 9, seed * 100 + 2 * k + (strand == "-"), nt, all_targets[name], n, strand=strand, as_int16=i16)[0], strand))
    return items


def _check_against_oracle(got, items, orc, opm, cfg, all_targets):
    tcs = {(n, s): oracle_tc(orc, opm, all_targets, n, s, cfg["HMM"]) for n, _, s in items}
    want = oracle_map(lambda it: oracle_units(orc, opm, cfg, tcs[(it[0], it[2])], it[1]), items)
    for (name, sig, strand), (row, pos), (wrow, wpos) in zip(items, got, want):
        assert tuple(row[:6]) == tuple(wrow[:6]), (name, strand, row, wrow)
        assert (pos is None) == (wpos is None), (name, strand, row)
        if pos is not None:
            assert pos.dtype == np.int64 and np.array_equal(pos, wpos), (name, strand, len(pos), len(wpos))
            assert len(pos) == row[0] - tcs[(name, strand)]["count_bias"]


def test_positions_equal_the_oracle_path(counter, pm, cfg, orc, opm, all_targets):
    items = _items(pm, all_targets, ["c9orf72", "fmr1", "htt", "units_di", "units_penta", "units_dodeca", "units_vntr70"], 1)
    items += _items(pm, all_targets, ["c9orf72", "fmr1"], 2, as_int16=False)
    got = counter.detect_batch(items, units=True)
    assert sum(p is not None and len(p) > 0 for _, p in got) >= len(items) - 2
    _check_against_oracle(got, items, orc, opm, cfg, all_targets)


def test_rows_do_not_change_with_units_on(counter, pm, pm_mod, cfg, targets, all_targets):
    """Rows and modification strings are byte-identical with and without positions -- the modification pass included
    (its flanked-model decode runs in MARK mode: test_gpu_detect.py::test_modification_pass's workload)."""
    from strique_amd.counter import repeatCounter
    items = _items(pm, all_targets, ["c9orf72", "fmr1", "htt", "units_dodeca"], 3)
    assert [r for r, _ in counter.detect_batch(items, units=True)] == counter.detect_batch(items)
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    rc.add_target("c9orf72", repeat, prefix, suffix)
    rng = np.random.default_rng(12)
    backbone = "".join(rng.choice(list("ACTG"), 2000))
    mitems = []
    for i, model in ((40, pm), (40, pm_mod), (110, pm_mod), (7, pm)):
        seq = backbone[:1000] + prefix + repeat * i + suffix + backbone[-1000:]
        sig = model.generate_signal(seq, samples=8, noise=True, rng=rng)
        mitems += [("c9orf72", sig, "+"), ("c9orf72", np.round(sig * (8192 / 1400.0) - 10).astype(np.int16), "+")]
    off = rc.detect_batch(mitems)
    on = rc.detect_batch(mitems, units=True)
    assert [r for r, _ in on] == off and all(set(r[6]) <= set("01") for r in off)
    # the same positions as a target without the modification model (count-mode decode)
    plain = counter.detect_batch(mitems, units=True)
    assert all(p is not None for _, p in on)
    assert _same([(r[:6], p) for r, p in on], [(r[:6], p) for r, p in plain])
    assert counter.detect_batch(items) == [r for r, _ in counter.detect_batch(items, units=True)]


def _same(a, b):
    return len(a) == len(b) and all(ra == rb and ((pa is None and pb is None) or (pa is not None and pb is not None and np.array_equal(pa, pb)))
                                    for (ra, pa), (rb, pb) in zip(a, b))


def test_every_route_gives_the_same_positions(counter, pm, all_targets):
    """Unit records (g2 and lane-layout kernels) against back-pointers + traceback, pipelined against serial, whole sub-batches
    against small ones."""
    items = _items(pm, all_targets, ["c9orf72", "fmr1", "htt", "units_di", "units_penta", "units_dodeca"], 5)
    base = counter.detect_batch(items, units=True)
    assert sum(p is not None for _, p in base) >= len(items) - 2
    for key, value in (("STRQ_UNITS_BACKPOINTERS", "1"), ("STRQ_VIT_NO_G2", "1"), ("STRQ_SERIAL", "1"), ("STRQ_SUBBATCH_READS", "3"),
                       ("STRQ_UNITS_WS_BYTES", "1")):
        counter.ctx.set_option(key, value)
        try:
            got = counter.detect_batch(items, units=True)
        finally:
            counter.ctx.set_option(key, "")
        assert _same(got, base), key
    counter.ctx.set_option("STRQ_VIT_NO_G2", "1"); counter.ctx.set_option("STRQ_UNITS_BACKPOINTERS", "1")
    try:
        assert _same(counter.detect_batch(items, units=True), base)
    finally:
        counter.ctx.set_option("STRQ_VIT_NO_G2", ""); counter.ctx.set_option("STRQ_UNITS_BACKPOINTERS", "")


def test_full_size_reads(counter, pm, cfg, orc, opm, all_targets):
    """50 kb reads: 2000 x GGGGCC (a window of ~100 k samples, 2000 hops), and empirical-noise reads; record route equals the
    back-pointer route, and the long read equals the oracle's path."""
    from strique_amd import synth
    table = synth.KmerTable(pm)
    noise = synth.EmpiricalNoise()
    items = [("c9orf72", synth.make_read(table, 13, 1, 50000, all_targets["c9orf72"], 2000, strand="+")[0], "+")]
    for i in range(3):
        strand = "+-"[i % 2]
        items.append(("c9orf72", synth.make_read(table, 7, 600 + i, 50000, all_targets["c9orf72"], (300, 800, 1200)[i], strand=strand, noise=noise)[0], strand))
    got = counter.detect_batch(items, units=True)
    counter.ctx.set_option("STRQ_UNITS_BACKPOINTERS", "1")
    try:
        ref = counter.detect_batch(items, units=True)
    finally:
        counter.ctx.set_option("STRQ_UNITS_BACKPOINTERS", "")
    assert _same(got, ref)
    row, pos = got[0]
    assert pos is not None and len(pos) > 1900 and np.all(np.diff(pos) > 0)
    _check_against_oracle(got[:1], items[:1], orc, opm, cfg, all_targets)


def test_bad_reads_are_not_decoded(counter, pm, all_targets):
    good = _items(pm, all_targets, ["c9orf72"], 7, as_int16=True)
    rng = np.random.default_rng(3)
    bad = [("c9orf72", np.full(5000, 300, np.int16), "+"),                           # constant: not normalised
           ("c9orf72", rng.integers(200, 800, 6000).astype(np.int16), "-"),         # no flank: the gate fails
           ("c9orf72", np.array([300, 310, 305], np.int16), "+"),                   # tiny
           ("fmr1", np.zeros(0, np.int16), "+")]                                    # empty
    items = bad[:2] + good + bad[2:]
    got = counter.detect_batch(items, units=True)
    assert [p is None for _, p in got] == [True, got[1][1] is None, False, False, True, True]
    assert got[0][0][0] == 0 and (got[1][1] is not None or got[1][0][0] == 0)
    assert counter.detect_batch(items) == [r for r, _ in got]


def test_count_units_on_the_bundled_read(workdir):
    """`count --units` on tests/golden/c9orf72.{fast5,sam}: the count TSV is byte-identical to a run without the flag, the side
    file has one row per count row with the positions detect_batch(..., units=True) gives; two ranks write the same side file."""
    import subprocess
    import sys
    from conftest import ROOT
    from strique_amd import cli
    from test_cli_end_to_end import _index
    fofn = workdir / "data" / "reads.fofn"
    fofn.write_text(_index(workdir))
    base = [str(fofn), str(workdir / "r9_4_450bps.model"), str(workdir / "repeat_config.tsv"),
            "--config", str(workdir / "STRique.json"), "--algn", str(workdir / "data" / "c9orf72.sam")]
    plain, with_units, units = workdir / "plain.tsv", workdir / "with.tsv", workdir / "units.tsv"
    cli.main(["count"] + base + ["--out", str(plain)])
    cli.main(["count"] + base + ["--out", str(with_units), "--units", str(units)])
    assert with_units.read_bytes() == plain.read_bytes()
    rows = plain.read_text().splitlines()[1:]
    urows = cli.parse_units(open(units))
    assert len(urows) == len(rows) == 1
    rid, target, strand, count = rows[0].split("\t")[:4]
    assert urows[0][:4] == (rid, target, strand, int(count))
    # the same read through the Python entry
    from strique_amd.counter import repeatCounter
    config = cli.parse_config(str(workdir / "repeat_config.tsv"), str(workdir / "STRique.json"))
    rc = repeatCounter(str(workdir / "r9_4_450bps.model"), align_config=config["align"], HMM_config=config["HMM"], device=0)
    chrom, b, e, repeat, prefix, suffix = config["repeat"][target]
    rc.add_target(target, repeat, prefix, suffix)
    raw = cli.Fast5Index(str(fofn)).get_raw(rid)
    row, pos = rc.detect(target, raw, strand, units=True)
    assert row[0] == int(count) and list(pos) == urows[0][4] and len(pos) > 700
    two, units2 = workdir / "two.tsv", workdir / "units2.tsv"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "STRique.py"), "count"] + base + ["--out", str(two), "--units", str(units2),
                                                                                          "--backend", "gloo", "--share-device"]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert two.read_bytes() == plain.read_bytes() and units2.read_bytes() == units.read_bytes()


from test_cli_end_to_end import workdir  # noqa: E402,F401  (the bundled fast5 / SAM / model files in a temporary directory)
