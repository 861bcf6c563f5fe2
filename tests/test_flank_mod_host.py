"""Flank methylation calls without a GPU: the rule of strique_amd/flank_mod.py (sites, groups, refusals, bounds, the side file), the
two models of strique_amd/hmm.py against RepeatModModel and against the oracle's un-baked nets, the ABI entry, and the properties
the GPU tests rely on in tests/flank_mod_ref.py (the tie cap, both statuses seen, the sign of the ratios)."""
import io
import os

import numpy as np
import pytest

import flank_mod_ref as fr
import mod_llr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6


def _flank(L, at, fill="AT"):
    """A flank of L bases without CG except at the positions `at`."""
    s = list((fill * L)[:L])
    for c in at:
        s[c:c + 2] = "CG"
    s = "".join(s)
    assert [i for i in range(L - 1) if s[i:i + 2] == "CG"] == sorted(at), s
    return s


def test_sites_and_groups():
    from strique_amd import flank_mod as fm
    # a pair at distance exactly k - 2 merges, at k - 1 it does not
    g = fm.groups(_flank(40, [10, 10 + K - 2]), K)
    assert [(x.sites, x.c0, x.c1) for x in g] == [((10, 14), 10 - K + 2, 14)] and g[0].n_columns == 2 * K - 3 and g[0].n_sites == 2
    g = fm.groups(_flank(40, [10, 10 + K - 1]), K)
    assert [(x.sites, x.c0, x.c1) for x in g] == [((10,), 6, 10), ((15,), 11, 15)]
    # a site at c = 0 and one at c = L - 2 keep at least one column; the columns are clipped to [0, n)
    L = 30
    g = fm.groups(_flank(L, [0, L - 2]), K)
    assert [(x.sites, x.c0, x.c1, x.n_columns) for x in g] == [((0,), 0, 0, 1), ((L - 2,), L - K, L - K, 1)]
    g = fm.groups(_flank(L, [2]), K)
    assert (g[0].c0, g[0].c1) == (0, 2)
    # a flank without CG; lower case is read as upper case
    assert fm.groups("ATGCATGCAATTGGCC", K) == [] and fm.sites("ATGC") == []
    assert fm.sites("aacgtt") == [2]
    with pytest.raises(ValueError, match="has no 6-mer"):
        fm.groups("ACGTA", K)
    # a single site spells k - 1 columns, i.e. 2 k - 2 bases
    flank = _flank(40, [20])
    assert fm.site_sequence(flank, fm.groups(flank, K)[0], K) == flank[16:26]


def test_minus_strand_mapping():
    from strique_amd import flank_mod as fm
    plus = "TTACGTTTTTTTTCGACGAAAAAAAAAAAA"          # configured suffix, not a palindrome: CG at 3, 13, 16
    L = len(plus)
    minus_prefix = fr.orc.revcomp(plus)                  # what the - strand's classifier reads as its prefix
    assert fm.sites(plus) == [3, 13, 16] and fm.sites(minus_prefix) == sorted(L - 2 - c for c in (3, 13, 16))
    gp = fm.groups(plus, K); gm = fm.groups(minus_prefix, K)
    assert [fm.configured(fm.SUFFIX, g, L, '+') for g in gp] == [(fm.SUFFIX, 3), (fm.SUFFIX, 13)]
    # the - strand sees the same groups in reverse order, names the configured flank and the group's first C on the + strand
    assert [fm.configured(fm.PREFIX, g, L, '-') for g in gm] == [(fm.SUFFIX, 13), (fm.SUFFIX, 3)]
    assert [g.n_sites for g in gm] == [2, 1]
    with pytest.raises(ValueError):
        fm.configured(fm.PREFIX, gm[0], L, '?')


def test_the_htt_rows_of_the_table(targets):
    """sites, groups, longest group of the HTT flanks (tests/golden/repeat_config_htt.tsv), by the rule and by the reference's
    restatement of it."""
    from strique_amd import flank_mod as fm
    _, prefix, suffix = targets["htt"]
    for flank, want in ((prefix, (15, 11, 13)), (suffix, (22, 11, 23))):
        g = fm.check(flank.upper(), K)
        assert (sum(x.n_sites for x in g), len(g), max(x.n_columns for x in g)) == want
        assert [(x.sites, x.c0, x.c1) for x in g] == fr.groups(flank.upper(), K)
    for name in ("c9orf72", "fmr1"):
        for flank in targets[name][1:]:
            assert [(x.sites, x.c0, x.c1) for x in fm.check(flank.upper(), K)] == fr.groups(flank.upper(), K)


def test_refusals():
    from strique_amd import flank_mod as fm
    # 32 columns: sites every k - 2 bases from 10 on, c_last - c_first + k - 1 = 32 (27 = 6 * 4 + 3 does not divide: use distances 4 .. 3)
    at = [10, 14, 18, 22, 26, 30, 34, 37]
    assert at[-1] - at[0] + K - 1 == 32
    with pytest.raises(ValueError, match="spans 32 profile columns, at most 31"):
        fm.check(_flank(80, at), K, "prefix")
    ok = fm.check(_flank(80, at[:-1] + [36]), K)
    assert len(ok) == 1 and ok[0].n_columns == 31
    # 65 groups, K - 1 apart
    at = [K - 1 + (K - 1) * i for i in range(65)]
    with pytest.raises(ValueError, match="holds 65 CpG groups, at most 64"):
        fm.check(_flank(400, at), K, "suffix")
    assert len(fm.check(_flank(400, at[:-1]), K)) == 64
    assert fm.too_long(64 * 150 + 1, 150) and not fm.too_long(64 * 150, 150)


def test_side_file_round_trip():
    from strique_amd import flank_mod as fm
    rows = [("r1", "htt", "+", 17, [(fm.PREFIX, 3, 1, -12.34564), (fm.SUFFIX, 140, 3, float("nan")), (fm.SUFFIX, 7, 2, None), (fm.PREFIX, 9, 1, 0.0)]),
            ("r2", "htt", "-", 0, None), ("r3", "c9orf72", "-", 5, [])]
    text = "\t".join(fm.HEADER) + "\n" + "".join(fm.format_row(*r) + "\n" for r in rows)
    assert text.splitlines()[1] == "r1\thtt\t+\t17\t4\tp:3:1:-12.3456,s:140:3:-,s:7:2:-,p:9:1:0.0000"
    assert text.splitlines()[2] == "r2\thtt\t-\t0\t0\t-"
    back = fm.parse(io.StringIO(text))
    assert back[0] == ("r1", "htt", "+", "17", [(0, 3, 1, -12.3456), (1, 140, 3, None), (1, 7, 2, None), (0, 9, 1, 0.0)])
    assert back[1] == ("r2", "htt", "-", "0", []) and back[2] == ("r3", "c9orf72", "-", "5", [])
    with pytest.raises(ValueError, match="not a --flank-mod file"):
        fm.parse(io.StringIO("ID\ttarget\n"))
    for bad in ("r\tt\t+\t1\t2\tp:3:1:0.5", "r\tt\t+\t1\t1\tq:3:1:0.5", "r\tt\t+\t1\t1\tp:3:0.5"):
        with pytest.raises(ValueError, match="flank-mod row of r"):
            fm.parse(io.StringIO("\t".join(fm.HEADER) + "\n" + bad + "\n"))


def _edges(g):
    return {(g.names[a], g.names[b]): p for a, b, p in g.edges}


def test_site_model_is_the_repeat_mod_model_without_its_loop(pm, pm_mod, cfg):
    from strique_amd import hmm
    repeat = "GGCCCC"
    seq, _ = hmm.extend_repeat(repeat, pm.kmer)
    rm = hmm.RepeatModModel(repeat, pm, pm_mod, cfg["HMM"]); sm = hmm.SiteModModel(seq, pm, pm_mod, cfg["HMM"])
    er, es = _edges(rm.graph), _edges(sm.graph)
    assert set(er) - set(es) == {("e0", "s0")} and set(es) <= set(er)
    assert es[("e0", "end")] == 1.0 and all(es[e] == er[e] for e in es if e != ("e0", "end"))
    assert rm.graph.names == sm.graph.names and rm.graph.kinds == sm.graph.kinds and rm.graph.params == sm.graph.params
    assert rm.graph.layout == sm.graph.layout
    assert rm.baked.names == sm.baked.names and np.array_equal(rm.baked.tag, sm.baked.tag)
    for f in ("emis_kind", "emis_a", "emis_b", "emis_c", "hint_slot", "hint_lane"):
        assert np.array_equal(getattr(rm.baked, f), getattr(sm.baked, f)), f
    # emitting states per group size: the three modes of the passage scorer
    for cols, ne in ((1, 6), (5, 22), (7, 30), (8, 34), (15, 62), (16, 66), (31, 126)):
        assert hmm.SiteModModel("ACGTTGCATGCAACGTTGCATGCAACGTTGCATGCAAC"[:cols + pm.kmer - 1], pm, pm_mod).baked.silent_start == ne


def test_models_against_the_oracles_nets(pm, pm_mod, opm, opm_mod, cfg, targets, orc):
    """The baked models decode what the un-baked nets decode: the same log-probability, and the same columns per observation."""
    from strique_amd import flank_mod, hmm, synth
    flank = targets["htt"][1].upper()[-60:]
    fmodel = hmm.FlankProfileModel(flank, pm, cfg["HMM"])
    onet = fr.profile_model(flank, opm, cfg["HMM"])
    n = len(flank) - K + 1
    assert fmodel.n_columns == n and fmodel.baked.silent_start == 2 * n
    assert fmodel.baked.names[:2 * n] == onet.names[:2 * n] and np.array_equal(fmodel.column_of[:2 * n], onet.column_of[:2 * n])
    assert (fmodel.column_of[2 * n:] == -1).all() and len(fmodel.column_of) == fmodel.baked.n_states
    assert (fmodel.baked.hint_slot[:2 * n] >= 0).all() and fmodel.baked.pos_index is not None
    assert (hmm.FlankProfileModel(targets["htt"][1].upper(), pm, cfg["HMM"]).baked.hint_slot < 0).all()          # 290 states: no lane layout
    rng = np.random.Generator(np.random.PCG64(5))
    x = synth.make_signal(rng, synth.KmerTable(pm), flank.encode(), as_int16=False)
    x = np.clip(x, opm.model_min + .5, opm.model_max - .5)
    lp_b, path_b, _ = orc.viterbi(fmodel.baked, x); lp_o, path_o, _ = orc.viterbi(onet, x)
    assert lp_b == lp_o and np.array_equal(fmodel.column_of[path_b], onet.column_of[path_o])
    g = fr.groups(flank, K)
    ranges = [(a, b) for _, a, b in g]
    assert g and fr.bounds(path_o, onet.column_of, ranges) == flank_mod.bounds(path_b, fmodel.column_of, ranges)
    # the site model, masked either way
    _, c0, c1 = g[0]
    seq = flank[c0:c1 + K]
    sm = hmm.SiteModModel(seq, pm, pm_mod, cfg["HMM"])

    class Arrays(object):
        pass
    a = Arrays(); a.__dict__.update(sm.baked._asdict())
    _, ob, om = fr.site_models(seq, opm, opm_mod, cfg["HMM"])
    xs = np.clip(synth.make_signal(rng, synth.KmerTable(pm_mod), ("AAAAAA" + seq + "TTTTTT").encode(), as_int16=False), sm.model_min, sm.model_max)
    for keep, o in ((0, ob), (1, om)):
        v = orc.viterbi(mod_llr_ref.masked(a, keep), xs, want_path=False)[0]
        assert v == orc.viterbi(o, xs, want_path=False)[0] and np.isfinite(v)


# ---- the bounds, by hand -------------------------------------------------------------------------------------------------------------
COLUMN_OF, HAND = fr.HAND_COLUMN_OF, fr.HAND_PATHS


def test_bounds_by_hand():
    from strique_amd import flank_mod as fm
    for path, ranges, want in HAND:
        assert fm.bounds(path, COLUMN_OF, ranges) == want, (path, ranges)
        assert fr.bounds(path, COLUMN_OF, ranges) == want, (path, ranges)
    assert (fm.SCORED, fm.NO_PATH, fm.EDGE, fm.SKIPPED, fm.TOO_LONG) == (fr.SCORED, fr.NO_PATH, fr.EDGE, fr.SKIPPED, fr.TOO_LONG) == (0, 1, 2, 3, 4)
    assert (fm.MAX_GROUP_COLUMNS, fm.MAX_GROUPS, fm.MAX_STRETCH) == (fr.MAX_COLUMNS, fr.MAX_GROUPS, fr.MAX_STRETCH)


def test_abi_exports_the_entries():
    from strique_amd import ffi
    lib = ffi.load_library()
    assert lib.strq_abi_version() == 13          # the entry is additive
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    for name in ("strq_debug_flank_mod_bounds", "strq_target_set_flank_mod", "strq_set_flank_mod", "strq_batch_fetch_flank_mod", "strq_last_flank_mod",
                 "strq_batch_fetch_flank_ranges"):
        getattr(lib, name)
        assert "int %s(" % name in header
    assert ffi.Context.debug_flank_mod_bounds and ffi.Context.set_flank_mod and ffi.Context.batch_fetch_flank_mod and ffi.Context.batch_fetch_flank_ranges
    # strq_flank_mod_group: six int32, two int64, two doubles
    assert ffi.FLANK_MOD_DTYPE.itemsize == 56 and ffi.FLANK_MOD_DTYPE.fields["begin"][1] == 24 and ffi.FLANK_MOD_DTYPE.fields["v_mod"][1] == 48
    assert "typedef struct {\n    int32_t flank, pos, n_sites, n_columns, status, pad_;\n    int64_t begin, end;\n    double v_base, v_mod;\n} strq_flank_mod_group;" in header


@pytest.mark.parametrize("argv,needle", [
    (["--flank-mod", "f.tsv"], "--flank-mod needs --mod_model"),
    (["--flank-mod", "f.tsv", "--mod_model", "m.model", "--scan", "--scan-min-score", "5"], "--flank-mod cannot be combined with --scan"),
])
def test_cli_refusals(capsys, argv, needle):
    from strique_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.count(["reads.fofn", "r9.model", "repeats.tsv"] + argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


def test_cli_output_table_and_blob():
    """The flank_mod entry of OUTPUTS: in front of tracts (anchored stays last), its value from a Detected record, and its field of
    the gather blob back bit for bit."""
    from strique_amd import cli, flank_mod as fm
    from strique_amd.counter import Detected
    names = [o.name for o in cli.OUTPUTS]
    assert names.index("flank_mod") < names.index("tracts") and names[-1] == "anchored" and cli.Merged(None, None, None, None, None).flank_mod is None
    calls = [(0, 3, 1, 5, fm.SCORED, 100, 140, -12.345678901234567), (1, 140, 3, 9, fm.EDGE, -1, -1, float("nan")), (1, 7, 2, 8, fm.SCORED, 10, 50, 0.1)]
    det = Detected((17, 1.0, 2.0, -3.0, 4, 5, "-"), None, None, None, flank_mod=calls)
    _, _, row, values = cli._read_values("htt", "+", det)
    assert values["flank_mod"] == [(0, 3, 1, -12.345678901234567), (1, 140, 3, None), (1, 7, 2, 0.1)]
    on = cli.outputs_on(flank_mod=True)
    blob = cli.pack_blob(on, "htt", "+", "-", values)
    assert cli.unpack_blob(on, blob)[3]["flank_mod"] == values["flank_mod"]
    assert cli.unpack_blob(on, cli.pack_blob(on, "htt", "+", "-", dict(flank_mod=None)))[3]["flank_mod"] is None
    o = on[0]
    assert o.format("r1", "htt", "+", row, values["flank_mod"]) == "r1\thtt\t+\t17\t3\tp:3:1:-12.3457,s:140:3:-,s:7:2:0.1000"
    assert o.format("r1", "htt", "+", row, None) == "r1\thtt\t+\t17\t0\t-" and o.header(None) == fm.HEADER


# ---- what the GPU tests take from the reference ----------------------------------------------------------------------------------------
class _Arrays(object):
    def __init__(self, model):
        self.__dict__.update(model.baked._asdict()); self.column_of = model.column_of


@pytest.mark.parametrize("names,as_int16", [(("c9orf72", "htt"), True), (("c9orf72",), False)])
def test_reference_ties_stay_under_the_cap(tables, cfg, targets, pm, names, as_int16):
    """The oracle alone, under both in-edge orders (its own net, the arrays bake() makes): at most TIE_CAP of the (read, group)
    pairs of a parametrisation of tests/test_gpu_flank_mod_models.py differ.  Along the way: every scorer mode occurs, scored and
    edge groups occur, and reads made from the mCpG table score above reads made from the base table."""
    from strique_amd import hmm
    cases, opm, opm_mod = fr.cases(tables, cfg, targets, names, as_int16)
    assert len(cases) == 4 * len(names) and all(c["sig"].dtype == (np.int16 if as_int16 else np.float64) for c in cases)
    pairs = ties = 0
    status, modes, llr = set(), set(), {"base": [], "mod": []}
    for c in cases:
        for which, flank, b, e, x in c["flanks"]:
            assert 0 <= b < e <= len(c["sig"]) and len(x) == e - b and not fr.MAX_STRETCH * len(flank) < len(x)
            res = fr.call(x, flank, opm, opm_mod, cfg["HMM"], alt=_Arrays(hmm.FlankProfileModel(flank, pm, cfg["HMM"])))
            for g in res:
                pairs += 1; ties += g["tie"]; status.add(g["status"])
                if g["status"] == fr.SCORED:
                    assert 0 <= g["u"] < g["w"] - 1 < len(x) and np.isfinite([g["v_base"], g["v_mod"]]).all(), g
                    modes.add(0 if g["n_columns"] <= 7 else (1 if g["n_columns"] <= 15 else 2))
                    llr[c["table"]].append(g["v_mod"] - g["v_base"])
                else:
                    assert (g["u"], g["w"]) == (-1, -1) and np.isnan([g["v_base"], g["v_mod"]]).all(), g
    print("flank-mod reference: %d pairs, %d ties, statuses %s, modes %s" % (pairs, ties, sorted(status), sorted(modes)))
    assert ties <= fr.TIE_CAP * pairs, (ties, pairs)
    assert {fr.SCORED, fr.EDGE} <= status and (modes == {0, 1, 2} if "htt" in names else modes >= {0, 2})
    assert np.median(llr["mod"]) > 0 > np.median(llr["base"])
