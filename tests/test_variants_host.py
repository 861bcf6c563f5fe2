"""count --variants without a GPU: the ABI, hmm.RepeatVariantModel against the helper's net, every argument error, the TSV, the gather,
and the accuracy of the design on the CPU oracle alone."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import variant_ref
from conftest import ROOT

ENTRIES = ("strq_target_set_variants", "strq_set_variants", "strq_batch_fetch_variants", "strq_last_variants")


def test_entries_are_declared_exported_and_documented():
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    declared = set(re.findall(r"\b(strq_[a-z_0-9]+)\s*\(", header))
    assert set(ENTRIES) <= declared
    assert "int strq_target_set_variants(strq_ctx* ctx, int32_t target_id, int32_t model_id, double lo, double hi, int32_t n_alt, int32_t context_units);" in header
    for name in ENTRIES:
        at = header.index("int %s(" % name)
        assert header[:at].rstrip().endswith("*/"), name          # a comment of its own in front of it
    from strique_amd import ffi
    lib = ffi.load_library()
    for name in ENTRIES:
        getattr(lib, name)
    assert lib.strq_abi_version() == 13          # the entries are additive
    assert ffi.Context.set_variants and ffi.Context.batch_fetch_variants


def test_argument_errors_without_a_context():
    from strique_amd import ffi
    lib = ffi.load_library()
    lib.strq_target_set_variants.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32]
    lib.strq_set_variants.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.strq_batch_fetch_variants.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.strq_last_variants.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.strq_target_set_variants(None, 0, 0, 0.0, 1.0, 1, 2) == ffi.STRQ_ERR_ARG
    assert lib.strq_set_variants(None, 1) == ffi.STRQ_ERR_ARG
    off = np.zeros(2, np.int64)
    assert lib.strq_batch_fetch_variants(None, None, None, off.ctypes.data, None, None, 0, None, None, 0, None) == ffi.STRQ_ERR_ARG
    out = np.zeros(4)
    assert lib.strq_last_variants(None, out.ctypes.data) == ffi.STRQ_ERR_ARG


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _as_graph(net):
    """The helper's un-baked net as a product Graph (same states, same edges in the same order), for the product's bake()."""
    from strique_amd import hmm
    g = hmm.Graph.__new__(hmm.Graph)
    g.names, g.kinds, g.params = list(net.name), list(net.kind), list(net.par)
    g.edges = [(a, b, p) for a, b, p in net.edges()]
    g.layout, g.positions = {}, {}
    g.start, g.end = net.start, net.end
    return g


CASES = [("fmr1", ["AGG"], 2, 26), ("fmr1", ["AGG", "CAG", "CGA"], 2, 62), ("c9orf72", ["GGCCTC"], 1, 38), ("c9orf72", ["GGCCTC", "GGACCC", "AGCCCC"], 1, 86)]


@pytest.mark.parametrize("locus,alts,m,n_emit", CASES)
@pytest.mark.parametrize("strand", "+-")
@pytest.mark.parametrize("prior", [None, 0.05])
def test_model_equals_the_helpers_net_after_baking(pm, opm, cfg, targets, locus, alts, m, n_emit, strand, prior):
    from strique_amd import hmm
    from strique_amd.counter import reverse_complement as rc
    config = dict(cfg["HMM"]) if prior is None else dict(cfg["HMM"], variant_prior=prior)
    repeat = targets[locus][0]
    r, a = (repeat, alts) if strand == "+" else (rc(repeat), [rc(x) for x in alts])          # as counter.add_target hands them over
    model = hmm.RepeatVariantModel(r, a, pm, config)
    got = model.baked
    assert model.context_units == m and got.silent_start == n_emit == 2 + 2 * len(repeat) + 2 * len(alts) * (m + 1) * len(repeat)
    net, m_ref = variant_ref.variant_net(*variant_ref.strand_units(repeat, alts, strand), opm, config)
    want = hmm.bake(_as_graph(net))
    assert m_ref == m
    strip = lambda names: [n.replace("variant-", "") for n in names]
    assert strip(got.names) == strip(want.names)
    assert np.array_equal(got.in_ptr, want.in_ptr) and np.array_equal(got.in_src, want.in_src)
    assert np.array_equal(got.in_logp.view(np.uint64), want.in_logp.view(np.uint64))
    for f in ("emis_kind", "emis_a", "emis_b", "emis_c"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f
    tags = {"base": 0, "alt1": 1, "alt2": 3, "alt3": 4, "s0": 2, "e0": 2}
    assert [int(t) for t in got.tag[:n_emit]] == [tags[n if n in ("s0", "e0") else n[:4]] for n in got.names[:n_emit]]
    assert got.n_states == n_emit + 2          # no silent state besides start and end
    # the prior: s0's out-edges into the branches
    s0 = got.names.index("s0")
    into = {}
    for l in range(n_emit):
        for e in range(got.in_ptr[l], got.in_ptr[l + 1]):
            if got.in_src[e] == s0:
                into[got.names[l]] = float(np.exp(got.in_logp[e]))
    nb = 1 + len(alts)
    p_alt = 1.0 / nb if prior is None else prior
    for name, p in into.items():
        assert name.startswith(("base", "alt")) and abs(p - (p_alt if name.startswith("alt") else 1 - (nb - 1) * p_alt) / 2) < 1e-12
    assert len(into) == 2 * nb
    # one slot when the model fits 64 lanes
    assert (got.hint_lane[:n_emit] >= 0).all() == (n_emit <= 64)


def test_dual_models_keep_their_tags_and_bake_its_results(pm, pm_mod, cfg, targets):
    from strique_amd import hmm
    mod = hmm.RepeatModModel(targets["c9orf72"][0], pm, pm_mod, cfg["HMM"])
    assert set(int(t) for t in mod.baked.tag) == {0, 1, 2}
    again = hmm.bake(mod.graph, count_states=(), tag_substring="mod", tag2_states=mod.hub_states)
    assert np.array_equal(again.tag, mod.baked.tag) and np.array_equal(again.in_logp, mod.baked.in_logp)


@pytest.mark.parametrize("alts,word", [([], "between 1 and 3"), (["AGG", "CAG", "CGA", "TGG"], "between 1 and 3"), (["AGN"], "'AGN'"), (["AG"], "'AG'"),
                                       (["AGGA"], "'AGGA'"), (["cgg"], "'CGG' is the repeat unit"), (["AGG", "agg"], "'AGG' is given twice"), ([""], "''")])
def test_alt_units_that_are_refused_name_the_unit(pm, alts, word):
    from strique_amd import hmm
    with pytest.raises(ValueError) as ei:
        hmm.RepeatVariantModel("CGG", alts, pm)
    assert word in str(ei.value)


def test_variant_prior_must_leave_the_base_branch_something(pm):
    from strique_amd import hmm
    with pytest.raises(ValueError, match="variant_prior"):
        hmm.RepeatVariantModel("CGG", ["AGG", "CAG"], pm, {"variant_prior": 0.5})


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_alt_units_file_is_parsed_and_every_error_has_its_message():
    from strique_amd import cli
    repeats = {"fmr1": "CGG", "c9orf72": "GGCCCC"}
    text = "# interruptions\n\nfmr1\tagg,CAG   # two\nc9orf72\tGGCCTC\n"
    assert cli.parse_alt_units(io.StringIO(text), repeats) == {"fmr1": ["AGG", "CAG"], "c9orf72": ["GGCCTC"]}
    for bad, word in (("htt\tCAA\n", "unknown target htt"), ("fmr1\tAGGA\n", "'AGGA': 4 nt"), ("fmr1\tAGG,AGG\n", "'AGG' is given twice"),
                      ("fmr1\tAGG,CAG,CGA,TGG\n", "4 units for target fmr1, at most 3"), ("fmr1\tAGG\nfmr1\tCAG\n", "target fmr1 is given twice"),
                      ("fmr1\tCGG\n", "is the repeat unit itself"), ("fmr1\tAGN\n", "only the letters"), ("fmr1\n", "expected target<TAB>unit")):
        with pytest.raises(ValueError) as ei:
            cli.parse_alt_units(io.StringIO(bad), repeats)
        assert word in str(ei.value) and "line" in str(ei.value), (bad, str(ei.value))


def test_variants_needs_alt_units_and_excludes_scan(capsys):
    from strique_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["count", "reads.fofn", "model", "repeats.tsv", "--variants", "v.tsv"])
    assert ei.value.code == 2 and "--variants needs --alt-units" in capsys.readouterr().err
    with pytest.raises(SystemExit) as ei:
        cli.main(["count", "reads.fofn", "model", "repeats.tsv", "--alt-units", "a.tsv", "--variants", "v.tsv", "--scan", "--scan-min-score", "5"])
    assert ei.value.code == 2 and "--variants cannot be combined with --scan" in capsys.readouterr().err


def _raw(pattern_branches, m=2, bias=1):
    """What the counter hands out for a read with these passages: (count_v, pattern, branch, end, V)."""
    br = np.array(pattern_branches, np.int8)
    pat = variant_ref.pattern_of(br, m)
    V = np.array([[-100.0 - j, -90.0 + 3 * j if b == 1 else -400.0, -95.0 if b == 2 else -np.inf][:3] for j, b in enumerate(br)]).reshape(len(br), 3)
    return len(pat) + bias, pat, br, np.arange(len(br), dtype=np.int64) * 50 + 1000, V


def test_variant_rows_are_formatted_and_parsed():
    from strique_amd import cli
    units = ["AGG", "CAG"]
    v = cli.variant_value(_raw([0, 0, 1, 0, 2, 0]), units)
    assert v == (11, 6, "0000100020", [(4, "AGG", 1100, 18.0), (8, "CAG", 1200, 9.0)])
    rows = [cli.format_variants("r1", "fmr1", "+", 9, v),
            cli.format_variants("r2", "fmr1", "-", 0, None),                                       # not decoded
            cli.format_variants("r3", "fmr1", "-", 4, cli.variant_value(_raw([0, 0, 0]), units)),      # decoded, no alt call
            cli.format_variants("r4", "fmr1", "+", 2, cli.variant_value(_raw([]), units))]            # decoded, no passage
    assert rows[0] == "r1\tfmr1\t+\t9\t11\t6\t2\t0000100020\t4:AGG:1100:18.0000,8:CAG:1200:9.0000"
    assert rows[1] == "r2\tfmr1\t-\t0\t-\t-\t-\t-\t-"
    assert rows[2] == "r3\tfmr1\t-\t4\t4\t3\t0\t000\t-" and rows[3] == "r4\tfmr1\t+\t2\t1\t0\t0\t-\t-"
    buf = io.StringIO()
    cli.write_rows(buf, list(enumerate(rows)), header=cli.VARIANTS_HEADER)
    text = buf.getvalue()
    assert text.splitlines()[0] == "ID\ttarget\tstrand\tcount\tcount_v\tn_passages\tn_alt\tpattern\tcalls"
    assert cli.parse_variants(io.StringIO(text)) == [("r1", "fmr1", "+", 9, 11, 6, "0000100020", [(4, "AGG", 1100, 18.0), (8, "CAG", 1200, 9.0)]),
                                                     ("r2", "fmr1", "-", 0, None, None, None, []),
                                                     ("r3", "fmr1", "-", 4, 4, 3, "000", []), ("r4", "fmr1", "+", 2, 1, 0, "", [])]
    # between ranks the ratios travel as repr(): bit for bit
    w = (7, 2, "0001", [(3, "AGG", 12, 0.1 + 0.2)])
    assert cli._unpack_variants(cli._pack_variants(w)) == w and cli._unpack_variants(cli._pack_variants((1, 0, "", []))) == (1, 0, "", [])
    assert cli.variant_value(None, units) is None
    assert "variants" in [o.name for o in cli.OUTPUTS] and cli.Merged(None, None, None, None, None).variants is None


VARIANTS_WORKER = r'''
import io, json, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
from strique_amd import cli, dist as sdist
from strique_amd.counter import Detected
import variant_ref
rank, world, local = sdist.init_process_group(backend="gloo")
cfg = json.load(open(os.path.join(%r, "tests", "golden", "config.json")))
loci = {}
for name, (chrom, b, e, *_r) in cfg["repeat"].items():
    loci.setdefault(chrom, []).append((name, b, e))
lines = ["@HD\tVN:1.0"]
for i in range(29):
    chrom, pos = ("chr9", 27570000) if i %% 3 else ("chrX", 146990000)
    lines.append("\t".join(["read%%d" %% i, "16" if i %% 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))
ALTS = {"fmr1": ["AGG", "CAG"], "c9orf72": ["GGCCTC"]}

class FakeCounter(object):                               # stands in for the GPU engine: rows and variants depend on the inputs only
    variants = False
    def set_variants(self, on):
        self.variants = bool(on)
    def detect_batch(self, items, units=False, records=False):
        variants = self.variants
        out = []
        for t, raw, s in items:
            row = (len(raw) %% 97, 1.5, 2.5, -3.0 * len(t), int(raw[0]), 7, "-")
            var = None
            if variants and len(raw) %% 5:
                nb = 1 + len(ALTS[t]); m = 2 if t == "fmr1" else 1
                br = np.array([(j * len(raw)) %% 7 %% nb if j %% 3 == 2 else 0 for j in range(len(raw) %% 11)], np.int8)
                pat = variant_ref.pattern_of(br, m)
                V = -np.abs(np.sin(np.arange(len(br) * nb, dtype=np.float64) + len(raw))).reshape(len(br), nb) * 1e3 / 7
                var = (len(pat) + 1, pat, br, np.arange(len(br), dtype=np.int64) * 40 + int(raw[0]), V)
            pos = np.arange(len(raw) %% 7, dtype=np.int64) * 13 + int(raw[0])
            det = Detected(row, pos if units else None, None, None, None, var)
            assert records or not variants
            out.append(det if records else ((row, pos) if units else row))
        return out

def get_raw(qname):
    i = int(qname[4:])
    return np.arange(100 + i, 300 + 2 * i)

log = cli.Log("error")
stats = {}
mine = cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, rank, world, stats=stats, units=True, variants=ALTS)
got = cli.gather_rows(mine, stats["items"], sdist, units=True, variants=True)       # still one gather: records + one blob per row
import torch.distributed as dist
if rank == 0:
    buf = io.StringIO(); cli.write_rows(buf, got.rows)
    ubuf = io.StringIO(); cli.write_rows(ubuf, got.units, header=cli.UNITS_HEADER)
    vbuf = io.StringIO(); cli.write_rows(vbuf, got.variants, header=cli.VARIANTS_HEADER)
    one = io.StringIO(); uone = io.StringIO(); vone = io.StringIO(); st1 = {}
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, one, stats=st1, units=True, units_out=uone, variants=ALTS, variants_out=vone)
    plain = io.StringIO(); uplain = io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, plain, units=True, units_out=uplain)
    assert buf.getvalue() == one.getvalue() == plain.getvalue()
    assert ubuf.getvalue() == uone.getvalue() == uplain.getvalue()
    assert vbuf.getvalue() == vone.getvalue(), (vbuf.getvalue(), vone.getvalue())
    assert len(vone.getvalue().splitlines()) == len(one.getvalue().splitlines()) == 30
    assert [r[1] for r in st1["variant_rows"]] == vone.getvalue().splitlines()[1:]
    parsed = cli.parse_variants(io.StringIO(vone.getvalue()))
    assert any(r[4] is None for r in parsed) and any(r[7] for r in parsed) and any(r[4] is not None and not r[7] for r in parsed)
    print("VARIANTS_GATHER_OK")
else:
    assert got.rows is None and got.variants is None
dist.barrier(); dist.destroy_process_group()
''' % (ROOT, ROOT, ROOT)


def test_two_rank_gather_carries_the_variant_rows(tmp_path):
    """`count --variants` under torchrun: the calls ride in the byte pool of the one gather, and rank 0's rows equal the single-process
    ones; the count rows and the unit rows are those of a run without the flag."""
    script = tmp_path / "variants_worker.py"
    script.write_text(VARIANTS_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "VARIANTS_GATHER_OK" in outs[0]


# ---- accuracy of the design, on the oracle alone --------------------------------------------------------------------------------
PROBE = [("fmr1", "AGG"), ("c9orf72", "GGCCTC")]


@pytest.mark.parametrize("locus,alt", PROBE)
@pytest.mark.parametrize("strand", "+-")
def test_planted_interruptions_are_called_at_their_index_and_the_count_is_corrected(pm, opm, orc, cfg, targets, locus, alt, strand):
    """The 16 probe reads of the issue: clean synthetic reads (PCG64(1000 + r), r = 0 .. 3 per target and strand), 3000 nt of background on
    either side of prefix + 60 units + suffix, four units at [8, 20, 32, 44] + U{0..3} replaced by the alt unit.  Every planted unit is
    called with the right alt at its exact pattern index, there is no extra call, and count_v = 60."""
    from strique_amd import synth
    params = orc.align_params(cfg["align"])
    tc = orc.classifier(*targets[locus], strand, opm, None, cfg["HMM"])
    vm = variant_ref.VariantModel(targets[locus][0], [alt], strand, opm, cfg["HMM"])
    for r in range(4):
        sig, planted = synth.make_variant_read(1000 + r, synth.KmerTable(pm), targets[locus], 60, alt, strand)
        ref = variant_ref.reference(sig, tc, opm, params, vm)
        assert ref["decoded"]
        print(locus, strand, r, "count", ref["row"][0], "count_v", ref["count_v"], "planted", planted, "called", variant_ref.calls(ref))
        assert variant_ref.calls(ref) == [(p, 1) for p in planted], (r, planted, variant_ref.calls(ref))
        assert ref["count_v"] == 60 and len(ref["pattern"]) + tc["count_bias"] == 60
        # the helper's own properties: passages tile the stretch, the called branch is never worse than the repeat unit's
        assert ref["bounds"][0][0] == 0 and ref["bounds"][-1][1] == len(ref["x"]) - 1
        for (u0, w0), (u1, w1) in zip(ref["bounds"], ref["bounds"][1:]):
            assert u1 == w0 + 1 and w0 >= u0 + 2
        for j, b in enumerate(ref["branch"]):
            assert ref["V"][j, b] - ref["V"][j, 0] >= -1e-9
        assert np.array_equal(ref["end"], ref["first"] + np.array([w for _, w in ref["bounds"]]))
