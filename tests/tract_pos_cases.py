"""The nine-read set of the tract pipeline tests, rebuilt for the tract-position tests (tests/test_gpu_tracts.py keeps its own): 6 to
10 kb reads of both compound loci on both strands, K = 2 and 3, a read whose gate fails (its flanks in the wrong order) and one of
a target without tracts.  The signals come from the product's synthesiser; what the reference makes of them from
tests/tract_pos_ref.py.  Built once per process and shared by the CPU tie guard and the GPU pipeline test."""
import numpy as np

import tract_pos_ref as tpr
import tract_ref as tr

# (target, strand, planted or None, what)
PIPELINE_READS = [
    ("htt_like", "+", (12, 7), "read"), ("htt_like", "-", (5, 9), "read"), ("cnbp_like", "+", (9, 6, 11), "read"), ("cnbp_like", "-", (6, 10, 7), "read"),
    ("htt_like", "+", (30, 4), "read"), ("cnbp_like", "-", (15, 3, 8), "read"), ("htt_like", "+", (8, 8), "swapped"), ("plain", "+", None, "plain"),
    ("htt_like", "-", (21, 16), "read"),
]
FLANKED_REPEAT = {"htt_like": "CAG", "cnbp_like": "CCTG"}
SEED = 4100          # read i is drawn from PCG64(SEED + i); the tie guard of tests/test_tract_positions_host.py holds for every read


def full_flanks(cfg):
    return cfg["repeat"]["c9orf72"][4].upper(), cfg["repeat"]["c9orf72"][5].upper()


def pipeline_signal(table, cfg, i, target, strand, planted, what):
    from strique_amd import synth
    prefix, suffix = full_flanks(cfg)
    rng = np.random.Generator(np.random.PCG64(SEED + i))
    total = 6000 + 450 * i
    if what == "plain":
        seq = synth.make_sequence(rng, total, prefix, cfg["repeat"]["c9orf72"][3], 20, suffix, strand)
    else:
        array = tr.array_of(*tr.LOCI[target], planted)
        # the whole array as `repeat`, once; "swapped": the suffix in front of the prefix, so that the gate fails
        seq = synth.make_sequence(rng, total, suffix, array, 1, prefix, strand) if what == "swapped" else synth.make_sequence(rng, total, prefix, array, 1, suffix, strand)
    return synth.make_signal(rng, table, seq, True, 0.0)


_PIPELINE = {}


def pipeline(pm, opm, orc, cfg):
    """[(item, row, record, (prefix_begin, window or None), model or None)]: item = (target, signal, strand); record = None or
    (counts, log_p, positions) of the reference on its own un-baked net, configured order; model = (tract_ref.model dict, strand)."""
    from conftest import oracle_map
    from strique_amd import synth
    key = (id(pm), id(opm))
    if key in _PIPELINE:
        return _PIPELINE[key]
    table = synth.KmerTable(pm)
    prefix, suffix = full_flanks(cfg)
    params = orc.align_params(cfg["align"])
    jobs = []
    for i, (target, strand, planted, what) in enumerate(PIPELINE_READS):
        sig = pipeline_signal(table, cfg, i, target, strand, planted, what)
        repeat = cfg["repeat"]["c9orf72"][3] if target == "plain" else FLANKED_REPEAT[target]
        tc = orc.classifier(repeat, prefix, suffix, strand, opm, None, cfg["HMM"])
        m = None if target == "plain" else (tr.model(*tr.LOCI[target], prefix[-50:], suffix[:50], strand, opm, cfg["HMM"]), strand)
        jobs.append(((target, sig, strand), tc, m))

    def one(job):
        item, tc, m = job
        row, b, x = tpr.window(item[1], tc, opm, params)
        rec = None if m is None else tpr.record_on(m[0]["prep"], m[0]["tract_of"], m[0]["K"], m[0]["bias"], m[1], b, x)
        return item, row, rec, (b, x), m

    out = oracle_map(one, jobs)
    # the cases are what they claim: the swapped read fails the gate, the plain read is decoded, every other read has a record
    for (target, strand, planted, what), (_, row, rec, _, _) in zip(PIPELINE_READS, out):
        assert (rec is not None) == (what == "read"), (target, strand, what, row)
        assert (row[3] == 0) == (what == "swapped"), (target, strand, what, row)
    _PIPELINE[key] = out
    return out
