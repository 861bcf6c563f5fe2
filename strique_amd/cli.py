"""`STRique.py`-compatible command line: `index` and `count`.

Mirrors the reference's CLI surface (scripts/STRique.py:874-945): same positional arguments and
flags, the same `repeat_config.tsv` / JSON config format (parse_config, :836-868), SAM record
decoding and locus intersection (repeatDetector, :648-705) and TSV output (outputWriter, :711-727).
What changes is the engine: instead of `--t` worker processes calling the CPU aligner one read at
a time, the records of the SAM stream are collected and handed to the GPU in batches
(`repeatCounter.detect_batch`); rows are written in input order.
"""
import argparse
import contextlib
import glob
import json
import os
import re
import sys
import tarfile
import tempfile
import threading
from collections import defaultdict, deque, namedtuple

import numpy as np

from . import anchored as anchored_mod
from . import flank_mod as flank_mod_rule
from . import motifs as motifs_mod
from . import renorm as renorm_mod
from . import scan as scan_mod
from . import tracts as tracts_mod
from .counter import Detected

HEADER = ['ID', 'target', 'strand', 'count', 'score_prefix', 'score_suffix', 'log_p', 'offset', 'ticks', 'mod']
# `count --units FILE`: the raw-signal sample of every repeat unit on the decoded Viterbi path, one row per count row
UNITS_HEADER = ['ID', 'target', 'strand', 'count', 'n_units', 'units']
# `count --confidence FILE`: forward log-likelihood and posterior mean / standard deviation of the count, one row per count row
CONF_HEADER = ['ID', 'target', 'strand', 'count', 'log_p', 'log_lik', 'count_mean', 'count_sd']
# `count --mod_model M --mod-llr FILE`: log-likelihood ratio (modified over unmodified) of every unit of the pattern, one row per count row
MODLLR_HEADER = ['ID', 'target', 'strand', 'count', 'mod_pattern', 'n_units', 'llr']
# `count --alt-units FILE --variants OUT`: the interruption calls of every read, one row per count row; calls: index:unit:sample:llr per alt call
VARIANTS_HEADER = ['ID', 'target', 'strand', 'count', 'count_v', 'n_passages', 'n_alt', 'pattern', 'calls']
LEVELS = ['error', 'warning', 'info', 'debug']


class Log(object):
    """Messages to stderr.  The engine thread of `run_count` logs while the main thread does: one write per message,
    under a lock, so that lines never interleave."""

    def __init__(self, level='warning'):
        import threading
        self.level = LEVELS.index(level)
        self._lock = threading.Lock()

    def __call__(self, message, level='info'):
        if LEVELS.index(level) <= self.level:
            with self._lock:
                sys.stderr.write("[%s] %s\n" % (level.upper(), message))
                sys.stderr.flush()


def parse_config(repeat_config_file, param_config_file=None, log=None):
    """{'repeat': {name: (chr, begin, end, repeat, prefix, suffix)}, 'align': dict|None, 'HMM': dict|None}"""
    repeats = {}
    with open(repeat_config_file, 'r') as fp:
        next(fp)                                         # header line
        for line in fp:
            cols = line.rstrip().split()
            if len(cols) == 7:
                repeats[cols[3]] = (cols[0], int(cols[1]), int(cols[2]), cols[4], cols[5], cols[6])
            elif log:
                log("Config: Repeat config column mismatch while parsing \n%s" % line, 'error')
    config = {'repeat': repeats, 'align': None, 'HMM': None}
    if param_config_file:
        with open(param_config_file) as fp:
            ld_conf = json.load(fp)
        if not isinstance(ld_conf, dict):
            raise SystemExit('Config: file format broken')
        for key in ('align', 'HMM'):
            if key not in ld_conf:
                raise SystemExit('Config: Error loading HMM config file, missing %s' % key)
            if not isinstance(ld_conf[key], dict):
                raise SystemExit('Config: file format broken')
        config['align'] = ld_conf['align']
        config['HMM'] = ld_conf['HMM']
    return config


class SamRecord(object):
    __slots__ = ('QNAME', 'FLAG', 'RNAME', 'POS', 'TLEN', 'CLIP_BEGIN', 'CLIP_END', 'QLEN')

    def __init__(self):
        self.QNAME = ''; self.FLAG = 0; self.RNAME = ''; self.POS = 0; self.TLEN = 0; self.CLIP_BEGIN = 0; self.CLIP_END = 0; self.QLEN = 0


def decode_cigar(cigar):
    return [(int(op[:-1]), op[-1]) for op in re.findall(r'(\d*\D)', cigar)]


def ops_length(ops, recOps='MIS=X'):
    return sum(n for n, op in ops if op in recOps)


def decode_sam(sam_line):
    """QNAME, FLAG, RNAME, POS, reference span from the CIGAR, soft/hard clips (STRique.py:656-671)."""
    cols = sam_line.rstrip().split('\t')
    sr = SamRecord()
    if len(cols) >= 11:
        try:
            sr.QNAME = cols[0]; sr.FLAG = int(cols[1]); sr.RNAME = cols[2]; sr.POS = int(cols[3])
            ops = decode_cigar(cols[5])
            sr.TLEN = ops_length(ops, recOps='MDN=X')
            sr.CLIP_BEGIN = sum(n for n, op in ops[:2] if op in 'SH')
            sr.CLIP_END = sum(n for n, op in ops[-2:] if op in 'SH')
            sr.QLEN = max(ops_length(ops, recOps='MIS=XH'), len(cols[9]) if cols[9] != '*' else 0)      # read length: the cost of its alignments
        except Exception:
            return SamRecord()
    return sr


def intersect_targets(sr, loci):
    """Targets whose locus lies inside the (clip-extended) alignment (STRique.py:673-679)."""
    return [name for name, begin, end in loci.get(sr.RNAME, [])
            if begin > sr.POS - sr.CLIP_BEGIN and end < sr.POS + sr.TLEN + sr.CLIP_END]


class Fast5Index(object):
    """`path[.fast5/group | .tar/member]<TAB>read_id` index (STRique_lib/fast5Index.py:45-60,220-233)."""

    def __init__(self, index_file):
        if not os.path.exists(index_file):
            raise RuntimeError("[Error] Raw fast5 index file %s not found." % index_file)
        with open(index_file) as fp:
            self.index = {rid: path for path, rid in (line.split('\t') for line in fp.read().split('\n') if line)}
        self.dir = os.path.dirname(index_file)
        self._joined = {}
        self._open = {}                  # path -> H5File, the few most recently used (bulk files hold thousands of reads)
        self._lock = threading.Lock()

    def _join(self, rel):
        """os.path.join(self.dir, rel), memoised per file (thousands of reads share a bulk file)."""
        full = self._joined.get(rel)
        if full is None:
            full = self._joined[rel] = os.path.join(self.dir, rel)
        return full

    def _file(self, path):
        from . import fast5
        with self._lock:                 # get_raw may be called from the reader threads of `count`
            f = self._open.pop(path, None)
            if f is None:
                f = fast5.H5File(path)
                # dozens of reader threads work on tasks from several bulk files at once: with only a few files kept, every
                # task re-opened (mmap) and dropped (munmap: a TLB shoot-down on every CPU the process runs on) its file
                while len(self._open) >= 32:
                    self._open.pop(next(iter(self._open)))
            self._open[path] = f         # most recently used last
            return f

    def get_raw(self, read_id, alloc=None, defer=False):
        """The raw signal of a read, or None.  `alloc`, `defer`: see fast5.H5File.dataset (compressed datasets: where the output
        array comes from; an InflatePlan instead of the samples, for fast5.inflate_plans to fill a whole task's reads at once)."""
        from . import fast5
        where = self.index.get(read_id)
        if where is None:
            return None
        cut = where.find('.fast5/')          # the common case, a read of a bulk file, without the regular expression
        if cut >= 0 and '.tar/' not in where:
            f = self._file(self._join(where[:cut + 6]))
            return f.dataset("/%s/Raw/Signal" % where[cut + 7:].strip('/'), alloc, defer)
        parts = re.split(r'(\.fast5|\.tar)/', where)
        if len(parts) == 1:
            f = self._file(os.path.join(self.dir, parts[0]))
            grp = "/Raw/Reads/" + f.listdir("/Raw/Reads")[0]
            return f.dataset(grp + "/Signal", alloc, defer)
        if parts[1] == '.fast5':
            f = self._file(os.path.join(self.dir, parts[0] + '.fast5'))
            return f.dataset("/%s/Raw/Signal" % parts[2].strip('/'), alloc, defer)
        with tarfile.open(os.path.join(self.dir, parts[0] + '.tar')) as tar:
            data = tar.extractfile(tar.getmember(parts[2])).read()
        f = fast5.H5File(data)
        return f.dataset("/Raw/Reads/" + f.listdir("/Raw/Reads")[0] + "/Signal")

    @staticmethod
    def index_records(path, recursive=False, out_prefix=""):
        from . import fast5
        if os.path.isfile(path):
            files = [path]
        elif recursive:
            files = [os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs if f.endswith(('.fast5', '.tar'))]
        else:
            files = glob.glob(os.path.join(path, '*.fast5')) + glob.glob(os.path.join(path, '*.tar'))
        for fpath in sorted(files):
            rel = os.path.normpath(os.path.join(out_prefix, os.path.dirname(os.path.relpath(fpath, start=path)), os.path.basename(fpath)))
            if fpath.endswith('.tar'):
                with tarfile.open(fpath) as tar:
                    for m in tar.getmembers():
                        if m.name.endswith('.fast5'):
                            try:
                                rid = fast5.read_raw(tar.extractfile(m).read())[0][0]
                                yield "\t".join([os.path.normpath(os.path.join(rel, m.name)), rid])
                            except Exception:
                                print("[ERROR] Failed to open %s, skip file for indexing" % m.name, file=sys.stderr)
                continue
            try:                                      # like the reference: a file that cannot be opened is reported and skipped
                f = fast5.H5File(fpath)
                top = f.listdir("/")
                recs = []
                if "Raw" in top:
                    rd = f.listdir("/Raw/Reads")[0]
                    grp = "/Raw/Reads/" + rd
                    rid = f.attrs(grp).get("read_id")
                    if rid is None:                       # attribute in a form the subset reader does not decode
                        rid = os.path.splitext(os.path.basename(fpath))[0]
                    recs.append("\t".join([rel, rid]))
                else:
                    for g in top:
                        if g.startswith("read_"):
                            recs.append("\t".join([os.path.join(rel, g), f.attrs("/%s/Raw" % g).get("read_id", g[5:])]))
            except Exception as e:
                print("[ERROR] Failed to open %s (%s), skip file for indexing" % (fpath, e), file=sys.stderr)
                continue
            for r in recs:
                yield r


def count(argv):
    parser = argparse.ArgumentParser(description="STR Detection in raw nanopore data")
    parser.add_argument("f5Index", help="Fast5 index")
    parser.add_argument("model", help="Pore model")
    parser.add_argument("repeat", help="Repeat region config file")
    parser.add_argument("--out", default=None, help="Output file name, if not given print to stdout")
    parser.add_argument("--algn", default=None, help="Alignment in sam format, if not given read from stdin")
    parser.add_argument("--mod_model", default=None, help="Base modification pore model")
    parser.add_argument("--config", help="Config file with HMM transition probabilities")
    parser.add_argument("--t", type=int, default=0, help="Reader threads that fetch and inflate raw signals ahead of the GPU batches (the reference's worker-process count); "
                                                          "0 (default): this rank's share of the CPUs the job may use (affinity mask, cgroup quota), at most 24")
    parser.add_argument("--log_level", default='warning', choices=LEVELS, help="Log level")
    parser.add_argument("--batch", type=int, default=2048, help="Reads per GPU batch.  (The library works in sub-batches of 16 reads per CU, two of them in flight, so a batch of "
                                                                "8192 and more keeps the HMM decode of one sub-batch under the alignments of the next -- but `count` is bound by reading "
                                                                "the files, and smaller batches keep readers and GPU busy at the same time: profiles/r06_cli_probe.txt)")
    parser.add_argument("--device", type=int, default=0, help="HIP device")
    parser.add_argument("--backend", default=None, choices=["nccl", "gloo"], help="torch.distributed backend when launched with torchrun (default: nccl = RCCL)")
    parser.add_argument("--share-device", action="store_true", help="testing: every rank uses --device instead of its LOCAL_RANK")
    parser.add_argument("--units", default=None, metavar="FILE", help="Also write the repeat-unit positions (raw-signal sample of every repeat unit "
                                                                        "on the decoded path) to FILE: one row per count row, columns " + " ".join(UNITS_HEADER))
    parser.add_argument("--confidence", default=None, metavar="FILE", help="Also write how far to trust each count to FILE: the forward log-likelihood of the decoded "
                                                                             "window (all paths, where log_p is the best one) and the posterior mean and standard deviation "
                                                                             "of the count; one row per count row, columns " + " ".join(CONF_HEADER))
    parser.add_argument("--mod-llr", dest="mod_llr", default=None, metavar="FILE", help="With --mod_model: also write how far to trust each methylation call to FILE: per repeat unit of "
                                                                                        "the pattern the log-likelihood ratio of the modified over the unmodified branch (positive: "
                                                                                        "modified); one row per count row, columns " + " ".join(MODLLR_HEADER))
    parser.add_argument("--alt-units", dest="alt_units", default=None, metavar="FILE", help="Sequence variants of the repeat unit (interruptions) to tell from it: a TSV of "
                                                                                          "target<TAB>unit[,unit...] (at most 3 units per target, as long as its repeat unit, on the "
                                                                                          "+ strand like it; # comments and blank lines allowed)")
    parser.add_argument("--variants", default=None, metavar="FILE", help="With --alt-units: also write which repeat units of a read are one of the alt units, and a count "
                                                                           "corrected for them, to FILE: one row per count row, columns " + " ".join(VARIANTS_HEADER) +
                                                                           " (calls: index:unit:sample:llr per alt call -- its index in pattern, the unit as configured, the raw "
                                                                           "sample behind it, the log-likelihood ratio of the best alt branch over the repeat unit)")
    parser.add_argument("--tract-units", dest="tract_units", default=None, metavar="FILE", help="Compound repeat loci -- several tracts in a fixed order, as (CAG)n CAACAG (CCG)m: a TSV "
                                                                                              "of target<TAB>U0,U1[,U2][<TAB>L0[,L1]] (2 or 3 units and the linkers between them on the + "
                                                                                              "strand; - or no third column: empty linkers; # comments and blank lines allowed)")
    parser.add_argument("--tracts", default=None, metavar="FILE", help="With --tract-units: also write the unit count of every tract of a read to FILE: one row per count row, "
                                                                       "columns " + " ".join(tracts_mod.HEADER) + " (counts in the configured order, joined by commas)")
    parser.add_argument("--tract-positions", dest="tract_positions", default=None, metavar="FILE", help="With --tract-units and --tracts: also write where the units of every tract lie in "
                                                                                                       "the raw signal to FILE: one row per count row, columns " + " ".join(tracts_mod.POS_HEADER) +
                                                                                                       " (spans first-last per tract joined by commas; positions joined by commas within a "
                                                                                                       "tract and ; between tracts; - for a tract or a read without positions)")
    parser.add_argument("--motif-units", dest="motif_units", default=None, metavar="FILE", help="Loci whose array may be made of another unit than the configured one (RFC1: AAAAG, "
                                                                                              "AAAGG or AAGGG): a TSV of target<TAB>U1[,U2[,U3]] (1 to 3 alternative units on the + "
                                                                                              "strand, of any length; # comments and blank lines allowed)")
    parser.add_argument("--motifs", default=None, metavar="FILE", help="With --motif-units: also write which unit each stretch of a read's array is made of to FILE: one row per count "
                                                                       "row, columns " + " ".join(motifs_mod.HEADER) + " (shares in the configured order, the configured unit first; runs "
                                                                       "unit:first-end in raw samples; count_m the count under the majority unit)")
    parser.add_argument("--motif-segment", dest="motif_segment", type=int, default=None, metavar="N", help="--motifs: observations per segment, %d to %d (default %d: a resolution "
                                                                                                           "chosen on synthetic reads, not a tuned value)" % (motifs_mod.SEGMENT_MIN, motifs_mod.SEGMENT_MAX, motifs_mod.SEGMENT))
    parser.add_argument("--scan", action="store_true", help="No alignment: every read of the index is compared with every target of the repeat config on both strands, "
                                                             "from its raw signal alone, and counted for the one it spans (if any).  Excludes --algn; stdin is not read")
    parser.add_argument("--scan-min-score", type=float, default=None, metavar="X", help="--scan: the smallest min(score_prefix, score_suffix) a target and strand needs to be "
                                                                                       "taken for a read.  Required with --scan: there is no default (README, 'Scan')")
    parser.add_argument("--scan-scores", default=None, metavar="FILE", help="--scan: also write score_prefix and score_suffix of every candidate to FILE, one row per read, "
                                                                            "with or without a winner (what a threshold for one's own data is chosen from)")
    parser.add_argument("--anchored", default=None, metavar="FILE", help="Also count the reads that end or start inside the repeat, from their one flank, and write them to FILE: "
                                                                           "one row per count row, columns " + " ".join(anchored_mod.HEADER) + " (kind: none, spanning, "
                                                                           "ends_in_repeat, starts_in_repeat; the count is a lower bound up to the decode's own error; "
                                                                           "free_samples in the thousands means the read was wrongly taken for anchored)")
    parser.add_argument("--anchored-min-score", type=float, default=None, metavar="X", help="--anchored: a flank counts as found when its normalised score is at least X.  "
                                                                                           "Required with --anchored: there is no default (README, 'Anchored counting')")
    parser.add_argument("--anchored-mod", dest="anchored_mod", default=None, metavar="FILE", help="With --mod_model and --anchored: also call the methylation pattern of the reads "
                                                                                                  "that end or start inside the repeat, on the samples their record puts into the repeat, and "
                                                                                                  "write it to FILE: one row per count row, columns " + " ".join(anchored_mod.MOD_HEADER) +
                                                                                                  " (llr: the per-unit ratios when --mod-llr is given as well, else -)")
    parser.add_argument("--flank-mod", dest="flank_mod", default=None, metavar="FILE", help="With --mod_model: also call the CpG groups of the configured flanks (one mCpG "
                                                                                            "log-likelihood ratio per group of CpG sites that share a k-mer) and write them to FILE: one row "
                                                                                            "per count row, columns " + " ".join(flank_mod_rule.HEADER) + " (calls: flank p|s : position of "
                                                                                            "the group's first C in the configured flank : sites : ratio, - without a score)")
    parser.add_argument("--renorm", type=float, default=None, metavar="MIN_SHARE", help="Refit scale and shift of every read's normalised signals against its target's k-mer "
                                                                                      "composition, and count on the corrected signals where the fitted repeat share is at least "
                                                                                      "MIN_SHARE (inside (0, 1); there is no default: README, 'Renorm').  The count rows of such "
                                                                                      "reads change: reads that are mostly repeat are the ones detect() loses without it")
    parser.add_argument("--renorm-out", dest="renorm_out", default=None, metavar="FILE", help="--renorm: also write the fit of every read to FILE: one row per count row, columns " +
                                                                                                " ".join(renorm_mod.HEADER) + " ('-' where a signal was not fitted)")
    parser.add_argument("--strict", action="store_true", help="Exit with status 2 when any read could not be processed (the reference only logs such reads and exits 0)")
    args = parser.parse_args(argv)
    if args.variants and not args.alt_units:
        parser.error("--variants needs --alt-units FILE: the units to tell from the repeat unit")
    if bool(args.tracts) != bool(args.tract_units):
        parser.error("--tract-units FILE and --tracts FILE need each other: the definitions, and where the counts go")
    if bool(args.motifs) != bool(args.motif_units):
        parser.error("--motif-units FILE and --motifs FILE need each other: the alternative units, and where the track goes")
    if args.motif_segment is not None and not args.motifs:
        parser.error("--motif-segment N needs --motif-units FILE --motifs FILE")
    if args.motif_segment is not None and not motifs_mod.SEGMENT_MIN <= args.motif_segment <= motifs_mod.SEGMENT_MAX:
        parser.error("--motif-segment N must lie between %d and %d" % (motifs_mod.SEGMENT_MIN, motifs_mod.SEGMENT_MAX))
    if args.tract_positions and not args.tracts:
        parser.error("--tract-positions FILE needs --tract-units FILE --tracts FILE: the positions are those of the tract counts")
    if args.scan and args.algn:
        parser.error("--scan takes the target and strand of a read from its signal: it cannot be combined with --algn")
    if not args.scan and (args.scan_scores or args.scan_min_score is not None):
        parser.error("--scan-min-score and --scan-scores need --scan")
    if args.scan and args.scan_min_score is None:
        parser.error("--scan needs --scan-min-score X: the scores of wrong and of true candidates overlap on noisy reads, so there is no default "
                     "(a first run with a high X and --scan-scores FILE shows what to choose from)")
    if args.scan_min_score is not None and not args.scan_min_score > 0:
        parser.error("--scan-min-score must be above 0")
    if args.anchored and args.anchored_min_score is None:
        parser.error("--anchored needs --anchored-min-score X: the scores of a flank that is there and of one that is not overlap on noisy reads, so there is no default")
    if args.anchored_min_score is not None and not args.anchored:
        parser.error("--anchored-min-score needs --anchored FILE")
    if args.anchored_min_score is not None and not args.anchored_min_score > 0:
        parser.error("--anchored-min-score must be above 0")
    if args.anchored_mod and not args.anchored:
        parser.error("--anchored-mod needs --anchored FILE --anchored-min-score X: the calls are made on the reads anchored counting finds")
    if args.renorm is not None and not 0 < args.renorm < 1:
        parser.error("--renorm MIN_SHARE must be inside (0, 1)")
    if args.renorm_out and args.renorm is None:
        parser.error("--renorm-out needs --renorm MIN_SHARE")
    # then what every output needs and excludes, in the order of OUTPUTS: said once, there
    for o in ALL_OUTPUTS:
        if getattr(args, _dest(o.flag)):
            if o.needs_mod and not args.mod_model:
                parser.error("%s needs --mod_model: %s" % (o.flag, o.needs_mod))
            if o.no_scan and args.scan:
                parser.error("%s cannot be combined with --scan: %s" % (o.flag, o.no_scan))
    log = Log(args.log_level)
    config = parse_config(args.repeat, args.config, log)
    alt_units = {}
    if args.alt_units:
        if not os.path.isfile(args.alt_units):
            log("Main: Alt-units file does not exist.", 'error'); raise SystemExit(1)
        try:
            with open(args.alt_units) as fp:
                alt_units = parse_alt_units(fp, {name: v[3] for name, v in config['repeat'].items()})
        except ValueError as e:
            log("Main: %s" % e, 'error'); raise SystemExit(1)
        if args.variants and not alt_units:
            log("Main: --variants: the alt-units file names no unit.", 'error'); raise SystemExit(1)
    tract_defs = {}
    if args.tract_units:
        if not os.path.isfile(args.tract_units):
            log("Main: Tract-units file does not exist.", 'error'); raise SystemExit(1)
        try:
            with open(args.tract_units) as fp:
                tract_defs = tracts_mod.parse_definitions(fp, set(config['repeat']))
        except ValueError as e:
            log("Main: %s" % e, 'error'); raise SystemExit(1)
        if not tract_defs:
            log("Main: --tracts: the tract-units file defines no target.", 'error'); raise SystemExit(1)
    motif_defs = {}
    if args.motif_units:
        if not os.path.isfile(args.motif_units):
            log("Main: Motif-units file does not exist.", 'error'); raise SystemExit(1)
        try:
            with open(args.motif_units) as fp:
                motif_defs = motifs_mod.parse_definitions(fp, {name: (v[3], None) for name, v in config['repeat'].items()})
        except ValueError as e:
            log("Main: %s" % e, 'error'); raise SystemExit(1)
        if not motif_defs:
            log("Main: --motifs: the motif-units file defines no target.", 'error'); raise SystemExit(1)
    for path, what in ((args.f5Index, "Fast5 index file"), (args.model, "Pore model file")):
        if not os.path.isfile(path):
            log("Main: %s does not exist." % what, 'error'); raise SystemExit(1)
    if args.mod_model and not os.path.isfile(args.mod_model):
        log("Main: Modification pore model file does not exist.", 'error'); raise SystemExit(1)
    from . import dist as sdist
    rank, world, local = sdist.env_rank_world()
    if world > 1:
        # one process per GPU (torchrun): the accepted (read, target) pairs are dealt to the ranks by read
        # length (strique_amd.dist.shard_indices), rank 0 gathers fixed-size result records plus the
        # modification strings once at the end (strique_amd.dist.gather_results) and writes the rows in input order
        if not args.algn and not args.scan:
            log("Main: --algn FILE is required when running on several GPUs (stdin cannot be shared).", 'error'); raise SystemExit(1)
        # this rank's share of the host's CPUs FIRST: sched_setaffinity pins the calling thread and what it creates afterwards, so the
        # threads torch.distributed / RCCL / gloo start in init_process_group -- and the reader, upload and statistics threads -- follow
        sdist.pin_rank_cpus()
        sdist.init_process_group(backend=args.backend)
    _tune_allocator()
    from .counter import repeatCounter
    device = args.device if (world == 1 or args.share_device) else local
    counter = repeatCounter(args.model, mod_model_file=args.mod_model, align_config=config['align'],
                            HMM_config=config['HMM'], device=device)
    loci = defaultdict(list)
    for name, (chrom, begin, end, repeat, prefix, suffix) in config['repeat'].items():
        try:
            counter.add_target(name, repeat, prefix, suffix, **({'alt_units': alt_units[name]} if name in alt_units else {}),
                               **({'tracts': tract_defs[name]} if name in tract_defs else {}),
                               **({'motifs': list(motif_defs[name])} if name in motif_defs else {}))
        except ValueError:
            raise
        except Exception as e:                # e.g. a flank longer than the compiled kernel shapes cover
            log("Main: target %s is not supported by the GPU engine (%s); its reads are skipped." % (name, e), 'error')
            continue
        loci[chrom].append((name, begin, end))
    f5 = Fast5Index(args.f5Index)
    scan = None
    if args.scan:
        scan = {"min_score": args.scan_min_score,
                "candidates": counter.candidates(), "scores": bool(args.scan_scores)}
        if not scan["candidates"]:
            log("Main: --scan without a usable target.", 'error'); raise SystemExit(1)
    # --scan: every read id of the index, in index order, instead of SAM records
    stream = list(f5.index) if args.scan else (open(args.algn) if args.algn else sys.stdin)
    readers = args.t
    if readers <= 0:
        # one process per GPU: every rank takes its share of the cores (LOCAL_WORLD_SIZE is set by torchrun) for its reader threads, at most
        # 24; the staging threads of the library and the engine thread run beside them
        local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        share = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        if share == (os.cpu_count() or 1):          # not pinned: an equal share by count
            share //= local_world
        quota = sdist.cpu_quota()                   # a container's CPU quota counts, not the CPUs it shows (16 of 256 on the MI355X boxes)
        if quota:
            share = min(share, max(1, int(quota) // local_world))
        readers = max(1, min(24, share))            # inflating is what the readers do: one per core they can get, 16 ... 24 measure the same end to end
    stats = {}
    fault = 0
    paths = {o.name: getattr(args, o.dest or _dest(o.flag)) for o in ALL_OUTPUTS}
    asked = {o.name: o.arg(args, alt_units) if o.arg else bool(paths[o.name]) for o in ALL_OUTPUTS if o.ask}
    with contextlib.ExitStack() as stack:
        # rank 0 writes: as the batches are done in a single process (run_count), after the gather otherwise
        files = {name: stack.enter_context(open(path, 'w')) if (path and rank == 0) else None for name, path in paths.items()}
        out = (stack.enter_context(open(args.out, 'w')) if args.out else sys.stdout) if rank == 0 else None
        now = {name: f if world == 1 else None for name, f in files.items()}
        try:
            rows = run_count(stream, loci, f5.get_raw, counter, log, args.batch, rank, world, out if world == 1 else None, readers=readers, stats=stats,
                             scan=scan, **asked, **{o.file: now[o.name] for o in ALL_OUTPUTS})
        except DeviceFault:
            if world == 1:
                raise SystemExit(3)
            fault = 1; rows = []
        if world > 1:
            import torch.distributed as dist
            # a rank that lost its device must not leave the others waiting in the gather: every rank learns about it
            # here (the faulty rank arrives at once, the others when their share is done) and all of them exit 3
            if sdist.any_rank(fault):
                if rank == 0:
                    log("Main: a rank reported a device error; no output written.", 'error')
                dist.destroy_process_group()
                raise SystemExit(3)
            merged = gather_rows(rows, stats["items"], sdist, scan=scan, **asked)
            if rank == 0:
                write_rows(out, merged.rows)
                for o in ALL_OUTPUTS:
                    if files[o.name] is not None:
                        write_rows(files[o.name], merged.riders[o.name] if o.name in merged.riders else getattr(merged, o.name), header=o.header(scan))
            dist.barrier()
            dist.destroy_process_group()
    if stats.get("failed"):
        # like the reference (STRique.py:704-713): reads that fail are logged, the run itself succeeds
        log("Main: %d read(s) could not be processed (see warnings above)." % stats["failed"], 'error')
        if args.strict:
            raise SystemExit(2)


def _tune_allocator():
    """The reader threads allocate one array per read (0.2 ... 8 MB).  glibc serves such sizes with a fresh mmap each time:
    every read then costs a map, a page fault per 4 KB while it is filled and an unmap, all under the process-wide mm lock,
    and the readers stop scaling beyond a few threads.  Raise the mmap threshold to its maximum (32 MB) and keep freed memory:
    the arrays come out of the per-thread arenas and their pages are reused."""
    try:
        import ctypes
        libc = ctypes.CDLL("libc.so.6")
        M_TRIM_THRESHOLD, M_MMAP_THRESHOLD = -1, -3
        libc.mallopt(M_MMAP_THRESHOLD, 32 << 20)
        libc.mallopt(M_TRIM_THRESHOLD, (1 << 31) - 1)
    except (OSError, AttributeError):
        pass


class DeviceFault(Exception):
    """The GPU engine reported a device error (fault, out of memory): it will not go away read by read."""


ROW_DTYPE = np.dtype([("count", np.int32), ("valid", np.int32), ("score_prefix", np.float64), ("score_suffix", np.float64),
                      ("log_p", np.float64), ("offset", np.int64), ("ticks", np.int64)])


def format_row(qname, target, strand, res):
    return '\t'.join(str(x) for x in (qname, target, strand) + tuple(res))


def format_units(qname, target, strand, n, positions):
    """One row of the `count --units` file: positions joined by commas, '-' when there are none (or no decode)."""
    pos = [] if positions is None else [int(x) for x in positions]
    return '\t'.join([str(qname), str(target), str(strand), str(n), str(len(pos)), ','.join(str(x) for x in pos) if pos else '-'])


def parse_units(stream):
    """Rows of a `count --units` file: [(ID, target, strand, count, [positions])] in file order."""
    out = []
    for line in stream:
        f = line.rstrip('\n').split('\t')
        if not line.strip() or f[0] == UNITS_HEADER[0]:
            continue
        pos = [] if f[5] == '-' else [int(x) for x in f[5].split(',')]
        if len(pos) != int(f[4]):
            raise ValueError("units row of %s: %s positions, n_units = %s" % (f[0], len(pos), f[4]))
        out.append((f[0], f[1], f[2], int(f[3]), pos))
    return out


def format_confidence(qname, target, strand, n, log_p, conf):
    """One row of the `count --confidence` file: count and log_p as the count row has them, then log_lik, count_mean, count_sd
    (str() of the floats, like the count TSV), '-' three times for a read that was not decoded."""
    tail = ['-', '-', '-'] if conf is None else [str(float(x)) for x in conf]
    return '\t'.join([str(qname), str(target), str(strand), str(n), str(log_p)] + tail)


def parse_confidence(stream):
    """Rows of a `count --confidence` file: [(ID, target, strand, count, log_p, (log_lik, count_mean, count_sd) or None)]."""
    out = []
    for line in stream:
        f = line.rstrip('\n').split('\t')
        if not line.strip() or f[0] == CONF_HEADER[0]:
            continue
        conf = None if f[5] == '-' else (float(f[5]), float(f[6]), float(f[7]))
        out.append((f[0], f[1], f[2], int(f[3]), float(f[4]), conf))
    return out


def format_mod_llr(qname, target, strand, n, mod, llr):
    """One row of the `count --mod-llr` file: count and pattern as the count row has them, the number of ratios, then the ratios
    with four decimals joined by commas (inf / -inf where one branch has no path), '-' when there are none."""
    vals = [] if llr is None else [float(x) for x in llr]
    return '\t'.join([str(qname), str(target), str(strand), str(n), str(mod), str(len(vals)), ','.join('%.4f' % x for x in vals) if vals else '-'])


def parse_mod_llr(stream):
    """Rows of a `count --mod-llr` file: [(ID, target, strand, count, mod_pattern, [ratios])] in file order."""
    out = []
    for line in stream:
        f = line.rstrip('\n').split('\t')
        if not line.strip() or f[0] == MODLLR_HEADER[0]:
            continue
        vals = [] if f[6] == '-' else [float(x) for x in f[6].split(',')]
        if len(vals) != int(f[5]):
            raise ValueError("mod-llr row of %s: %s ratios, n_units = %s" % (f[0], len(vals), f[5]))
        out.append((f[0], f[1], f[2], int(f[3]), f[4], vals))
    return out


def parse_alt_units(stream, repeats):
    """The `--alt-units` file: lines of target<TAB>unit[,unit...], `#` comments and blank lines skipped.  repeats: {target: repeat
    unit} of the repeat config.  Returns {target: [units]}, upper-cased; ValueError for an unknown target, a target given twice, more
    than 3 units, and whatever hmm.check_alt_units refuses (a unit of another length than the repeat unit, a unit given twice, ...)."""
    from .hmm import VARIANT_TAGS, check_alt_units
    out = {}
    for no, line in enumerate(stream, 1):
        text = line.split('#', 1)[0].strip()
        if not text:
            continue
        f = text.split('\t') if '\t' in text else text.split()
        if len(f) != 2:
            raise ValueError("alt units, line %d: expected target<TAB>unit[,unit...]" % no)
        name, units = f[0], [u.strip().upper() for u in f[1].split(',') if u.strip()]
        if name not in repeats:
            raise ValueError("alt units, line %d: unknown target %s" % (no, name))
        if name in out:
            raise ValueError("alt units, line %d: target %s is given twice" % (no, name))
        if len(units) > len(VARIANT_TAGS):
            raise ValueError("alt units, line %d: %d units for target %s, at most %d" % (no, len(units), name, len(VARIANT_TAGS)))
        try:
            out[name] = check_alt_units(repeats[name], units)
        except ValueError as e:
            raise ValueError("alt units, line %d: %s" % (no, e))
    return out


def variant_value(raw, units):
    """What the variants file says of one read, from the counter's (count_v, pattern, branch, end, V) and the alt units of its target as
    configured: (count_v, n_passages, pattern, [(index, unit, sample, llr)]) -- one call per alt passage: the index of its alt character in
    the pattern, the raw sample of the hub emission behind it, llr = max over the alt branches of V_b, less V_0.  None stays None."""
    if raw is None:
        return None
    count_v, pattern, branch, end, V = raw
    n_alt = int(np.count_nonzero(branch))
    m = (len(pattern) - len(branch)) // n_alt if n_alt else 0          # an alt passage is '0' * m + str(b): m characters more than a base one
    calls, at = [], 0
    for j, b in enumerate(branch):
        if b:
            at += m
            calls.append((at, units[int(b) - 1], int(end[j]), float(np.max(V[j, 1:]) - V[j, 0])))
        at += 1
    return int(count_v), len(branch), pattern, calls


def format_variants(qname, target, strand, n, v):
    """One row of the `count --variants` file: the count as the count row has it, then count_v, the passages, the alt calls, the pattern
    and the calls as index:unit:sample:llr (llr with four decimals) joined by commas; '-' for a field without value."""
    if v is None:
        return '\t'.join([str(qname), str(target), str(strand), str(n), '-', '-', '-', '-', '-'])
    count_v, n_pass, pattern, calls = v
    return '\t'.join([str(qname), str(target), str(strand), str(n), str(count_v), str(n_pass), str(len(calls)), pattern if pattern else '-',
                      ','.join('%d:%s:%d:%.4f' % c for c in calls) if calls else '-'])


def parse_variants(stream):
    """Rows of a `count --variants` file: [(ID, target, strand, count, count_v, n_passages, pattern, [(index, unit, sample, llr)])] in file
    order; count_v, n_passages and pattern None for a read without a decode."""
    out = []
    for line in stream:
        f = line.rstrip('\n').split('\t')
        if not line.strip() or f[0] == VARIANTS_HEADER[0]:
            continue
        if f[4] == '-':
            out.append((f[0], f[1], f[2], int(f[3]), None, None, None, []))
            continue
        calls = []
        if f[8] != '-':
            for c in f[8].split(','):
                i, unit, sample, llr = c.split(':')
                calls.append((int(i), unit, int(sample), float(llr)))
        if len(calls) != int(f[6]):
            raise ValueError("variants row of %s: %s calls, n_alt = %s" % (f[0], len(calls), f[6]))
        out.append((f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]), '' if f[7] == '-' else f[7], calls))
    return out


def _pack_variants(v):
    """(count_v, n_passages, pattern, calls) as it travels between ranks: the ratios as repr(), which float() reads back bit for bit."""
    count_v, n_pass, pattern, calls = v
    return '|'.join([str(int(count_v)), str(int(n_pass)), pattern, ','.join('%d:%s:%d:%s' % (i, u, s, repr(float(x))) for i, u, s, x in calls)])


def _unpack_variants(text):
    count_v, n_pass, pattern, calls = text.split('|')
    out = []
    for c in calls.split(',') if calls else []:
        i, u, s, x = c.split(':')
        out.append((int(i), u, int(s), float(x)))
    return int(count_v), int(n_pass), pattern, out


def _floats(values):
    """Floats as they travel between ranks: repr(), which float() reads back bit for bit."""
    return ','.join(repr(float(x)) for x in values)


def _unfloats(text):
    return [float(x) for x in text.split(',')]


# The optional per-read outputs of `count`, in the order of the fields of `Merged` and of the gather blob.  name: the keyword of
# run_count / counter.detect_batch and the field of `Merged`; header(scan): the header of its file; format(qname, target, strand, row,
# value): one row of its file (row: the count row's tuple, None for a scan read without a winner -- only an output with rowless=True
# writes one then); pack(value) / unpack(text): its field of the gather blob (absent values are '-' and never reach them); stat: the
# key of run_count's `stats` that collects its rows; file: run_count's keyword of its file.
# ask: how run_count asks the counter for it -- 'keyword': detect_batch(..., name=True); 'switch': counter.set_<name>(True) for the run,
# set_<name>(False) behind it, and detect_batch(..., records=True); with `level` run_count's own value travels instead of True (as a
# keyword with records=True, as a switch with None behind the run); None: the scan gives it, not the counter.
# value(det, target, counter, asked): its value from a Detected record (asked: run_count's {name: value}).
# refuse(asked, scan): the text of run_count's ValueError for what was asked, or None.
# For count(): flag, its argument -- what the errors name, and the attribute that tells whether it was asked for; dest: the attribute
# of its file where that is another one; arg(args, alt_units): what run_count is given for it (default: whether the file was named);
# needs_mod / no_scan: why "<flag> needs --mod_model" / "<flag> cannot be combined with --scan" (None: it does not / it can).
# rides (RIDERS below): (the output whose value it formats, the keyword of that output's switch that makes the value carry it).
Output = namedtuple('Output', ['name', 'header', 'format', 'pack', 'unpack', 'stat', 'rowless', 'file', 'ask', 'value', 'flag',
                               'level', 'refuse', 'dest', 'arg', 'needs_mod', 'no_scan', 'rides'], defaults=(False, None, None, None, None, None, None))
_ALIGNED = "the %s pass runs on reads whose target and strand an alignment gives"
_BOTH_FLANKS = "a scan takes a read for a target when it finds both flanks"


def _asked(o, value):
    """Whether run_count's value for output `o` asks for it: by truth, but for an output whose value says more than yes (the ones with
    `arg`: a threshold, the alt units) -- such a one is on unless None, as an empty {target: alt units} is."""
    return value is not None if o.arg else bool(value)


def _dest(flag):
    return flag[2:].replace('-', '_')


def _not_with_scan(text):
    return lambda asked, scan: text if scan else None


OUTPUTS = (
    Output('units', lambda scan: UNITS_HEADER, lambda q, t, s, row, v: format_units(q, t, s, row[0], v),
           lambda v: ','.join(str(int(x)) for x in v), lambda text: [int(x) for x in text.split(',')], 'unit_rows', False,
           file='units_out', ask='keyword', flag='--units', value=lambda d, t, c, a: d.units),
    Output('confidence', lambda scan: CONF_HEADER, lambda q, t, s, row, v: format_confidence(q, t, s, row[0], row[3], v),
           _floats, _unfloats, 'conf_rows', False,
           file='conf_out', ask='keyword', flag='--confidence', value=lambda d, t, c, a: d.conf, no_scan=_ALIGNED % "forward"),
    Output('mod_llr', lambda scan: MODLLR_HEADER, lambda q, t, s, row, v: format_mod_llr(q, t, s, row[0], row[6], v),
           _floats, _unfloats, 'llr_rows', False,
           file='llr_out', ask='keyword', flag='--mod-llr', value=lambda d, t, c, a: d.llr,
           needs_mod="the ratios belong to the calls of the modification model", no_scan=_ALIGNED % "scoring"),
    Output('scores', lambda scan: scan_mod.scores_header(scan["candidates"]),
           lambda q, t, s, row, v: scan_mod.format_scores(q, None if row is None else (t, s), v),
           lambda v: _floats(x for pair in v for x in pair), lambda text: list(zip(*[iter(_unfloats(text))] * 2)), 'score_rows', True,
           file='scores_out', ask=None, flag='--scan-scores', value=None),
    Output('renorm', lambda scan: renorm_mod.HEADER, lambda q, t, s, row, v: renorm_mod.format_row(q, t, s, v),
           lambda v: renorm_mod.pack(v), lambda text: renorm_mod.unpack(text), 'renorm_rows', False,
           file='renorm_out', ask='switch', level=True, flag='--renorm',
           value=lambda d, t, c, a: d.renorm and renorm_mod.report(d.renorm, c.renorm_bin_width),
           refuse=lambda asked, scan: ("renorm cannot be combined with a scan" if scan else
                                       None if 0 < asked['renorm'] < 1 else "the renorm share threshold must be inside (0, 1)"),
           dest='renorm_out', arg=lambda args, alt_units: args.renorm,
           no_scan="the fit needs the target of a read, which a scan finds with the maps as they are"),
    Output('variants', lambda scan: VARIANTS_HEADER, lambda q, t, s, row, v: format_variants(q, t, s, row[0], v),
           lambda v: _pack_variants(v), lambda text: _unpack_variants(text), 'variant_rows', False,
           file='variants_out', ask='switch', flag='--variants',
           value=lambda d, t, c, a: variant_value(d.variants, (a.get('variants') or {}).get(t, ())),
           refuse=_not_with_scan("variants cannot be combined with a scan"),
           arg=lambda args, alt_units: alt_units if args.variants else None, no_scan=_ALIGNED % "variant"),
    Output('flank_mod', lambda scan: flank_mod_rule.HEADER, lambda q, t, s, row, v: flank_mod_rule.format_row(q, t, s, row[0], v),
           lambda v: _pack_flank_mod(v), lambda text: _unpack_flank_mod(text), 'flank_mod_rows', False,
           file='flank_mod_out', ask='switch', flag='--flank-mod',
           value=lambda d, t, c, a: flank_mod_value(d.flank_mod),
           refuse=_not_with_scan("flank methylation calls cannot be combined with a scan"),
           needs_mod="the calls compare the modification model's k-mer table with the base table", no_scan=_ALIGNED % "flank"),
    Output('tracts', lambda scan: tracts_mod.HEADER, lambda q, t, s, row, v: tracts_mod.format_row(q, t, s, row[0], v and v[:2]),
           lambda v: _pack_tracts(v), lambda text: _unpack_tracts(text), 'tract_rows', False,
           file='tracts_out', ask='switch', flag='--tracts', value=lambda d, t, c, a: d.tracts,
           refuse=_not_with_scan("tracts cannot be combined with a scan"), no_scan=_ALIGNED % "tract"),
    Output('anchored_mod', lambda scan: anchored_mod.MOD_HEADER, lambda q, t, s, row, v: anchored_mod.format_mod_row(q, t, s, *(v or (None, None))),
           lambda v: _pack_anchored_mod(v), lambda text: _unpack_anchored_mod(text), 'anchored_mod_rows', False,
           file='anchored_mod_out', ask='switch', flag='--anchored-mod', value=lambda d, t, c, a: (d.anchored, d.anchored_mod),
           refuse=lambda asked, scan: None if asked.get('anchored') is not None else "anchored methylation calls need anchored counting",
           needs_mod="the calls are those of the modification model", no_scan=_BOTH_FLANKS),
    Output('anchored', lambda scan: anchored_mod.HEADER, lambda q, t, s, row, v: anchored_mod.format_row(q, t, s, v),
           lambda v: _pack_anchored(v), lambda text: _unpack_anchored(text), 'anchored_rows', False,
           file='anchored_out', ask='keyword', level=True, flag='--anchored', value=lambda d, t, c, a: d.anchored,
           refuse=_not_with_scan("anchored counting cannot be combined with a scan"),
           arg=lambda args, alt_units: args.anchored_min_score, no_scan=_BOTH_FLANKS),
)
# Outputs that ride on another output: a file, a flag, a keyword of run_count and a stat of their own, but no pass of the counter, no
# field of Detected, of `Merged` or of the gather blob -- the value is the one of the output they ride on (with the keyword on, that
# value carries what they write; it travels between ranks in that output's field), asked for as run_count(..., <name>=True).
RIDERS = (
    Output('tract_positions', lambda scan: tracts_mod.POS_HEADER, lambda q, t, s, row, v: tracts_mod.format_positions_row(q, t, s, row[0], v),
           None, None, 'tract_position_rows', False,
           file='tract_positions_out', ask='rider', flag='--tract-positions', value=None,
           refuse=lambda asked, scan: ("tract positions cannot be combined with a scan" if scan else
                                       None if asked.get('tracts') else "tract positions need the tract counts"),
           no_scan=_ALIGNED % "tract", rides=('tracts', 'positions')),
)

def motifs_value(rec, units):
    """The value of the motifs output from a record of repeatCounter.motif_records and the target's candidates: None or a motifs.Row."""
    if rec is None:
        return None
    majority, shares, count_m, log_p_m, runs, winners, _ = rec
    return motifs_mod.Row(tuple(units), len(winners), majority, tuple(shares), count_m, log_p_m, [tuple(r) for r in runs])


def _pack_motifs(v):
    """A motifs.Row as it travels between ranks: units | segments | majority | shares | count_m | log_p_m | runs, floats as repr()."""
    return '|'.join([','.join(v.units), str(int(v.n_segments)), str(int(v.majority)), ','.join(repr(float(x)) for x in v.shares),
                     '-' if v.count_m is None else str(int(v.count_m)), '-' if v.log_p_m is None else repr(float(v.log_p_m)),
                     ','.join('%d:%d:%d' % tuple(r) for r in v.runs)])


def _unpack_motifs(text):
    f = text.split('|')
    return motifs_mod.Row(tuple(f[0].split(',')), int(f[1]), int(f[2]), tuple(float(x) for x in f[3].split(',')), None if f[4] == '-' else int(f[4]),
                          None if f[5] == '-' else float(f[5]), [tuple(int(x) for x in r.split(':')) for r in f[6].split(',')])


# Outputs beside the passes of the counter: a file, a flag, a keyword of run_count and a stat of their own, and a field of their own at
# the end of the gather blob when they are on -- but no row of counter.PASSES and no field of Detected or `Merged`: the counter keeps
# their values beside the records of its last call (ask 'side': set_<name>(True, value) before the run, set_<name>(False) behind it;
# side(counter, target, k): the value of read k of that call).  They travel between ranks like the RIDERS' rows, in Merged.riders.
SIDE_RECORDS = {'motifs': 'motif_records'}          # where the counter keeps the values of its last call
SIDES = (
    Output('motifs', lambda scan: motifs_mod.HEADER, lambda q, t, s, row, v: motifs_mod.format_row(q, t, s, row[0], v),
           _pack_motifs, _unpack_motifs, 'motif_rows', False,
           file='motifs_out', ask='side', flag='--motifs', value=None,
           refuse=_not_with_scan("motifs cannot be combined with a scan"),
           arg=lambda args, alt_units: (args.motif_segment or motifs_mod.SEGMENT) if args.motifs else None,
           no_scan="the track scores the stretch between the two flanks of the target an alignment gives"),
)
ALL_OUTPUTS = OUTPUTS + RIDERS + SIDES
# (`renorm`, `variants`, `flank_mod`, `tracts`, `anchored_mod` and `anchored`, the last fields, default to None: callers that build a Merged from the five
# values before them keep working.  `anchored` stays the last field, as it did when `variants`, `anchored_mod` and `tracts` came in: fields
# behind the first five are taken by name.)
class Merged(namedtuple('Merged', ['rows'] + [o.name for o in OUTPUTS], defaults=(None, None, None, None, None, None))):
    riders = {}          # gather_rows: {name: rows} of the RIDERS that were on (no field: the fields are those of OUTPUTS)


def flank_mod_value(calls):
    """The value of the flank_mod output from Detected.flank_mod: None, or [(flank, pos, n_sites, llr or None)] -- a group that was not
    scored has no ratio."""
    if calls is None:
        return None
    return [(int(f), int(pos), int(ns), float(llr) if status == flank_mod_rule.SCORED else None) for f, pos, ns, _, status, _, _, llr in calls]


def _pack_flank_mod(v):
    """The calls of a read as they travel between ranks: flank:pos:n_sites:ratio per group, the ratio as repr(), '-' for none."""
    return ','.join('%d:%d:%d:%s' % (f, pos, ns, '-' if llr is None else repr(float(llr))) for f, pos, ns, llr in v)


def _unpack_flank_mod(text):
    out = []
    for item in text.split(','):
        f, pos, ns, llr = item.split(':')
        out.append((int(f), int(pos), int(ns), None if llr == '-' else float(llr)))
    return out


def _pack_tracts(v):
    """(counts, log_p[, positions]) of a read as it travels between ranks: the log-probability as repr(), which float() reads back bit
    for bit; with positions a third part -- 'x' for None, else the tracts joined by '|', a tract's positions by commas, '-' for none."""
    text = ','.join(str(int(c)) for c in v[0]) + ';' + repr(float(v[1]))
    if len(v) == 3:
        text += ';' + ('x' if v[2] is None else '|'.join(','.join(str(int(x)) for x in p) if len(p) else '-' for p in v[2]))
    return text


def _unpack_tracts(text):
    f = text.split(';')
    rec = (tuple(int(c) for c in f[0].split(',')), float(f[1]))
    if len(f) == 3:
        rec += (None if f[2] == 'x' else tuple(np.array([] if p == '-' else [int(x) for x in p.split(',')], np.int64) for p in f[2].split('|')),)
    return rec


def _pack_anchored_mod(v):
    """(anchored record or None, methylation call or None) of a read as it travels between ranks: the record as _pack_anchored
    packs it, then the pattern and the ratios ('-' for None each); call (pattern, ratios or None)."""
    rec, call = v
    fields = ['-' if rec is None else _pack_anchored(rec)]
    if call is not None:
        fields += ['+' + call[0], '-' if call[1] is None or len(call[1]) == 0 else _floats(call[1])]
    return ';'.join(fields)


def _unpack_anchored_mod(text):
    f = text.split(';')
    rec = None if f[0] == '-' else _unpack_anchored(f[0])
    return (rec, None) if len(f) == 1 else (rec, (f[1][1:], None if f[2] == '-' else _unfloats(f[2])))


def _pack_anchored(rec):
    """The anchored record of a read (kind, status, count, log_p, begin, end, free_samples) as it travels between ranks."""
    kind, status, count, log_p, begin, end, free = rec
    return ','.join([str(int(kind)), str(int(status)), str(int(count)), repr(float(log_p)), str(int(begin)), str(int(end)), str(int(free))])


def _unpack_anchored(text):
    f = text.split(',')
    return (int(f[0]), int(f[1]), int(f[2]), float(f[3]), int(f[4]), int(f[5]), int(f[6]))


def outputs_on(**flags):
    """The entries of OUTPUTS whose flag (its name as a keyword) is set."""
    unknown = set(flags) - set(Merged._fields[1:]) - {o.name for o in RIDERS + SIDES}
    if unknown:
        raise TypeError("no such output: %s" % ", ".join(sorted(unknown)))
    return [o for o in ALL_OUTPUTS if flags.get(o.name)]


def as_detected(res, units=False, confidence=False, mod_llr=False):
    """One result of counter.detect_batch(..., units, confidence, mod_llr) as a Detected record: a record as it is (what run_count
    asks for with anchored counting on: the anchored record of every read travels in it), else the legacy shape detect_batch
    documents -- (row[, positions][, conf][, llr]), without any of the three the bare row."""
    if isinstance(res, Detected):
        return res
    if not (units or confidence or mod_llr):
        return Detected(res, None, None, None)
    rest = iter(res[1:])
    return Detected(res[0], *[next(rest) if asked else None for asked in (units, confidence, mod_llr)])


def _read_values(target, strand, det, scores=None, counter=None, asked=None):
    """What the writers know of one read: (target, strand, row or None, {output name: value or None}); counter and asked (run_count's
    {name: value}): what the value functions of OUTPUTS take -- run_count hands over both for every read; without them a record
    gives the values that need neither."""
    if det is None:
        return target, strand, None, dict(scores=scores)
    return target, strand, det.row, dict({o.name: o.value(det, target, counter, asked or {}) for o in OUTPUTS if o.value}, scores=scores)


def _emit(sink, on, seq, qname, target, strand, row, values):
    """The rows of one read, (seq, text) each: its count row to sink['rows'], the row of every output of `on` to sink[name]."""
    for o in on:
        if row is not None or o.rowless:
            sink[o.name].append((seq, o.format(qname, target, strand, row, values.get(o.rides[0] if o.rides else o.name))))
    if row is not None:
        sink['rows'].append((seq, format_row(qname, target, strand, row)))


def _absent(v):
    return v is None or (not isinstance(v, str) and len(v) == 0)


def pack_blob(on, target, strand, mod, values):
    """What travels beside the fixed-size record of a read: target, strand, modification pattern, then one field per entry of
    OUTPUTS, tab-separated; '-' for the target and strand of a scan read without a winner (its record says so: valid = 2), for an
    output that is not in `on` and for a value that is None or empty."""
    fields = ['-' if target is None else target, '-' if strand is None else strand, mod]
    for o in OUTPUTS:
        v = values.get(o.name) if o in on else None
        fields.append('-' if _absent(v) else o.pack(v))
    for o in SIDES:          # (a field of their own, only when they are on)
        if o in on:
            v = values.get(o.name)
            fields.append('-' if v is None else o.pack(v))
    return '\t'.join(fields)


def unpack_blob(on, blob):
    """(target, strand, mod, values) of pack_blob(on, ...): target and strand as they travelled, None for every '-' value."""
    fields = blob.split('\t')
    values = {o.name: None if (o not in on or f == '-') else o.unpack(f) for o, f in zip(OUTPUTS, fields[3:])}
    for o, f in zip([o for o in SIDES if o in on], fields[3 + len(OUTPUTS):]):
        values[o.name] = None if f == '-' else o.unpack(f)
    return fields[0], fields[1], fields[2], values


def gather_rows(rows, items, sdist, units=False, scan=None, **flags):
    """Reads of this rank (run_count with world > 1) -> fixed-size records + one blob per read (pack_blob) -> one gather -> on rank 0
    the rows of every file in input order: Merged(rows, one field per entry of OUTPUTS), [(sequence number, TSV row)] each, None for
    an output whose flag (its name, given as a keyword like units= and scan=; outputs_on raises TypeError for a name that is no output)
    was not set (scores: asked for by scan) and for every field off rank 0.  `items`: every accepted (qname,
    strand, target) of the input, which each rank derives from the same SAM file (scan: from the same index).  A read that failed
    travels as a record with valid = 0 and writes nothing; a scan read without a winner as one with valid = 2: it writes a score row."""
    on = outputs_on(units=units, scores=bool(scan), **flags)
    rec = np.zeros(len(rows), ROW_DTYPE); blobs = []; idx = np.zeros(len(rows), np.int64)
    for k, (seq, read) in enumerate(rows):
        idx[k] = seq
        if read is None:
            blobs.append("")
            continue
        target, strand, row, values = read
        if row is None:
            rec[k]["valid"] = 2
        else:
            n, sp, ss, p, offset, ticks, mod = row
            rec[k] = (n, 1, sp, ss, float(p), offset, ticks)
        blobs.append(pack_blob(on, target, strand, '-' if row is None else mod, values))
    full, full_blobs = sdist.gather_results(rec, idx, len(items), blobs)
    if full is None:
        return Merged(*[None] * len(Merged._fields))
    sink = defaultdict(list)
    for seq, (qname, _, _) in enumerate(items):
        r = full[seq]
        if not r["valid"]:
            continue
        target, strand, mod, values = unpack_blob(on, full_blobs[seq])
        row = None
        if r["valid"] != 2:
            n = int(r["count"]); lp = float(r["log_p"])
            p = lp if (n or lp != 0) else 0              # the reference prints the integer 0 for a failed gate (STRique.py:602,616)
            row = (n, float(r["score_prefix"]), float(r["score_suffix"]), p, int(r["offset"]), int(r["ticks"]), mod)
        _emit(sink, on, seq, qname, target, strand, row, values)
    merged = Merged(sink['rows'], *[sink[o.name] if o in on else None for o in OUTPUTS])
    merged.riders = {o.name: sink[o.name] for o in RIDERS + SIDES if o in on}
    return merged


def write_rows(out, rows, header=True):
    """header: True = the count header, a list = that header, False = none."""
    if header:
        print('\t'.join(HEADER if header is True else header), file=out)
    for _, row in rows:
        print(row, file=out)
    out.flush()


def route(stream, loci, log):
    """Accepted SAM records of `stream`: (qname, strand, [targets], read length)."""
    for line in stream:
        if line.startswith('@'):
            continue
        sr = decode_sam(line)
        if not sr.QNAME:
            log("Detector: Error parsing alignment \n%s" % line, 'error'); continue
        targets = intersect_targets(sr, loci)
        if not targets:
            log("Detector: No target for %s" % sr.QNAME, 'debug'); continue
        yield sr.QNAME, ('+' if sr.FLAG & 0x10 == 0 else '-'), targets, sr.QLEN


def run_count(stream, loci, get_raw, counter, log, batch_size, rank=0, world=1, out=None, readers=0, stats=None, scan=None, **asked):
    """Route the SAM records of `stream` to their targets, run this rank's share through
    `counter.detect_batch` and return [(sequence number, TSV row or -- several ranks -- what gather_rows takes)].

    Single process: rows [(seq, TSV row)] are also written to `out` as soon as their batch is done.
    Several ranks: the records are read first (the SAM carries the read lengths), the accepted
    (read, target) pairs are dealt to the ranks by descending read length
    (strique_amd.dist.shard_indices: the DP cost of a read is proportional to its length), and the
    return value goes to `gather_rows`.
    `readers` > 0: raw signals are fetched by that many threads ahead of the GPU batches (inflating
    the deflate chunks of a fast5 releases the GIL and is what bounds a `count` run on real files);
    the order of the rows does not change.
    Further keywords: the optional outputs of OUTPUTS, each by its name and by the keyword of its file (units=True, units_out=FILE;
    confidence, conf_out; mod_llr, llr_out; anchored=score threshold, anchored_out; anchored_mod, anchored_mod_out; variants={target:
    [alt units as configured]}, variants_out; renorm=share threshold, renorm_out; tracts, tracts_out; tract_positions (with tracts), tract_positions_out; flank_mod, flank_mod_out; the
    score rows of a scan: scores_out); any other keyword is a TypeError.  OUTPUTS says how the counter is asked for each of them, which
    of them a scan excludes (ValueError) and how the value of a read is taken from its result, which is normalised to a Detected record
    (as_detected).  Single process: the rows of an output go to its file with the count rows; they are collected in stats[its `stat`
    key] either way.  A switch of the counter that an output turns on belongs to this run: it is off again when the run is through.
    The count rows and the other files do not depend on what else is asked for, but with renorm: the rows of the reads it applies to change.
    `scan` ({"min_score", "candidates", "scores"}): `stream` is a list of read ids instead of a SAM stream; every read goes through
    counter.scan_batch and takes target and strand from its winner -- a read without one writes no row, as a read without a target
    writes none; single process: the score rows (strique_amd.scan.format_scores, every read) go to `scores_out` and to
    stats["score_rows"]; several ranks: the reads are dealt out by position (no SAM, no lengths).
    Several ranks: every result is (seq, (target, strand, row or None, values) or None) for `gather_rows` -- see _read_values."""
    from .ffi import StriqueHipError, STRQ_ERR_ARG, STRQ_ERR_UNSUPPORTED
    if stats is None:
        stats = {}
    stats.setdefault("failed", 0)
    files = dict({o.name: asked.pop(o.file, None) for o in ALL_OUTPUTS}, rows=out)
    unknown = set(asked) - {o.name for o in ALL_OUTPUTS if o.ask}
    if unknown:
        raise TypeError("run_count() got an unexpected keyword argument '%s'" % sorted(unknown)[0])
    asked['scores'] = bool(scan and scan["scores"])
    on = [o for o in ALL_OUTPUTS if _asked(o, asked.get(o.name))]
    riding = {o.rides[0]: {o.rides[1]: True} for o in on if o.rides}
    for o in on:
        refused = o.refuse and o.refuse(asked, scan)
        if refused:
            raise ValueError(refused)
    if out is not None:
        print('\t'.join(HEADER), file=out)
    for o in ALL_OUTPUTS:
        stats.setdefault(o.stat, [])
        if files[o.name] is not None:
            print('\t'.join(o.header(scan)), file=files[o.name])
    legacy = {name: bool(asked.get(name)) for name in ('units', 'confidence', 'mod_llr')}          # the shapes as_detected takes apart
    extras = {}
    for o in on:
        if o.ask == 'switch':
            getattr(counter, 'set_' + o.name)(asked[o.name] if o.level else True, **riding.get(o.name, {}))
        elif o.ask == 'keyword':
            extras[o.name] = asked[o.name] if o.level else True
        elif o.ask == 'side':
            getattr(counter, 'set_' + o.name)(True, asked[o.name])
        if o.ask == 'switch' or o.level:
            extras['records'] = True
    sides = [o for o in on if o.ask == 'side']
    rows = []
    records = ((rid, '.', ['.'], 0) for rid in stream) if scan else route(stream, loci, log)
    mine_set = None
    if world > 1:
        from . import dist as sdist
        records = list(records)
        items, cost = [], []
        for qname, strand, targets, qlen in records:
            for t in targets:
                items.append((qname, strand, t)); cost.append(qlen)
        mine_set = set(int(i) for i in sdist.shard_indices(len(items), rank, world, cost))
        stats["items"] = items

    import threading
    faulted = threading.Event()

    def run_batch(batch):
        """Engine thread: one batch through the GPU pipeline (the library releases the GIL for the whole call), its rows
        formatted; returns (rows, number of failed reads)."""
        failed = 0
        results = None
        side_values = {}
        if faulted.is_set():                                      # queued behind the batch that faulted: the device is not touched again
            raise DeviceFault("not run: the device failed in an earlier batch")
        def scan_some(raws):
            got, sc = counter.scan_batch(raws, min_score=scan["min_score"], units=legacy['units'], scores=True)
            return [(g, [tuple(x) for x in s]) for g, s in zip(got, sc)]
        try:
            if scan:
                results = scan_some([raw for _, _, _, _, raw in batch])
            else:
                results = counter.detect_batch([(t, raw, s) for _, _, t, s, raw in batch], **extras)
                side_values = {o.name: list(getattr(counter, SIDE_RECORDS[o.name])) for o in sides}
        except StriqueHipError as e:
            if e.code not in (STRQ_ERR_ARG, STRQ_ERR_UNSUPPORTED):
                # a device fault or an out-of-memory condition will not go away read by read
                faulted.set()
                log("Detector: device error, giving up: %s" % e, 'error')
                raise DeviceFault(str(e))
            log("Detector: batch rejected (%s), retrying read by read" % e, 'warning')
        except Exception as e:                                    # a bad batch never kills the run
            log("Detector: batch failed (%s), retrying read by read" % e, 'warning')
        if results is None:
            results = []
            for _, _, t, s, raw in batch:
                try:
                    results.append(scan_some([raw])[0] if scan else counter.detect(t, raw, s, **extras))
                    for o in sides:
                        side_values.setdefault(o.name, []).append(getattr(counter, SIDE_RECORDS[o.name])[0])
                except StriqueHipError as e1:
                    if e1.code not in (STRQ_ERR_ARG, STRQ_ERR_UNSUPPORTED):
                        faulted.set()
                        log("Detector: device error, giving up: %s" % e1, 'error')
                        raise DeviceFault(str(e1))
                    log("Detector: read failed: %s" % e1, 'warning'); results.append(None); failed += 1
                except Exception as e1:
                    log("Detector: read failed: %s" % e1, 'warning'); results.append(None); failed += 1
                for o in sides:          # (a read that failed has no value)
                    side_values.setdefault(o.name, [])
                    if len(side_values[o.name]) < len(results):
                        side_values[o.name].append(None)
        sink = defaultdict(list)
        for k, ((seq, qname, target, strand, _), res) in enumerate(zip(batch, results)):
            read = None
            if res is not None and scan:
                winner, sc = res
                read = _read_values(None, None, None, sc) if winner is None else _read_values(winner[0], winner[1], as_detected(winner[2], legacy['units']), sc, counter, asked)
            elif res is not None:
                read = _read_values(target, strand, as_detected(res, **legacy), None, counter, asked)
                for o in sides:
                    read[3][o.name] = motifs_value(side_values[o.name][k], counter.motif_units.get(target, ()))
            if world > 1:
                sink['rows'].append((seq, read))
            elif read is not None:
                _emit(sink, on, seq, qname, *read)
        return sink, failed

    # The batches run on an engine thread, one at a time and in order, while this thread routes the next SAM records and
    # collects their signals: the GPU call of batch k overlaps the host-side preparation of batch k + 1 (at 50 kb per read
    # that preparation -- SAM decode, index look-ups, waiting for the reader threads -- costs about as much as the call).
    from concurrent.futures import ThreadPoolExecutor
    engine = ThreadPoolExecutor(max_workers=1)
    in_flight = deque()

    def collect(keep):
        while len(in_flight) > keep:
            sink, failed = in_flight.popleft().result()          # re-raises DeviceFault from the engine thread
            stats["failed"] += failed
            rows.extend(sink['rows'])
            for o in ALL_OUTPUTS:
                stats[o.stat].extend(sink[o.name])
            for name, f in files.items():
                if f is not None:
                    write_rows(f, sink[name], header=False)

    def flush(batch):
        if not batch:
            return
        collect(1)                                               # at most one batch running and one waiting
        in_flight.append(engine.submit(run_batch, batch))

    import inspect
    try:
        takes_alloc = "alloc" in inspect.signature(get_raw).parameters
    except (TypeError, ValueError):
        takes_alloc = False

    def fetch(qname, alloc=None, defer=False):
        try:
            return get_raw(qname, alloc, defer) if takes_alloc else get_raw(qname)
        except NotImplementedError as e:          # a storage layout / filter the HDF5 subset reader does not cover
            log("Detector: cannot read %s: %s" % (qname, e), 'error'); stats["failed"] += 1
            return None
        except Exception as e:
            log("Detector: cannot read %s: %s" % (qname, e), 'warning')
            return None

    pool = None
    if readers > 1:
        pool = ThreadPoolExecutor(max_workers=readers)
    CHUNK = 32                             # reads per reader task: one future per read costs more Python time than a contiguous read does
    pending = deque()                      # (future or list of raw signals, [(qname, strand, [(seq, target)])]), in input order
    group = []
    batch = []

    def fetch_many(qnames):
        alloc = None          # (huge-page slabs shared by the reads of a task measured no gain over one inflate call per task: profiles/r04_reader.md -- removed)
        if not takes_alloc or os.environ.get("STRQ_READ_ONE_BY_ONE"):
            return [fetch(q, alloc) for q in qnames]
        # compressed datasets: located first (Python, under the interpreter lock), then inflated together in one native call
        from .fast5 import InflatePlan, inflate_plans
        got = [fetch(q, alloc, True) for q in qnames]
        plans = [(i, g) for i, g in enumerate(got) if isinstance(g, InflatePlan)]
        if plans:
            try:
                errors = inflate_plans([p for _, p in plans])
            except Exception as e:
                errors = [str(e)] * len(plans)
            for (i, p), err in zip(plans, errors):
                if err is None:
                    got[i] = p.out
                else:
                    log("Detector: cannot read %s: %s" % (qnames[i], err), 'warning'); got[i] = None
        return got

    def push_group():
        nonlocal group
        if group:
            names = [g[0] for g in group]
            pending.append((pool.submit(fetch_many, names) if pool is not None else fetch_many(names), group))
            group = []

    def drain(keep):
        nonlocal batch
        while len(pending) > keep:
            raws, grp = pending.popleft()
            if pool is not None:
                raws = raws.result()
            for (qname, strand, mine), raw in zip(grp, raws):
                if raw is None:
                    log("Detector: No fast5 for ID %s" % qname, 'warning'); continue
                for sq, t in mine:
                    batch.append((sq, qname, t, strand, raw))
                if len(batch) >= batch_size:
                    flush(batch); batch = []

    seq = 0
    lookahead = max(1, 2 * batch_size // CHUNK) if pool is not None else 0
    finished = False
    try:
        for qname, strand, targets, _qlen in records:
            mine = [(seq + i, t) for i, t in enumerate(targets) if mine_set is None or (seq + i) in mine_set]
            seq += len(targets)
            if not mine:
                continue
            group.append((qname, strand, mine))
            if len(group) >= CHUNK:
                push_group()
                drain(lookahead)
        push_group()
        drain(0)
        flush(batch)
        collect(0)
        finished = True
    finally:
        if finished:
            engine.shutdown(wait=True)
            if pool is not None:
                pool.shutdown()
            for o in on:
                if o.ask == 'switch':
                    getattr(counter, 'set_' + o.name)(None if o.level else False)          # the switch belongs to this run
                elif o.ask == 'side':
                    getattr(counter, 'set_' + o.name)(False)
        else:
            # an exception is on its way out (a DeviceFault from the engine thread, a broken input): the batch queued behind
            # the failed one must not be handed to a device that may be hung, and nobody waits for it -- the caller exits,
            # or tells the other ranks (dist.any_rank), right away
            for fut in in_flight:
                fut.cancel()
            engine.shutdown(wait=False, cancel_futures=True)
            if pool is not None:
                pool.shutdown(wait=False, cancel_futures=True)
    return rows


def index(argv):
    parser = argparse.ArgumentParser(description="Fast5 raw data archive indexing")
    parser.add_argument("input", help="Input batch or directory of batches")
    parser.add_argument("--recursive", action='store_true', help="Recursively scan input")
    parser.add_argument("--out_prefix", default="", help="Prefix for file paths in output")
    parser.add_argument("--tmp_prefix", default=None, help="Prefix for temporary data")
    args = parser.parse_args(argv)
    for record in Fast5Index.index_records(args.input, recursive=args.recursive, out_prefix=args.out_prefix):
        print(record)


def plot(argv):
    """The `plot` command (argument contract of scripts/STRique.py:948-960).  The figures themselves are this
    package's own: strique_amd/plotting.py draws them from the TSV columns `offset` / `ticks` / scores."""
    parser = argparse.ArgumentParser(description="Signal plots over STR expansions")
    parser.add_argument("f5Index", help="Fast5 index")
    parser.add_argument("--counts", default=None, help="Repeat count output from STRique, if not given read from stdin")
    parser.add_argument("--output", default=None, help="Output directory for plots, use instead of interactive GUI")
    parser.add_argument("--format", default='png', choices=["png", "pdf", "svg"], help="Output format when writing to files")
    parser.add_argument("--width", default=16, type=int, help="Plot width")
    parser.add_argument("--height", default=9, type=int, help="Plot height")
    parser.add_argument("--dpi", default=80, type=int, help="Resolution of plot")
    parser.add_argument("--extension", type=float, default=0.1, help="Extension as fraction of repeat signal around STR region to plot")
    parser.add_argument("--zoom", type=int, default=500, help="Region around prefix and suffix to plot")
    parser.add_argument("--units", default=None, metavar="FILE", help="Repeat-unit positions from `count --units`: marked in the panels")
    parser.add_argument("--tract-positions", dest="tract_positions", default=None, metavar="FILE",
                        help="Unit positions per tract from `count --tract-positions`: marked in the panels, one tick colour per tract")
    parser.add_argument("--log_level", default='warning', choices=LEVELS, help="Log level")
    args = parser.parse_args(argv)
    log = Log(args.log_level)
    if not os.path.isfile(args.f5Index):
        log("Main: Fast5 index file does not exist.", 'error'); raise SystemExit(1)
    from . import plotting
    import matplotlib
    if args.output:
        matplotlib.use("Agg")
        os.makedirs(args.output, exist_ok=True)
    from matplotlib.figure import Figure
    reads = Fast5Index(args.f5Index)
    unit_pos = None
    if args.units:
        with open(args.units) as f:
            unit_pos = {(r[0], r[1], r[2]): r[4] for r in parse_units(f)}
    tract_pos = None
    if args.tract_positions:
        with open(args.tract_positions) as f:
            tract_pos = {(r[0], r[1], r[2]): r[4][2] for r in tracts_mod.parse_positions(f) if r[4] is not None and r[4][2] is not None}
    made = []
    with (open(args.counts) if args.counts else sys.stdin) as stream:
        for row in plotting.parse_counts(stream):
            raw = reads.get_raw(row.read_id)
            if raw is None:
                log("Plot: No fast5 for ID %s" % row.read_id, 'warning'); continue
            if args.output:
                fig = Figure(figsize=(args.width, args.height), dpi=args.dpi, layout="constrained")
            else:
                import matplotlib.pyplot as plt
                fig = plt.figure(figsize=(args.width, args.height), dpi=args.dpi, layout="constrained")
            key = (row.read_id, row.target, row.strand)
            extra = {}
            if unit_pos is not None:
                extra['units'] = unit_pos.get(key, [])
            if tract_pos is not None:
                extra['tract_positions'] = tract_pos.get(key, ())          # (a read without positions: every Axes carries an empty tuple)
            plotting.draw(fig, raw, row, extension=args.extension, zoom=args.zoom, **extra)
            if args.output:
                path = os.path.join(args.output, plotting.figure_name(row, args.format))
                fig.savefig(path); made.append(path)
            else:
                plt.show()
    return made


def calibrate_reads(items, counter, min_score, posterior=False):
    """One pass of `calibrate` over a batch: items [(target, raw signal, strand)] through counter.state_stats_batch; the records
    calibrate.pool takes (posterior: calibrate.pool_posterior, from the state posteriors), of the reads that have statistics and whose
    two flank scores are at least min_score."""
    records = []
    got = counter.state_stats_batch(items, posterior=True) if posterior else counter.state_stats_batch(items)
    for (target, _, strand), (row, stats) in zip(items, got):
        if stats is None or row[1] < min_score or row[2] < min_score:
            continue
        model = counter.targets[target][0 if strand == '+' else 1].repeatHMM
        records.append((model.state_kmers(),) + tuple(stats[:3]))
    return records


def calibrate(argv):
    from . import calibrate as cal
    parser = argparse.ArgumentParser(prog="STRique.py calibrate",
                                     description="Re-estimate the k-mer levels of the configured repeat loci from the reads that span them: the mean of the "
                                                 "observations the best path of the count decode assigns to every match state (one pass; for a second "
                                                 "round run the command again with the table it wrote as the model)")
    parser.add_argument("f5Index", help="Fast5 index")
    parser.add_argument("model", help="Pore model")
    parser.add_argument("repeat", help="Repeat region config file")
    parser.add_argument("--out", required=True, metavar="MODEL", help="The re-estimated pore model: every k-mer of the input table in input order")
    parser.add_argument("--min-score", dest="min_score", type=float, default=None, metavar="S",
                        help="A read contributes when both of its flank scores are at least S.  Required: there is no default (README, 'Calibrate')")
    parser.add_argument("--min-obs", dest="min_obs", type=int, default=None, metavar="N",
                        help="A k-mer's mean is replaced when at least N observations were assigned to it: the standard error of a level is stdv / sqrt(N).  "
                             "Required: there is no default (README, 'Calibrate')")
    parser.add_argument("--stats", default=None, metavar="FILE", help="Also write one row per k-mer seen to FILE, columns " + " ".join(cal.STATS_HEADER))
    parser.add_argument("--posterior", action="store_true",
                        help="Soft assignment: every observation is shared among the states in proportion to the posterior probability that the state "
                             "emitted it (forward-backward over all paths) instead of going wholly to the state of the best path; --min-obs then counts "
                             "expected observations, and the third column of --stats is exp_obs (README, 'Calibrate')")
    parser.add_argument("--config", help="Config file with HMM transition probabilities")
    parser.add_argument("--algn", default=None, help="Alignment in sam format, if not given read from stdin")
    parser.add_argument("--batch", type=int, default=2048, help="Reads per GPU batch")
    parser.add_argument("--device", type=int, default=0, help="HIP device")
    parser.add_argument("--log_level", default='warning', choices=LEVELS, help="Log level")
    parser.add_argument("--mod_model", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--scan", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args(argv)
    if args.min_score is None:
        parser.error("calibrate needs --min-score S: which reads hold their flanks well enough to teach the table is the caller's decision, so there is no default")
    if args.min_obs is None:
        parser.error("calibrate needs --min-obs N: the standard error of a level is stdv / sqrt(N), so there is no default")
    if args.min_obs < 1:
        parser.error("--min-obs must be at least 1")
    if args.mod_model:
        parser.error("calibrate cannot be combined with --mod_model: it re-estimates the levels of one table from the flanked decode")
    if args.scan:
        parser.error("calibrate cannot be combined with --scan: the state statistics are not available in a scan")
    from . import dist as sdist
    if sdist.env_rank_world()[1] > 1:
        parser.error("calibrate runs in a single process: the statistics of several ranks are not pooled")
    log = Log(args.log_level)
    config = parse_config(args.repeat, args.config, log)
    for path, what in ((args.f5Index, "Fast5 index file"), (args.model, "Pore model file")):
        if not os.path.isfile(path):
            log("Main: %s does not exist." % what, 'error'); raise SystemExit(1)
    from .counter import repeatCounter
    counter = repeatCounter(args.model, align_config=config['align'], HMM_config=config['HMM'], device=args.device)
    loci = defaultdict(list)
    for name, (chrom, begin, end, repeat, prefix, suffix) in config['repeat'].items():
        counter.add_target(name, repeat, prefix, suffix)
        loci[chrom].append((name, begin, end))
    f5 = Fast5Index(args.f5Index)
    stream = open(args.algn) if args.algn else sys.stdin
    records, batch, n_reads = [], [], 0
    try:
        for qname, strand, targets, _ in route(stream, loci, log):
            raw = f5.get_raw(qname)
            if raw is None:
                log("Detector: No fast5 for ID %s" % qname, 'warning'); continue
            for target in targets:
                batch.append((target, raw, strand)); n_reads += 1
            if len(batch) >= max(1, args.batch):
                records += calibrate_reads(batch, counter, args.min_score, args.posterior); batch = []
        if batch:
            records += calibrate_reads(batch, counter, args.min_score, args.posterior)
    finally:
        if args.algn:
            stream.close()
    new_means, rows = cal.estimate(cal.pool_posterior(records) if args.posterior else cal.pool(records), counter.pm, args.min_obs)
    cal.write_model(args.out, counter.pm, new_means)
    if args.stats:
        with open(args.stats, 'w') as fp:
            fp.write(cal.format(rows, posterior=True) if args.posterior else cal.format(rows))
    log("Main: %d of %d read(s) contributed, %d k-mer(s) updated." % (len(records), n_reads, len(new_means)), 'info')


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    parser = argparse.ArgumentParser(description='STRique: a nanopore raw signal repeat detection pipeline (MI355X engine)',
                                     usage='''STRique.py <command> [<args>]
Available commands are:
   index      Index batch(es) of bulk-fast5 or tar archived single fast5
   count      Count single read repeat expansions
   plot       Plot repeat signal after counting
   calibrate  Re-estimate the k-mer levels of the repeat loci from spanning reads
''')
    parser.add_argument('command', help='Subcommand to run')
    args = parser.parse_args(argv[:1])
    if args.command == 'count':
        count(argv[1:])
    elif args.command == 'index':
        index(argv[1:])
    elif args.command == 'plot':
        plot(argv[1:])
    elif args.command == 'calibrate':
        calibrate(argv[1:])
    else:
        print('Unrecognized command', file=sys.stderr)
        parser.print_help(file=sys.stderr)
        raise SystemExit(1)


if __name__ == '__main__':
    main()
