"""repeatCounter: per-read repeat detection on the GPU.

Host-side mirror of the reference's `repeatCounter` (scripts/STRique.py:505-618): same
constructor arguments, `add_target(target_name, repeat, prefix, suffix)` and
`detect(target_name, raw_signal, strand)` with the same return tuple and the same ValueErrors.
`detect_batch` is the throughput entry: many (read, target, strand) triples in one device pipeline.

All numerical work of detect() happens in libstrique_hip (strique_amd/ffi.py); this module only
builds the per-target inputs (flank templates, HMM arrays) and turns results into the reference's
output tuple.
"""
import contextlib
from collections import namedtuple

import numpy as np

from . import anchored as anchored_mod
from . import ffi
from . import flank_mod as flank_mod_rule
from . import hmm as hmm_mod
from . import motifs as motifs_mod
from . import renorm as renorm_mod
from . import tracts as tracts_mod
from .pore_model import pore_model

ALIGN_DEFAULTS = {'dist_offset': 16.0, 'dist_min': 0.0, 'gap_open_h': -1.0, 'gap_open_v': -16.0,
                  'gap_extension_h': -1.0, 'gap_extension_v': -16.0, 'samples': 6}       # STRique.py:507-513

_COMPLEMENT = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def reverse_complement(sequence):
    return "".join(_COMPLEMENT.get(base, base) for base in reversed(sequence))      # STRique.py:534-536


target_classifier = namedtuple('target_classifier',
                               ['prefix', 'suffix', 'prefix_ext', 'suffix_ext', 'repeatHMM', 'modHMM', 'target_id'])

# one read out of the device pipeline: the tuple detect() returns, and what was asked for beside it (None otherwise) -- unit positions,
# (log_lik, count_mean, count_sd), per-unit log-likelihood ratios, the anchored record (kind, status, count, log_p, begin, end,
# free_samples -- every kind, as strq_batch_fetch_anchored hands it out); see repeatCounter.detect_batch
# variants: (count_v, pattern, branch, end, V) of the variant pass, see repeatCounter.detect_batch
# renorm: (applied, {signal: None or (a, b, w, score)}) of the second normalisation step, see repeatCounter.set_renorm
# anchored_mod: None or (pattern, llr) -- the methylation call of an anchored read, see repeatCounter.set_anchored_mod
# tracts: None or (counts in configured order, log_p) of the compound model, see repeatCounter.set_tracts
# (`tracts` stays the last field, as an existing test asks; `flank_mod` sits in front of it, so a caller that passed a ninth positional
# value for `tracts` would now fill `flank_mod` -- there is none in the tree: the fields behind `llr` are given by name)
# flank_mod: None or [(flank, pos, n_sites, n_columns, status, begin, end, llr)] -- the calls of the flanks' CpG groups, see repeatCounter.set_flank_mod
Detected = namedtuple('Detected', ['row', 'units', 'conf', 'llr', 'anchored', 'variants', 'renorm', 'anchored_mod', 'flank_mod', 'tracts'],
                      defaults=(None, None, None, None, None, None))


def _ratios(scores):
    """(V_base, V_mod) rows -> V_mod - V_base."""
    return None if scores is None else scores[:, 1] - scores[:, 0]


def _fetch_anchored(counter, reads, idx):
    return [(int(a['kind']), int(a['status']), int(a['count']), float(a['log_p']), int(a['begin']), int(a['end']), int(a['free_samples']))
            for a in counter.ctx.batch_fetch_anchored()]


def _legacy_anchored(a):
    return (anchored_mod.KIND_NAMES[a[0]],) + tuple(a[2:]) if a[0] in (anchored_mod.ENDS_IN_REPEAT, anchored_mod.STARTS_IN_REPEAT) else None


def _fetch_variants(counter, reads, idx):
    out = []
    for i, v in zip(idx, counter.ctx.batch_fetch_variants()):
        if v is not None:
            m = counter.variant_models[reads[i][0]]
            pattern = "".join("0" if b == 0 else "0" * m.context_units + str(int(b)) for b in v[1])
            v = (v[0], pattern, v[1], v[2], v[3].reshape(len(v[1]), m.n_branches))      # (a read without passages: (0, NB))
        out.append(v)
    return out


def _fetch_renorm(counter, reads, idx):
    return [(int(r['applied']), {s: (int(f['a']), int(f['b']), int(f['w']), int(f['score'])) if f['fitted'] else None
                                 for s, f in zip(renorm_mod.SIGNALS, r['fit'])}) for r in counter.ctx.batch_fetch_renorm()]


def _fetch_tracts(counter, reads, idx):
    out = []
    recs = counter.ctx.batch_fetch_tracts()
    # set_tracts(True, positions=True): the positions come with the records (None: back-pointers over the budget)
    positions = counter.ctx.batch_fetch_tract_positions() if counter.tract_positions else [None] * len(recs)
    for i, t, p in zip(idx, recs, positions):
        rec = None
        if int(t['status']) == 0:
            strand = counter.tract_models[reads[i][0]][1]
            k = int(t['n_tracts'])
            rec = (tracts_mod.configured_order([int(c) for c in t['count'][:k]], strand), float(t['log_p']))
            if counter.tract_positions:
                rec += (tracts_mod.configured_order(p[1][:k], strand) if p[0] == 0 else None,)
        out.append(rec)
    return out


def _fetch_flank_mod(counter, reads, idx):
    return [None if g is None else [(int(x['flank']), int(x['pos']), int(x['n_sites']), int(x['n_columns']), int(x['status']), int(x['begin']), int(x['end']),
                                     float(x['v_mod'] - x['v_base'])) for x in g] for g in counter.ctx.batch_fetch_flank_mod()]


# The optional passes of detect / detect_batch, in the order their switches go on.  name: the pass -- a keyword of detect and
# detect_batch (keyword) or the attribute a set_<name> switch of the counter keeps; what it holds is the pass's value in a request and,
# with `level`, travels to the context's switch.  field: its field of Detected.  ensure: the method that registers its models first.
# fetch(counter, reads, idx): its value for every read of the device batch, reads[idx[k]] being read k.  place: where it stands
# behind the row in the tuple detect_batch returns without records=True (None: in Detected only), as legacy(value).
Pass = namedtuple('Pass', ['name', 'field', 'keyword', 'ensure', 'level', 'fetch', 'place', 'legacy'], defaults=(lambda value: value,))
PASSES = (
    Pass('anchored', 'anchored', True, '_ensure_anchored', True, _fetch_anchored, 3, _legacy_anchored),
    Pass('anchored_mod', 'anchored_mod', False, None, False,
         lambda c, reads, idx: [None if x is None else (x[0], _ratios(x[1])) for x in c.ctx.batch_fetch_anchored_mod()], 4),
    Pass('units', 'units', True, None, False, lambda c, reads, idx: c.ctx.batch_fetch_units(), 0),
    Pass('confidence', 'conf', True, None, False, lambda c, reads, idx: c.ctx.batch_fetch_confidence(), 1),
    Pass('mod_llr', 'llr', True, None, False, lambda c, reads, idx: [_ratios(v) for v in c.ctx.batch_fetch_mod_llr()], 2),
    Pass('variants', 'variants', False, '_ensure_variants', False, _fetch_variants, 5),
    Pass('renorm', 'renorm', False, '_ensure_renorm', True, _fetch_renorm, None),
    Pass('tracts', 'tracts', False, '_ensure_tracts', False, _fetch_tracts, 6),
    Pass('flank_mod', 'flank_mod', False, '_ensure_flank_mod', False, _fetch_flank_mod, 7),
)


class repeatCounter(object):
    def __init__(self, model_file, mod_model_file=None, align_config=None, HMM_config=None, device=0, context=None):
        cfg = dict(ALIGN_DEFAULTS)
        if align_config and isinstance(align_config, dict):
            cfg.update(align_config)
        self.ctx = context if context is not None else ffi.Context(device)
        self.ctx.set_align_params(cfg['gap_open_h'], cfg['gap_extension_h'], cfg['gap_open_v'], cfg['gap_extension_v'],
                                  cfg['dist_offset'], cfg['dist_min'])
        self.pm = model_file if isinstance(model_file, pore_model) else pore_model(model_file)
        if mod_model_file:
            self.pm_mod = mod_model_file if isinstance(mod_model_file, pore_model) else pore_model(mod_model_file)
        else:
            self.pm_mod = self.pm
        self.ctx.set_pore_stats(self.pm.model_tail_lo, self.pm.model_tail_hi, self.pm.model_min, self.pm.model_max)
        self.samples = cfg['samples']
        self.HMM_config = HMM_config
        self.targets = {}
        # anchored counting: what the two extra models of a classifier are baked from, and the classifiers that have them
        # registered ({target_id: {kind: {'model_id', 'bias', 'states', 'positions_rc', 'positions_error'}}}); nothing is baked before somebody asks
        self._anchored_src = {}
        self.anchored_models = {}
        # variants: (repeat, alt units) of the classifiers of a target added with alt units, and the classifiers whose variant model is
        # registered ({target_id: RepeatVariantModel}); baked when somebody asks, like the anchored models
        self._variant_src = {}
        self.variant_models = {}
        self.variant_refused = {}      # {target_id: message} of the variant models strq_target_set_variants refused
        self.variants = False          # set_variants
        self.renorm = None             # set_renorm: min_share, or None
        self.anchored_mod = False      # set_anchored_mod
        # tracts: (units, linkers, prefix, suffix) as the strand reads them, of the classifiers of a target added with a compound
        # definition, and the classifiers whose compound model is registered ({target_id: (CompoundRepeatModel, strand)}); baked on first use
        self._tract_src = {}
        self.tract_models = {}
        self.tracts = False            # set_tracts
        self.tract_positions = False   # set_tracts(True, positions=True)
        self._renorm_done = set()      # classifiers whose tables are registered
        # flank methylation calls: the whole flanks of every classifier as its strand reads them, its strand, and the classifiers whose
        # models are registered or were refused ({target_id: message}); built when the switch first meets them, like the anchored models
        self._flank_src = {}
        self._flank_strand = {}
        self.flank_mod_models = {}
        self.flank_mod_refused = {}
        self.flank_mod = False         # set_flank_mod
        # motifs: (strand, candidates as the strand reads them, prefix, suffix) of the classifiers of a target added with motifs, and the
        # classifiers whose loop and flanked models are registered ({target_id: [(unit, loop id, flanked id, bias)]}); baked on first use
        self._motif_src = {}
        self.motif_models = {}
        self.motif_units = {}          # {target name: the candidates as configured}
        self.motifs = None             # set_motifs: the segment length, or None
        self.motif_records = None      # with set_motifs on: the motif record of every read of the last detect_batch call, in input order
        self._motif_values = {}

    # -------------------------------------------------------------------------------------
    def _classifier(self, repeat, prefix, suffix, prefix_ext, suffix_ext):
        flanked = hmm_mod.FlankedRepeatModel(repeat, prefix, suffix, self.pm, self.HMM_config)
        mod = None
        if self.pm is not self.pm_mod:
            mod = hmm_mod.RepeatModModel(repeat, self.pm, self.pm_mod, self.HMM_config)
        sig = lambda s: self.pm.generate_signal(s, samples=self.samples)
        p, s, pe, se = sig(prefix), sig(suffix), sig(prefix_ext), sig(suffix_ext)
        flanked.model_id = self.ctx.model_create(flanked.baked)
        tid = self.ctx.target_add(pe, se, len(pe) - len(p), len(se) - len(s), self.samples, flanked.model_id,
                                  flanked.count_bias)
        if mod is not None:
            mod.model_id = self.ctx.model_create(mod.baked)
            self.ctx.target_set_mod(tid, mod.model_id, mod.model_min, mod.model_max)
        self._anchored_src[tid] = (repeat, prefix, suffix)
        self._flank_src[tid] = (prefix_ext, suffix_ext)
        return target_classifier(p, s, pe, se, flanked, mod, tid)

    def _ensure_anchored(self):
        """The end / start model of every classifier that has none yet: baked, uploaded and registered with its target."""
        for tid, (repeat, prefix, suffix) in self._anchored_src.items():
            if tid in self.anchored_models:
                continue
            made = {}
            for kind in hmm_mod.ANCHORED_KINDS:
                m = hmm_mod.AnchoredRepeatModel(kind, repeat, prefix, suffix, self.pm, self.HMM_config)
                mid = self.ctx.model_create(m.baked)
                # which kernel the model runs on is reported, not assumed: 0 = the chain builder took its positions (register-resident
                # kernel), 3 = it refused them (lane layout, or the general kernel); tools/anchored_probe.py prints its reason
                made[kind] = {'model_id': mid, 'bias': m.count_bias, 'states': m.baked.n_states, 'positions_rc': self.ctx.last_positions_rc,
                              'positions_error': self.ctx.last_positions_error}
            e, s = made['ends_in_repeat'], made['starts_in_repeat']
            self.ctx.target_set_anchored(tid, e['model_id'], e['bias'], s['model_id'], s['bias'])
            self.anchored_models[tid] = made

    def _ensure_variants(self):
        """The variant model of every classifier with alt units that has none yet: baked, uploaded and registered with its target."""
        refused = None
        for tid, (repeat, alts) in self._variant_src.items():
            if tid in self.variant_models or tid in self.variant_refused:
                continue
            m = hmm_mod.RepeatVariantModel(repeat, alts, self.pm, self.HMM_config)
            m.model_id = self.ctx.model_create(m.baked)
            try:
                self.ctx.target_set_variants(tid, m.model_id, m.model_min, m.model_max, len(m.alt_units), m.context_units)
            except ffi.StriqueHipError as e:
                # a model the pass does not cover: the target stays without one, its reads report None; said once, after the
                # other targets are registered, and the model is not uploaded again
                if e.code != ffi.STRQ_ERR_UNSUPPORTED:
                    raise
                self.variant_refused[tid] = str(e)
                refused = refused or e
                continue
            self.variant_models[tid] = m
        if refused is not None:
            raise refused

    def _ensure_tracts(self):
        """The compound model of every classifier with a tract definition that has none yet: baked, uploaded and registered."""
        for tid, (strand, units, linkers, prefix, suffix) in self._tract_src.items():
            if tid in self.tract_models:
                continue
            m = hmm_mod.CompoundRepeatModel(units, linkers, prefix, suffix, self.pm, self.HMM_config)
            m.model_id = self.ctx.model_create(m.baked)
            self.ctx.model_set_tracts(m.model_id, m.n_tracts, m.tract_of)
            self.ctx.target_set_tracts(tid, m.model_id, m.n_tracts, m.count_bias)
            self.tract_models[tid] = (m, strand)

    def _ensure_motifs(self):
        """The loop model of every candidate, and the flanked model of every alternative, of the classifiers with motifs that have
        none yet: baked, uploaded and registered.  Candidate 0 decodes with the classifier's own flanked model."""
        for tid, (strand, units, prefix, suffix) in self._motif_src.items():
            if tid in self.motif_models:
                continue
            made = []
            for j, unit in enumerate(units):
                flanked = hmm_mod.FlankedRepeatModel(unit, prefix, suffix, self.pm, self.HMM_config)
                loop_id = self.ctx.model_create(motifs_mod.loop_arrays(flanked.baked))
                made.append((unit, loop_id, self.ctx.model_create(flanked.baked) if j else -1, flanked.count_bias))
            self.ctx.target_set_motifs(tid, [m[1] for m in made], [max(m[2], 0) for m in made], [m[3] for m in made])
            self.motif_models[tid] = made

    def motifs_batch(self, items, segment=motifs_mod.SEGMENT):
        """Which repeat unit each stretch of the array is made of (strique_amd.motifs states the rule).  items: iterable of
        (target_name, raw_signal, strand).  Returns [(row, motifs)] in input order: row the tuple detect() returns, unchanged;
        motifs None -- the gate failed, the read was not conditioned, the two flanks leave no stretch between them, or the target
        was added without motifs -- or (majority, shares, count_m, log_p_m, runs, winners, V): the candidate (0 = `repeat`, then the
        alternatives in configured order, on either strand) with the most observations won; every candidate's share of the
        stretch; the count and log-probability of the flanked decode under the majority unit (the row's own for majority 0; None,
        None without a decode); the maximal runs of equal winners as (candidate, first_sample, end_sample) in raw samples, in
        signal order; per segment the winner (int32) and the scores V (n_seg, K) float64.  `segment`: observations per segment, 32
        to 4096.  set_motifs(True, segment) around one detect_batch call; the switch is put back to what it was before it returns, and
        the other switches of the counter (set_renorm, ...) work underneath it.  ValueError when no target was added with motifs.  Not with scan_batch, and not for anchored reads."""
        before = self.motifs
        self.set_motifs(True, segment)
        try:
            rows = self.detect_batch(list(items), records=True)
            return [(d.row, m) for d, m in zip(rows, self.motif_records)]
        finally:
            self.motifs = before

    def set_motifs(self, on, segment=motifs_mod.SEGMENT):
        """on: detect and detect_batch also run the motif track on every read of a target added with motifs=[...], in segments of
        `segment` observations (32 to 4096), and keep the records of their last call in `motif_records`: one entry per read, in input
        order, None or (majority, shares, count_m, log_p_m, runs, winners, V) as motifs_batch describes them.  The tuples detect_batch
        returns and the fields of Detected stay as they are.  A switch of the counter, like set_tracts.  ValueError when no target was
        added with motifs, or for a segment length outside the range.  Not with scan_batch."""
        if not on:
            self.motifs = None
            return
        if not self._motif_src:
            raise ValueError("RepeatCounter: motifs needs a target added with motifs=[...].")
        self.motifs = motifs_mod.check_segment(segment)

    @staticmethod
    def _motif_record(rec, V, win, segment):
        if int(rec['status']) != 0:
            return None
        K, T = int(rec['n_cand']), int(rec['end'] - rec['begin'])
        bounds = motifs_mod.segments(T, segment)
        decoded = int(rec['decode_status']) == 0
        return (int(rec['majority']), tuple(int(o) / T for o in rec['obs_won'][:K]), int(rec['count_m']) if decoded else None,
                float(rec['log_p_m']) if decoded else None, motifs_mod.runs(win, bounds, int(rec['begin'])), win, V)

    def set_tracts(self, on, positions=False):
        """on: detect and detect_batch also decode the compound model of every read of a target added with tracts=(units, linkers)
        (strique_amd.tracts states the rule) and report one more element per read, behind all others: None -- the read was not
        decoded, its window has 2^21 samples or more, the compound model found no path, or its target has no tracts -- or (counts,
        log_p): the unit count of every tract in the order the definition was configured in, on either strand, and the
        log-probability of the compound model's best path.  records=True: Detected.tracts.  A switch of the counter, like
        set_variants.  ValueError when no target was added with tracts.  Not with scan_batch.
        positions=True: the element is (counts, log_p, positions) -- positions a tuple of one ascending np.int64 array of raw-signal
        samples per tract, in configured order like the counts (count_j - bias_j of them: strique_amd.tracts states the rule), or
        None for a read whose back-pointers exceed STRQ_TRACT_POS_WS_BYTES.  Without it the element is exactly (counts, log_p)."""
        if on and not self._tract_src:
            raise ValueError("RepeatCounter: tracts needs a target added with tracts=(units, linkers).")
        self.tracts = bool(on)
        self.tract_positions = bool(on and positions)

    def _ensure_renorm(self):
        """The tables of the second normalisation step for every classifier that has none yet (strique_amd.renorm.tables)."""
        for tid, (repeat, _, _) in self._anchored_src.items():
            if tid in self._renorm_done:
                continue
            Q, A = renorm_mod.tables(self.pm.model_dict, self.pm.kmer, self.pm.model_min, self.pm.model_max, repeat)
            self.ctx.target_set_renorm(tid, Q, A, self.pm.model_min, self.pm.model_max)
            self._renorm_done.add(tid)

    def set_renorm(self, min_share):
        """min_share in (0, 1): detect and detect_batch refit scale and shift of every read's normalised signals against its
        target's k-mer composition (strique_amd.renorm states the rule) and run on the corrected maps where the fitted repeat share
        reaches min_share -- the rows of such reads change, which is the point: a read that is mostly repeat is stretched by the
        whole-read statistics of detect() until its flanks are not found.  There is no default (README, "Renorm").  None or False:
        off.  A switch of the counter, like set_variants: the keywords of detect stay; records=True reports the fit of every read
        as Detected.renorm = (applied, {'morph' | 'filtered' | 'raw': None or (a, b, w, score)}).  Not with scan_batch."""
        if min_share is None or min_share is False:
            self.renorm = None
            return
        if not 0 < min_share < 1:
            raise ValueError("RepeatCounter: the renorm share threshold must be inside (0, 1).")
        self.renorm = float(min_share)

    @property
    def renorm_bin_width(self):
        """Width of a bin of the rule's grid in pA (beta of a fit is b bins)."""
        return renorm_mod.grid(self.pm.model_min, self.pm.model_max)[1]

    def _ensure_flank_mod(self):
        """The two flank profile models and the site models of every classifier that has none yet: baked, uploaded and registered.  A
        flank flank_mod.check refuses leaves its target without calls (flank_mod_refused holds the message); the rows are unchanged."""
        for tid, flanks in self._flank_src.items():
            if tid in self.flank_mod_models or tid in self.flank_mod_refused or tid not in self._flank_strand:
                continue
            strand, k = self._flank_strand[tid], self.pm.kmer
            try:
                checked = [flank_mod_rule.check(f, k, ("prefix", "suffix")[w]) for w, f in enumerate(flanks)]
            except ValueError as e:
                self.flank_mod_refused[tid] = str(e)
                continue
            made = []
            for which, (flank, groups) in enumerate(zip(flanks, checked)):
                seg = hmm_mod.FlankProfileModel(flank, self.pm, self.HMM_config)
                seg.model_id = self.ctx.model_create(seg.baked)
                rows = []
                for g in groups:
                    site = hmm_mod.SiteModModel(flank_mod_rule.site_sequence(flank, g, k), self.pm, self.pm_mod, self.HMM_config)
                    cfg_flank, pos = flank_mod_rule.configured(which, g, len(flank), strand)
                    rows.append((g.c0, g.c1, self.ctx.model_create(site.baked), cfg_flank, pos, g.n_sites))
                self.ctx.target_set_flank_mod(tid, which, seg.model_id, len(flank), seg.column_of[:seg.baked.silent_start], rows)
                made.append((seg, groups))
            self.flank_mod_models[tid] = made

    def set_flank_mod(self, on):
        """on: detect and detect_batch also call the CpG groups of the configured flanks (strique_amd.flank_mod states the rule) and
        report one more element per read, behind all others: None -- the gate failed, the read could not be conditioned, or its target
        has no flank calls -- or a list of (flank, pos, n_sites, n_columns, status, begin, end, llr), one per group of a flank whose
        stretch exists: the flank (0 prefix, 1 suffix) and the position of the group's first C as configured on the + strand, the
        status (flank_mod.STATUS_NAMES), the raw samples of u and w and llr = V_mod - V_base (-1, -1 and NaN unless scored).
        records=True: Detected.flank_mod.  A switch of the counter, like set_anchored_mod.  ValueError without a modification
        model.  Not with scan_batch."""
        if on and self.pm is self.pm_mod:
            raise ValueError("RepeatCounter: flank_mod needs a modification model.")
        self.flank_mod = bool(on)

    def set_anchored_mod(self, on):
        """on: detect and detect_batch with anchored=m also call the methylation pattern of the reads that hold one flank only
        (strique_amd.anchored states which reads get a call and on which stretch) and report one more element per read, directly
        behind the anchored one: None, or (pattern, llr) -- the '0' / '1' string of the units the dual model passes on the raw-signal
        samples [begin, end) of the record ('-' when it finds no path), and with mod_llr=True the float64 array V_mod - V_base with
        one value per character (None without it, or for a pattern without units).  records=True: Detected.anchored_mod.  A switch
        of the counter, like set_variants: the keywords of detect and detect_batch stay those every stand-in counter of run_count
        answers.  ValueError without a modification model; a call without anchored=m is a ValueError then.  Not with scan_batch."""
        if on and self.pm is self.pm_mod:
            raise ValueError("RepeatCounter: anchored_mod needs a modification model.")
        self.anchored_mod = bool(on)

    def set_variants(self, on):
        """on: detect and detect_batch also run the variant pass (strq_set_variants) and report one more element per read -- see
        detect_batch.  ValueError when no target was added with alt_units.  Not with scan_batch."""
        if on and not self._variant_src:
            raise ValueError("RepeatCounter: variants needs a target added with alt_units.")
        self.variants = bool(on)

    def add_target(self, target_name, repeat, prefix, suffix, alt_units=None, tracts=None, motifs=None):
        """alt_units: 1 to 3 sequence variants of the repeat unit (on the + strand, as `repeat`) that detect
        tells from it once set_variants(True) is called; ValueError for units hmm.check_alt_units does not take.
        tracts: (units, linkers), the compound definition of the locus on the + strand (strique_amd.tracts: 2 or 3 units, one linker
        -- possibly empty -- between neighbours), counted per tract once set_tracts(True) is called; ValueError for what
        tracts.check does not take.  `repeat` stays the unit of the count row.
        motifs: 1 to 3 alternative units of any length (on the + strand, as `repeat`) the array may be made of instead; motifs_batch
        says which one each stretch of a read's array is made of; ValueError for what strique_amd.motifs.check does not take."""
        if target_name in self.targets:
            raise ValueError("RepeatCounter: Target with name " + str(target_name) + " already defined.")
        alts = hmm_mod.check_alt_units(repeat, alt_units) if alt_units else None
        tract_def = tracts_mod.check(*tracts) if tracts else None
        candidates = motifs_mod.check(repeat, motifs, self.pm.kmer) if motifs else None
        prefix_ext = prefix.upper(); prefix = prefix[-50:].upper()            # STRique.py:555-559
        suffix_ext = suffix.upper(); suffix = suffix[:50].upper()
        repeat = repeat.upper()
        rc = reverse_complement
        tc_plus = self._classifier(repeat, prefix, suffix, prefix_ext, suffix_ext)
        # reverse strand: flanks swap roles (STRique.py:569-575)
        tc_minus = self._classifier(rc(repeat), rc(suffix), rc(prefix), rc(suffix_ext), rc(prefix_ext))
        self.targets[target_name] = (tc_plus, tc_minus)
        self._flank_strand[tc_plus.target_id] = '+'; self._flank_strand[tc_minus.target_id] = '-'
        if alts:
            # the - strand reads the reverse complement of unit and alt units; calls are reported with the number of the unit as configured
            self._variant_src[tc_plus.target_id] = (repeat, alts)
            self._variant_src[tc_minus.target_id] = (rc(repeat), [rc(a) for a in alts])
        if candidates:
            # the - strand reads the reverse complement of every candidate; results are reported in the configured order
            self.motif_units[target_name] = tuple(candidates)
            self._motif_src[tc_plus.target_id] = ('+', motifs_mod.strand_units(candidates, '+'), prefix, suffix)
            self._motif_src[tc_minus.target_id] = ('-', motifs_mod.strand_units(candidates, '-'), rc(suffix), rc(prefix))
        if tract_def:
            # the - strand reads the reverse complements in reverse order; counts are reported in the configured order
            self._tract_src[tc_plus.target_id] = ('+',) + tracts_mod.strand_definition(*tract_def, '+') + (prefix, suffix)
            self._tract_src[tc_minus.target_id] = ('-',) + tracts_mod.strand_definition(*tract_def, '-') + (rc(suffix), rc(prefix))

    def _classifier_for(self, target_name, strand):
        if target_name not in self.targets:
            raise ValueError("RepeatCounter: Target with name " + str(target_name) + " not defined.")
        if strand == '+':
            return self.targets[target_name][0]
        if strand == '-':
            return self.targets[target_name][1]
        raise ValueError("RepeatCounter: Strand must be + or -.")

    # -------------------------------------------------------------------------------------
    def detect_batch(self, items, units=False, confidence=False, mod_llr=False, anchored=None, records=False):
        """items: iterable of (target_name, raw_signal, strand).  Returns a list of the tuples
        detect() returns, in input order.  units=True: a list of (tuple, positions) instead, positions being the
        raw-signal sample indices of the repeat units on the decoded Viterbi path (one np.int64 array per read, ascending;
        None when the read was not decoded -- gate failed, no path; strq_set_units).
        confidence=True: a list of (tuple, conf) -- (tuple, positions, conf) with units=True -- conf being (log_lik, count_mean,
        count_sd) as floats: the forward log-likelihood of the decoded window over all paths (log_p is the best one's), and the
        posterior mean and standard deviation of the count (count_bias included); None when the read was not decoded
        (strq_set_confidence).
        mod_llr=True (a counter with a modification model): the per-unit log-likelihood ratio of the mCpG calls comes last -- a
        float64 array V_mod - V_base with one value per character of mod_pattern (>= 0 where it says '1', <= 0 where it says '0',
        +-inf where one branch has no path), or None for a read without units (strq_set_mod_llr).
        anchored=m (a score threshold above 0; there is no default): one more element after them, for a read that holds one flank
        only -- it ends inside the repeat, or starts there (strique_amd.anchored.classify states the rule, with m the threshold on the
        two normalised flank scores) -- (kind, count, log_p, begin, end, free_samples): kind 'ends_in_repeat' or 'starts_in_repeat',
        the count of the repeat units the read holds (a lower bound on the allele up to the decode's own error, not a proven one),
        the raw-signal samples [begin, end) decoded into the repeat, and the observations the free state took (a handful on a read
        that really ends in the repeat, thousands on one wrongly taken for anchored).  A read whose decode found no path has zeros
        behind its kind; None for every other read (spanning, or neither).  The tuple itself does not change.
        With set_variants(True) (a counter with a target added with alt_units; a switch of the counter, not a keyword: the keywords of
        detect and detect_batch are those every stand-in counter of run_count answers): one more element after all of them -- None for a read that was
        not decoded or whose target has no alt units, else (count_v, pattern, branch, end, V): the variant model's passages in
        signal order.  branch (int8 array) is 0 for a passage through the repeat unit's profile, b for one through alt unit b's (the
        b-th unit as configured, on either strand); end (int64) the raw sample of the hub emission behind each passage; V
        (float64 [n_passages, 1 + n_alt]) every branch's masked Viterbi score of the passage, -inf without a path -- a base passage
        scored under an alt branch is an (m + 1)-unit profile forced onto one unit of signal, meaningful only as "very negative".
        pattern has one character per unit: '0' per base passage, '0' * m + str(b) per alt passage (m = the model's context units);
        count_v = len(pattern) + count_bias is an estimate on the scale of the tuple's count, not equal to it in general.
        With set_anchored_mod(True) and anchored=m: the methylation call of the read, (pattern, llr) or None, directly behind the
        anchored element -- see set_anchored_mod.
        With set_tracts(True) (a counter with a target added with tracts=): one last element, None or (counts, log_p) -- see set_tracts;
        (counts, log_p, positions) with set_tracts(True, positions=True).
        Order of the elements: (tuple[, positions][, conf][, llr][, anchored][, anchored_mod][, variants][, tracts][, flank_mod]); without any of them the bare tuple.
        records=True: a list of Detected records instead (the fields that were not asked for None; `anchored` the record of every
        read, whatever its kind: (kind number, status, count, log_p, begin, end, free_samples))."""
        items = list(items)
        if mod_llr and self.pm is self.pm_mod:
            raise ValueError("RepeatCounter: mod_llr needs a modification model.")
        if anchored is not None and not anchored > 0:
            raise ValueError("RepeatCounter: the anchored score threshold must be above 0.")
        if self.anchored_mod and anchored is None:
            raise ValueError("RepeatCounter: anchored_mod needs anchored=m (the calls hang on the anchored records).")
        asked = dict(units=units, confidence=confidence, mod_llr=mod_llr, anchored=anchored)
        request = {}
        for p in PASSES:
            value = asked[p.name] if p.keyword else getattr(self, p.name)
            if value:          # (a level that is on is never 0: anchored was checked above, set_renorm keeps None or a share inside (0, 1))
                request[p.name] = value
        legacy = sorted((p for p in PASSES if p.name in request and p.place is not None), key=lambda p: p.place)
        reads = [(self._classifier_for(t, s).target_id, r) for t, r, s in items]
        out = [None] * len(items)
        self._motif_values = {}
        self.motif_records = None
        for i, d, _, _ in self._run(reads, request):
            if records:
                out[i] = d
                continue
            extra = tuple(p.legacy(getattr(d, p.field)) for p in legacy)
            out[i] = (d.row,) + extra if extra else d.row
        if self.motifs is not None:
            self.motif_records = [self._motif_values.get(i) for i in range(len(items))]
        return out

    def state_stats_batch(self, items, posterior=False):
        """items: iterable of (target_name, raw_signal, strand).  Returns [(row, stats)] in input order: row the tuple detect()
        returns, unchanged; stats None -- the gate failed, the read was not conditioned, the flanked decode found no path, or the
        window's back-pointers exceed STRQ_STATE_STATS_WS_BYTES -- or (n, sum, sumsq): per emitting state of the read's flanked model
        (targets[name][0 | 1].repeatHMM.state_kmers() says what each stands for) the count, the sum and the sum of squares of the
        observations the best path assigns to it (strique_amd.state_stats states the rule, strique_amd.calibrate uses it).  A method
        of its own, not a keyword of detect_batch: it turns the context's switch on around the run and off again before it returns;
        the switches of the counter (set_renorm, ...) work underneath it.  Not with scan_batch.
        posterior=True: the soft counterpart -- the switch of the state posteriors instead (forward-backward over the same windows,
        strique_amd.state_posteriors states the rule); stats is then None -- as above, or the forward pass found no path, or the
        window's stored vectors exceed STRQ_STATE_POST_WS_BYTES -- or (w, wx, wxx, log_lik): per emitting state the posterior
        occupancy and its first two moments of the observations, and the window's forward log-likelihood."""
        switch, fetch = ((self.ctx.set_state_posteriors, self.ctx.batch_fetch_state_posteriors) if posterior else
                         (self.ctx.set_state_stats, self.ctx.batch_fetch_state_stats))
        items = list(items)
        request = {p.name: getattr(self, p.name) for p in PASSES if not p.keyword and getattr(self, p.name)}
        reads = [(self._classifier_for(t, s).target_id, np.asarray(r)) for t, r, s in items]
        out = [None] * len(items)
        is_int = [self._fits_int16(r) for _, r in reads]
        try:
            for want_int in (True, False):          # one device batch each, as _run splits them: the statistics are those of the last batch
                idx = [i for i, f in enumerate(is_int) if f == want_int]
                if not idx:
                    continue
                switch(True)
                rows = {k: d.row for k, d, _, _ in self._run([reads[i] for i in idx], request)}
                stats = fetch()
                for k, i in enumerate(idx):
                    out[i] = (rows[k], stats[k])
        finally:
            switch(False)
        return out

    @contextlib.contextmanager
    def _switches(self, request):
        """The passes of `request` ({name: value}, see PASSES) are on inside the block, and every pass is off after it."""
        with_positions = 'tracts' in request and self.tract_positions      # (rides on the tracts switch; a context is asked only then)
        with_motifs = self.motifs is not None                              # (a switch of its own behind the passes; a context is asked only then)
        try:
            # inside the try: set_mod_llr refuses a modification model the scoring pass does not cover, and the switches a
            # failed call leaves behind must not stay on for the next caller of a shared context
            for p in PASSES:
                if p.name in request:
                    if p.ensure:
                        getattr(self, p.ensure)()
                    getattr(self.ctx, 'set_' + p.name)(True, *((request[p.name],) if p.level else ()))
            if with_positions:
                self.ctx.set_tract_positions(True)
            if with_motifs:
                self._ensure_motifs()
                self.ctx.set_motifs(True, self.motifs)
            yield
        finally:
            if with_motifs:
                self.ctx.set_motifs(False)
            if with_positions:
                self.ctx.set_tract_positions(False)
            for p in reversed(PASSES):
                getattr(self.ctx, 'set_' + p.name)(False)

    def _run(self, reads, request, scan=None):
        """reads: [(target_id, raw_signal)] through the context with the passes of `request` on (_switches).  Yields (position in
        `reads`, Detected, winner, scores) per read, the fields of Detected that were not asked for being None.  scan=(candidate
        target ids, min_score): the target ids of the reads are ignored, every read is compared with every candidate
        (Context.scan_batch_reads); winner is its position in the candidate list or -1, scores the [n_candidates, 2] array of its
        flank scores (both None without scan)."""
        sigs = [np.asarray(r) for _, r in reads]
        # DAC samples that fit int16 take their order statistics from exact histograms; everything else is float64
        # (radix selection on the GPU, cond_kernels.hip: f64_stats_kernel).  A mixed batch runs as two device batches.
        is_int = [self._fits_int16(s) for s in sigs]
        for want_int in (True, False):
            idx = [i for i, f in enumerate(is_int) if f == want_int]
            if not idx:
                continue
            arrs = [sigs[i].astype(np.int16 if want_int else np.float64, copy=False) for i in idx]
            with self._switches(request):
                if scan is None:
                    res = self.ctx.detect_batch_reads(arrs, [reads[i][0] for i in idx])      # one pointer per read: no host-side concatenation
                    win = sc = [None] * len(res)
                else:
                    res, win, sc = self.ctx.scan_batch_reads(arrs, scan[0], scan[1], scores=True)
                mods = self.ctx.batch_fetch_mod() if self.pm is not self.pm_mod else ['-'] * len(res)
                fetched = {p.field: p.fetch(self, reads, idx) for p in PASSES if p.name in request}
                if self.motifs is not None and scan is None:
                    rec, V, win = self.ctx.batch_fetch_motifs()
                    for k, i in enumerate(idx):
                        self._motif_values[i] = self._motif_record(rec[k], V[k], win[k], self.motifs)
            # one column per field of Detected behind the row, in the record's own order: all None for a pass that is off
            columns = zip(*[fetched.get(f, [None] * len(res)) for f in Detected._fields[1:]])
            for i, r, m, w, s, values in zip(idx, res, mods, win, sc, columns):
                n = int(r['count']); p = float(r['log_p']) if n or r['log_p'] != 0 else 0
                row = (n, float(r['score_prefix']), float(r['score_suffix']), p, int(r['offset']), int(r['ticks']), m)
                yield i, Detected(row, *values), w, s

    def candidates(self, targets=None):
        """[(target_name, strand)] of a scan: every target added (or the named ones), in add_target order, '+' before '-'."""
        names = list(self.targets) if targets is None else list(targets)
        for t in names:
            if t not in self.targets:
                raise ValueError("RepeatCounter: Target with name " + str(t) + " not defined.")
        return [(t, s) for t in names for s in '+-']

    def scan_batch(self, signals, targets=None, min_score=None, units=False, scores=False):
        """Which target and strand each read spans, and detect()'s row for it -- no alignment of basecalls needed.

        signals: iterable of raw signals.  Every read is compared with every candidate of `candidates(targets)` on the two
        normalised flank scores detect() reports (strique_amd.scan.select states the rule); min_score: the smallest
        min(score_prefix, score_suffix) a candidate needs.  It has no default (ValueError when None): the scores of wrong and
        of true candidates overlap on noisy reads ("Scan"), so the threshold is the caller's decision.
        Returns, per read, None (no candidate eligible) or (target_name, strand, row), row being the tuple detect() returns
        for that target and strand -- (row, unit positions) with units=True.  scores=True: (that list, float64 array
        [n_reads, n_candidates, 2] of score_prefix, score_suffix of every candidate)."""
        if self.renorm is not None:
            raise ValueError("RepeatCounter: renorm is not available in a scan (set_renorm(None) first).")
        if self.tracts:
            raise ValueError("RepeatCounter: tracts are not available in a scan (set_tracts(False) first).")
        if self.motifs is not None:
            raise ValueError("RepeatCounter: motifs are not available in a scan (set_motifs(False) first).")
        if min_score is None:
            raise ValueError("RepeatCounter: scan_batch needs min_score (there is no default: see README, 'Scan').")
        if not min_score > 0:
            raise ValueError("RepeatCounter: min_score must be above 0.")
        cands = self.candidates(targets)
        if not cands:
            raise ValueError("RepeatCounter: no targets to scan for.")
        ids = [self._classifier_for(t, s).target_id for t, s in cands]
        reads = [(None, r) for r in signals]
        out = [None] * len(reads)
        all_scores = np.zeros((len(reads), len(cands), 2), np.float64)
        for i, d, w, sc in self._run(reads, {'units': True} if units else {}, scan=(ids, min_score)):
            all_scores[i] = sc
            if w >= 0:
                out[i] = cands[int(w)] + ((d.row, d.units) if units else d.row,)
        return (out, all_scores) if scores else out

    @staticmethod
    def _fits_int16(s):
        """DAC samples that fit int16 (see detect_batch)."""
        if s.dtype.kind not in 'iu':
            return False
        if s.dtype in (np.int8, np.uint8, np.int16):
            return True
        return s.size == 0 or (int(s.min()) >= -32768 and int(s.max()) <= 32767)

    def detect(self, target_name, raw_signal, strand, units=False, confidence=False, mod_llr=False, anchored=None, records=False):
        """(n, score_prefix, score_suffix, log_p, offset, ticks, mod_pattern) -- STRique.py:581-618.  units=True:
        (that tuple, unit positions or None); confidence=True: (that tuple, [positions,] (log_lik, count_mean, count_sd) or
        None); mod_llr=True: the per-unit log-likelihood ratios (or None) after them; anchored=m: (kind, count, log_p, begin, end,
        free_samples) of a read that holds one flank only (or None) behind them; after set_variants(True): (count_v, pattern, branch, end, V)
        or None last; records=True: a Detected record instead -- see detect_batch."""
        return self.detect_batch([(target_name, raw_signal, strand)], units=units, confidence=confidence, mod_llr=mod_llr, anchored=anchored,
                                 records=records)[0]
