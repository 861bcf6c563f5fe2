"""Profile-HMM topologies of the repeat counter and their 'baked' array form.

Host-side mirror of the reference's HMM classes (scripts/STRique.py:201-500): `profileHMM`,
`repeatHMM`, `flankedRepeatHMM`, `repeatModHMM`.  The reference builds pomegranate objects; here
the same states / transitions are written into a plain `Graph`, and `bake()` restates what
pomegranate 0.10.0's `HiddenMarkovModel.bake(merge='All')` (requirements.txt:11, called at
STRique.py:431,490) does to such a graph before `viterbi()` can run on it:

  1. states without in-edges (except start) or without out-edges (except end) are dropped,
     repeatedly -- this removes the unused start/end nodes of every embedded sub-model;
  2. every state whose out-edge probabilities do not sum to 1 (rounded to 8 decimals) is
     re-weighted in log space: logp -= log(round(sum, 8));
  3. silent states with a single certain (p == 1) out-edge are spliced out (also in front of the
     model end: adding log(1) = 0.0 is exact, so no path value changes);
  4. emitting states first, sorted by name; silent states after them in topological order.

The arrays go to the GPU through the C ABI (strq_model_create) and to the CPU oracle in tests.
pomegranate itself is not available in this image: SURVEY.md A.4 marks these semantics
"[recalled]"; the pre-bake topology is pinned by tests/golden/hmm_topology.json, which was
recorded from the reference's own classes.
"""
import math
from collections import namedtuple

import numpy as np

SQRT_2_PI = 2.50662827463      # the constant pomegranate's NormalDistribution uses

SILENT, NORMAL, UNIFORM = 0, 1, 2


class Graph(object):
    """States and transitions, nothing else."""

    def __init__(self):
        self.names, self.kinds, self.params = [], [], []
        self.edges = []                       # (src, dst, probability)
        self.layout = {}                      # optional: state -> (slot, lane) placement hint for the GPU kernel
        self.positions = {}                   # optional: emitting state -> (0 match-type | 1 insert-type, position along the profile chain)
        self.start = self.add_state("start", SILENT)
        self.end = self.add_state("end", SILENT)

    def add_state(self, name, kind, params=()):
        self.names.append(name); self.kinds.append(kind); self.params.append(tuple(float(p) for p in params))
        return len(self.names) - 1

    def add_transition(self, a, b, probability):
        self.edges.append((a, b, float(probability)))


PROFILE_DEFAULTS = {            # STRique.py:214-227
    'match_loop': .75, 'match_match': .15, 'match_insert': .09, 'match_delete': .01,
    'insert_loop': .15, 'insert_match_0': .40, 'insert_match_1': .40, 'insert_delete': .05,
    'delete_delete': .005, 'delete_insert': .05, 'delete_match': .945,
}

Profile = namedtuple("Profile", "s1 s2 e1 e2 match insert delete")


def _layer(defaults, overrides):
    tp = dict(defaults)
    if overrides:
        tp.update(overrides)
    return tp


def add_profile(g, sequence, pm, transition_probs=None, state_prefix='', no_silent=False,
                std_scale=1.0, std_offset=0.0):
    """One match/insert/delete column per k-mer of `sequence` (STRique.py:201-300)."""
    tp = _layer(PROFILE_DEFAULTS, transition_probs)
    k = pm.kmer
    n = len(sequence) - k + 1
    digits = int(np.ceil(np.log10(n)))
    match, insert, delete = [], [], []
    for idx in range(n):
        name = state_prefix + str(idx).rjust(digits, '0')
        mean, stdv = pm.model_dict[sequence[idx:idx + k]]
        match.append(g.add_state(name + 'm', NORMAL, (mean, stdv * std_scale + std_offset)))
        if not no_silent:
            delete.append(g.add_state(name + 'd', SILENT))
        insert.append(g.add_state(name + 'i', UNIFORM, (pm.model_min, pm.model_max)))
    s1 = g.add_state(state_prefix + 's1', SILENT); s2 = g.add_state(state_prefix + 's2', SILENT)
    e1 = g.add_state(state_prefix + 'e1', SILENT); e2 = g.add_state(state_prefix + 'e2', SILENT)
    last = n - 1
    for i in range(n):
        g.add_transition(match[i], match[i], tp['match_loop'])
        if i < last:
            g.add_transition(match[i], match[i + 1], tp['match_match'])
    for i in range(n):
        g.add_transition(insert[i], insert[i], tp['insert_loop'])
        g.add_transition(match[i], insert[i], tp['match_insert'])
        g.add_transition(insert[i], match[i], tp['insert_match_1'])
        if not no_silent and i < last:
            g.add_transition(insert[i], delete[i + 1], tp['insert_delete'])
        if i < last:
            g.add_transition(insert[i], match[i + 1], tp['insert_match_0'])
    if not no_silent:
        for i in range(n):
            g.add_transition(delete[i], insert[i], tp['delete_insert'])
            if i > 0:
                g.add_transition(match[i - 1], delete[i], tp['match_delete'])
            if i < last:
                g.add_transition(delete[i], match[i + 1], tp['delete_match'])
                g.add_transition(delete[i], delete[i + 1], tp['delete_delete'])
        g.add_transition(s1, delete[0], 1)
        g.add_transition(s2, match[0], 1)
        g.add_transition(delete[last], e1, tp['delete_delete'])
        g.add_transition(delete[last], e2, tp['delete_match'])
    else:
        for i in range(n - 2):
            g.add_transition(match[i], match[i + 2], tp['match_delete'])   # skip edge instead of a delete state
        g.add_transition(s1, insert[0], 1)
        g.add_transition(s2, match[0], 1)
    g.add_transition(insert[last], e1, tp['insert_delete'])
    g.add_transition(insert[last], e2, tp['insert_match_0'])
    g.add_transition(match[last], e2, tp['match_match'])
    g.add_transition(match[last], e1, tp['match_delete'])
    return Profile(s1, s2, e1, e2, match, insert, delete)


def extend_repeat(repeat, kmer):
    """Repeat unit padded so that it yields every k-mer of the tandem array, and the number of
    whole extra units that padding contains (STRique.py:328-335)."""
    if len(repeat) >= kmer:
        return repeat + repeat[:kmer - 1], 0
    ext = kmer - 1 + (len(repeat) - 1) - ((kmer - 1) % len(repeat))
    seq = repeat + (repeat * kmer)[:ext]
    return seq, int(len(seq) / len(repeat)) - 1


Repeat = namedtuple("Repeat", "s1 s2 e1 e2 d1 d2 profile repeat_offset")


def add_repeat(g, repeat, pm, transition_probs=None, state_prefix='', std_scale=1.0, std_offset=0.0):
    """One repeat unit closed into a loop through two emitting 'dummy' states (STRique.py:313-354)."""
    tp = _layer({'skip': .999, 'leave_repeat': .002}, transition_probs)
    seq, repeat_offset = extend_repeat(repeat, pm.kmer)
    prof = add_profile(g, seq, pm, tp, state_prefix, no_silent=True, std_scale=std_scale, std_offset=std_offset)
    d1 = g.add_state(state_prefix + 'dummy1', UNIFORM, (pm.model_min, pm.model_max))
    d2 = g.add_state(state_prefix + 'dummy2', UNIFORM, (pm.model_min, pm.model_max))
    e1 = g.add_state(state_prefix + 'e1', SILENT)
    e2 = g.add_state(state_prefix + 'e2', SILENT)
    g.add_transition(prof.e1, d1, 1)
    g.add_transition(prof.e2, d2, 1)
    g.add_transition(d1, e1, tp['leave_repeat'])
    g.add_transition(d2, e2, tp['leave_repeat'])
    g.add_transition(d1, prof.s1, 1 - tp['leave_repeat'])
    g.add_transition(d2, prof.s2, 1 - tp['leave_repeat'])
    return Repeat(prof.s1, prof.s2, e1, e2, d1, d2, prof, repeat_offset)


class FlankedRepeatModel(object):
    """prefix profile -> repeat loop -> suffix profile (STRique.py:384-431)."""

    def __init__(self, repeat, prefix, suffix, pm, config=None):
        tp = _layer({'skip': 1 - 1e-4, 'seq_std_scale': 1.0, 'rep_std_scale': 1.0,
                     'seq_std_offset': 0.0, 'rep_std_offset': 0.0, 'e1_ratio': 0.1},
                    config if isinstance(config, dict) else None)
        units = int(np.ceil(pm.kmer / len(repeat)))
        prefix_seq = prefix + (repeat * units)[:-1]
        suffix_seq = repeat * units + suffix
        self.flanking_count = units * 2 - 1
        g = Graph()
        pre = add_profile(g, prefix_seq, pm, tp, 'prefix', std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset'])
        suf = add_profile(g, suffix_seq, pm, tp, 'suffix', std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset'])
        rep = add_repeat(g, repeat, pm, tp, 'repeat', std_scale=tp['rep_std_scale'], std_offset=tp['rep_std_offset'])
        g.add_transition(g.start, pre.s1, tp['e1_ratio'])
        g.add_transition(g.start, pre.s2, 1 - tp['e1_ratio'])
        g.add_transition(pre.e1, rep.s1, 1)
        g.add_transition(pre.e2, rep.s2, 1)
        g.add_transition(rep.e1, suf.s1, 1)
        g.add_transition(rep.e2, suf.s2, 1)
        g.add_transition(suf.e1, g.end, 1)
        g.add_transition(suf.e2, g.end, 1)
        # placement hint for the Viterbi kernel: one slot per column type, lane = profile position, the
        # repeat unit right behind the prefix (its natural neighbour)
        # busy states (matches, the repeat unit) in the first two slots, plain inserts in the last two:
        # the kernel keeps 6 in-edge registers for the former and 3 for the latter
        lay = {}
        for p_, st in enumerate(pre.match): lay[st] = (0, p_)
        for p_, st in enumerate(suf.match): lay[st] = (1, p_)
        for p_, st in enumerate(pre.insert): lay[st] = (2, p_)
        for p_, st in enumerate(suf.insert): lay[st] = (3, p_)
        b0, b1 = len(pre.match), len(suf.match)
        for q_, st in enumerate(rep.profile.match): lay[st] = (0, b0 + q_)
        for q_, st in enumerate(rep.profile.insert): lay[st] = (1, b1 + q_)
        lay[rep.d2] = (0, b0 + len(rep.profile.match)); lay[rep.d1] = (1, b1 + len(rep.profile.insert))
        if max(l for _, l in lay.values()) < 64:
            g.layout = lay
        # the same states as one chain of positions: prefix profile, repeat unit, the two dummy states (match-type dummy2,
        # insert-type dummy1: they feed suffix00m / suffix00d the way a match / insert feeds the next position), suffix profile
        pos = {}
        P, R = len(pre.match), len(rep.profile.match)
        for p_, st in enumerate(pre.match): pos[st] = (0, p_)
        for p_, st in enumerate(pre.insert): pos[st] = (1, p_)
        for q_, st in enumerate(rep.profile.match): pos[st] = (0, P + q_)
        for q_, st in enumerate(rep.profile.insert): pos[st] = (1, P + q_)
        pos[rep.d2] = (0, P + R); pos[rep.d1] = (1, P + R)
        for p_, st in enumerate(suf.match): pos[st] = (0, P + R + 1 + p_)
        for p_, st in enumerate(suf.insert): pos[st] = (1, P + R + 1 + p_)
        g.positions = pos
        self.graph = g
        self.repeat_offset = rep.repeat_offset
        # visits of the two dummy states count repeat units (STRique.py:374-378)
        self.count_states = (rep.d1, rep.d2)
        self.count_bias = self.flanking_count - self.repeat_offset
        self.baked = bake(g, count_states=self.count_states, tag_substring='repeat')
        # what every emitting state stands for (state_kmers): section, column type and, for a match state, the k-mer of its column
        k = pm.kmer
        rep_seq = extend_repeat(repeat, k)[0]
        what = {rep.d1: ('repeat', 'dummy', None), rep.d2: ('repeat', 'dummy', None)}
        for section, prof, seq in (('prefix', pre, prefix_seq), ('repeat', rep.profile, rep_seq), ('suffix', suf, suffix_seq)):
            for c_, st in enumerate(prof.match): what[st] = (section, 'match', seq[c_:c_ + k])
            for st in prof.insert: what[st] = (section, 'insert', None)
        self._state_what = what

    def state_kmers(self):
        """Per emitting state in baked order (state s of a decode path, s < baked.silent_start): (section, kind, kmer) -- section
        'prefix' | 'repeat' | 'suffix', kind 'match' | 'insert' | 'dummy', kmer the k-mer of a match state's column (prefix_seq[c:c+k],
        the extend_repeat sequence for the loop, suffix_seq[c:c+k]) and None otherwise.  The sequences are the model's own: a model
        built for the - strand carries the k-mers of the reverse-complemented locus."""
        return [self._state_what[int(o)] for o in self.baked.orig_index[:self.baked.silent_start]]


class CompoundRepeatModel(object):
    """prefix profile -> loop tract0 -> junction0 profile -> loop tract1 [-> junction1 -> tract2] -> suffix profile: the flanked
    model with K = 2 or 3 repeat loops in a fixed order (strique_amd.tracts states the rule and the sequences of the sections).
    `units`, `linkers`, `prefix`, `suffix` as the strand reads them (tracts.strand_definition).  Loops take the rep_std_*
    parameters, profiles -- the junctions too, with their delete states -- the seq_std_* ones; the sections are joined e1 -> s1,
    e2 -> s2 with probability 1 and start is wired as in FlankedRepeatModel.  `tract_of[state]` is the tract whose two dummy
    states the baked state is one of (else -1), `count_bias[j]` what turns the visits of tract j into its count."""

    def __init__(self, units, linkers, prefix, suffix, pm, config=None):
        from . import tracts
        tp = _layer({'skip': 1 - 1e-4, 'seq_std_scale': 1.0, 'rep_std_scale': 1.0,
                     'seq_std_offset': 0.0, 'rep_std_offset': 0.0, 'e1_ratio': 0.1},
                    config if isinstance(config, dict) else None)
        self.units, self.linkers = tracts.check(units, linkers)
        g = Graph()
        parts, loops, profiles = [], [], []
        for what, name, seq in tracts.sections(self.units, self.linkers, prefix, suffix, pm.kmer):
            if what == 'loop':
                parts.append(add_repeat(g, seq, pm, tp, name, std_scale=tp['rep_std_scale'], std_offset=tp['rep_std_offset']))
                loops.append(parts[-1])
            else:
                parts.append(add_profile(g, seq, pm, tp, name, std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset']))
                profiles.append(parts[-1])
        g.add_transition(g.start, parts[0].s1, tp['e1_ratio'])
        g.add_transition(g.start, parts[0].s2, 1 - tp['e1_ratio'])
        for a, b in zip(parts, parts[1:]):
            g.add_transition(a.e1, b.s1, 1)
            g.add_transition(a.e2, b.s2, 1)
        g.add_transition(parts[-1].e1, g.end, 1)
        g.add_transition(parts[-1].e2, g.end, 1)
        # placement hint for the lane kernels, in the spirit of the flanked model's: the states with many in-edges -- the matches
        # and the first insert of every loop, which the spliced hubs feed -- fill the first two slots in model order, the states
        # with uniform emissions and at most three in-edges (the other inserts, the dummy states) the last two -- where they fit.
        # The loops go first: their first match and insert are the states with six in-edges, which the packed kernel shapes want
        # in the first slot
        busy, flat = [], []
        for p in parts:
            if isinstance(p, Repeat):
                busy += p.profile.match + p.profile.insert[:1]
                flat += p.profile.insert[1:] + [p.d1, p.d2]
        for p in parts:
            if not isinstance(p, Repeat):
                busy += p.match; flat += p.insert
        if len(busy) <= 128 and len(flat) <= 128:
            lay = {}
            for i, st in enumerate(busy): lay[st] = (i // 64, i % 64)
            for i, st in enumerate(flat): lay[st] = (2 + i // 64, i % 64)
            g.layout = lay
        self.graph = g
        self.repeat_offset = tuple(l.repeat_offset for l in loops)
        self.count_states = tuple((l.d1, l.d2) for l in loops)
        self.count_bias = tuple(2 * tracts.flank_units(u, pm.kmer) - 1 - l.repeat_offset for u, l in zip(self.units, loops))
        self.n_tracts = len(loops)
        self.baked = bake(g, count_states=[s for pair in self.count_states for s in pair], tag_substring='tract')
        new = {int(old): k for k, old in enumerate(self.baked.orig_index)}
        self.tract_of = np.full(self.baked.n_states, -1, np.int32)
        for j, pair in enumerate(self.count_states):
            for s in pair:
                self.tract_of[new[s]] = j


ANCHORED_KINDS = ('ends_in_repeat', 'starts_in_repeat')


class AnchoredRepeatModel(object):
    """FlankedRepeatModel with one flank profile replaced by a single emitting free state, for a read that holds one flank only
    (strique_amd/anchored.py states which reads those are):

      ends_in_repeat    prefix profile -> repeat loop -> `tail` -> end      the read breaks off inside the array
      starts_in_repeat  start -> `head` -> repeat loop -> suffix profile    the read starts inside it

    `tail` / `head` emit uniformly over the pore model's range, stay with `free_loop` and emit at least one observation, so that
    the end state keeps its single kind of in-edge and no state gains an in-edge over the flanked model.  The topology forces
    one pass through the loop (a read cut one base into the array decodes one visit), hence the -1 in `count_bias`."""

    def __init__(self, kind, repeat, prefix, suffix, pm, config=None):
        if kind not in ANCHORED_KINDS:
            raise ValueError("AnchoredRepeatModel: kind must be one of %s" % (ANCHORED_KINDS,))
        tp = _layer({'skip': 1 - 1e-4, 'seq_std_scale': 1.0, 'rep_std_scale': 1.0,
                     'seq_std_offset': 0.0, 'rep_std_offset': 0.0, 'e1_ratio': 0.1, 'free_loop': 0.999},
                    config if isinstance(config, dict) else None)
        units = int(np.ceil(pm.kmer / len(repeat)))
        self.kind = kind
        g = Graph()
        lay, pos = {}, {}
        if kind == 'ends_in_repeat':
            pre = add_profile(g, prefix + (repeat * units)[:-1], pm, tp, 'prefix', std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset'])
            rep = add_repeat(g, repeat, pm, tp, 'repeat', std_scale=tp['rep_std_scale'], std_offset=tp['rep_std_offset'])
            free = g.add_state('tail', UNIFORM, (pm.model_min, pm.model_max))
            g.add_transition(g.start, pre.s1, tp['e1_ratio'])
            g.add_transition(g.start, pre.s2, 1 - tp['e1_ratio'])
            g.add_transition(pre.e1, rep.s1, 1)
            g.add_transition(pre.e2, rep.s2, 1)
            g.add_transition(rep.e1, free, 1)
            g.add_transition(rep.e2, free, 1)
            g.add_transition(free, free, tp['free_loop'])
            g.add_transition(free, g.end, 1 - tp['free_loop'])
            # two slots: match-type states, insert-type states; lane = position along the chain.  The free state takes the next lane
            # of the first slot, or -- where the flanked model's layout fills all 64 lanes -- the first lane of a third slot (the model
            # then has 129 emitting states, i.e. three slots): whenever the flanked model has a layout, so has this one
            P, R = len(pre.match), len(rep.profile.match)
            for p_, st in enumerate(pre.match): lay[st] = (0, p_); pos[st] = (0, p_)
            for p_, st in enumerate(pre.insert): lay[st] = (1, p_); pos[st] = (1, p_)
            for q_, st in enumerate(rep.profile.match): lay[st] = (0, P + q_); pos[st] = (0, P + q_)
            for q_, st in enumerate(rep.profile.insert): lay[st] = (1, P + q_); pos[st] = (1, P + q_)
            lay[rep.d2] = (0, P + R); lay[rep.d1] = (1, P + R); lay[free] = (0, P + R + 1) if P + R + 1 < 64 else (2, 0)
            pos[rep.d2] = (0, P + R); pos[rep.d1] = (1, P + R); pos[free] = (0, P + R + 1)
            bias = -units - 1
        else:
            free = g.add_state('head', UNIFORM, (pm.model_min, pm.model_max))
            rep = add_repeat(g, repeat, pm, tp, 'repeat', std_scale=tp['rep_std_scale'], std_offset=tp['rep_std_offset'])
            suf = add_profile(g, repeat * units + suffix, pm, tp, 'suffix', std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset'])
            g.add_transition(g.start, free, 1)
            g.add_transition(free, free, tp['free_loop'])
            g.add_transition(free, rep.s1, (1 - tp['free_loop']) * tp['e1_ratio'])
            g.add_transition(free, rep.s2, (1 - tp['free_loop']) * (1 - tp['e1_ratio']))
            g.add_transition(rep.e1, suf.s1, 1)
            g.add_transition(rep.e2, suf.s2, 1)
            g.add_transition(suf.e1, g.end, 1)
            g.add_transition(suf.e2, g.end, 1)
            # the same two slots, the free state behind the suffix matches (or in a third slot, as above); along the chain it stands
            # in front of the unit
            R, S = len(rep.profile.match), len(suf.match)
            pos[free] = (0, 0)
            for q_, st in enumerate(rep.profile.match): lay[st] = (0, q_); pos[st] = (0, 1 + q_)
            for q_, st in enumerate(rep.profile.insert): lay[st] = (1, q_); pos[st] = (1, 1 + q_)
            lay[rep.d2] = (0, R); lay[rep.d1] = (1, R)
            pos[rep.d2] = (0, 1 + R); pos[rep.d1] = (1, 1 + R)
            for p_, st in enumerate(suf.match): lay[st] = (0, 1 + R + p_); pos[st] = (0, 2 + R + p_)
            for p_, st in enumerate(suf.insert): lay[st] = (1, 1 + R + p_); pos[st] = (1, 2 + R + p_)
            lay[free] = (0, 1 + R + S) if 1 + R + S < 64 else (2, 0)
            bias = -1
        if max(l for _, l in lay.values()) < 64:
            g.layout = lay
        g.positions = pos
        self.graph = g
        self.free_state = free
        self.repeat_offset = rep.repeat_offset
        self.count_states = (rep.d1, rep.d2)
        # the flanked model's bias (flanking units - units the padded repeat profile holds), less the units of the flank profile
        # that is gone (ends_in_repeat: the suffix profile starts with `units` of them), less the forced pass through the loop
        self.count_bias = (units * 2 - 1) - rep.repeat_offset + bias
        self.baked = bake(g, count_states=self.count_states, tag_substring='repeat')


class RepeatModModel(object):
    """Unmodified and modified repeat-unit profiles side by side between two emitting hub states
    (STRique.py:447-490)."""

    def __init__(self, repeat, pm_base, pm_mod, config=None):
        tp = _layer({'rep_std_scale': 1.5, 'rep_std_offset': 0.0, 'leave_repeat': .002},
                    config if isinstance(config, dict) else None)
        seq, _ = extend_repeat(repeat, pm_base.kmer)
        self.model_min = min(pm_base.model_min, pm_mod.model_min)
        self.model_max = max(pm_base.model_max, pm_mod.model_max)
        g = Graph()
        s0 = g.add_state('s0', UNIFORM, (self.model_min, self.model_max))
        e0 = g.add_state('e0', UNIFORM, (self.model_min, self.model_max))
        base = add_profile(g, seq, pm_base, tp, 'base', no_silent=True, std_scale=tp['rep_std_scale'],
                           std_offset=tp['rep_std_offset'])
        mod = add_profile(g, seq, pm_mod, tp, 'mod', no_silent=True,
                          std_scale=tp['rep_std_scale'] * pm_mod.scale2stdv(pm_base),
                          std_offset=tp['rep_std_offset'])
        g.add_transition(g.start, s0, 1)
        for p in (base, mod):
            g.add_transition(s0, p.s1, 0.25)
            g.add_transition(s0, p.s2, 0.25)
        for p in (base, mod):
            g.add_transition(p.e1, e0, 1)
            g.add_transition(p.e2, e0, 1)
        g.add_transition(e0, g.end, tp['leave_repeat'])
        g.add_transition(e0, s0, 1 - tp['leave_repeat'])
        lay = {}
        lane = 0
        for group in (base.match, base.insert, mod.match, mod.insert, [s0, e0]):
            for st in group:
                lay[st] = (0, lane); lane += 1
        if lane <= 64:
            g.layout = lay
        self.graph = g
        self.hub_states = (s0, e0)
        # tag 2 = hub states s0/e0 (group separators of mod_repeats, STRique.py:496), 1 = modified branch
        self.baked = bake(g, count_states=(), tag_substring='mod', tag2_states=(s0, e0))


class FlankProfileModel(object):
    """One flank profile on its own, for the segmentation of a flank stretch (strique_amd/flank_mod.py states the rule):
    start -> (e1_ratio) s1 | s2 -> profile of `flank` with the seq_std_* parameters -> end, i.e. the flanked model's prefix
    section alone.  `column_of[state]` is the profile column of a baked match or insert state, -1 for every other state."""

    def __init__(self, flank, pm, config=None):
        tp = _layer({'skip': 1 - 1e-4, 'seq_std_scale': 1.0, 'seq_std_offset': 0.0, 'e1_ratio': 0.1},
                    config if isinstance(config, dict) else None)
        g = Graph()
        prof = add_profile(g, flank, pm, tp, 'flank', std_scale=tp['seq_std_scale'], std_offset=tp['seq_std_offset'])
        g.add_transition(g.start, prof.s1, tp['e1_ratio'])
        g.add_transition(g.start, prof.s2, 1 - tp['e1_ratio'])
        g.add_transition(prof.e1, g.end, 1)
        g.add_transition(prof.e2, g.end, 1)
        # two slots where the columns fit the lanes (match-type, insert-type; lane = column); a longer flank takes whatever
        # kernel shape holds its states.  The same states as a chain of positions
        pos = {}
        for p_, st in enumerate(prof.match): pos[st] = (0, p_)
        for p_, st in enumerate(prof.insert): pos[st] = (1, p_)
        g.positions = pos
        if len(prof.match) <= 64:
            g.layout = dict(pos)          # (slot, lane) = (kind, column)
        self.graph = g
        self.n_columns = len(prof.match)
        self.baked = bake(g)
        new = {int(old): k for k, old in enumerate(self.baked.orig_index)}
        self.column_of = np.full(self.baked.n_states, -1, np.int32)
        for p_, (m_, i_) in enumerate(zip(prof.match, prof.insert)):
            self.column_of[new[m_]] = p_
            self.column_of[new[i_]] = p_


class SiteModModel(object):
    """RepeatModModel over a linear sequence -- the bases the columns of one CpG group of a flank spell -- passed once: the same
    topology, tags, std scaling and layout hint, but no extend_repeat, no e0 -> s0 edge, and e0 -> end with probability 1."""

    def __init__(self, sequence, pm_base, pm_mod, config=None):
        tp = _layer({'rep_std_scale': 1.5, 'rep_std_offset': 0.0},
                    config if isinstance(config, dict) else None)
        self.model_min = min(pm_base.model_min, pm_mod.model_min)
        self.model_max = max(pm_base.model_max, pm_mod.model_max)
        g = Graph()
        s0 = g.add_state('s0', UNIFORM, (self.model_min, self.model_max))
        e0 = g.add_state('e0', UNIFORM, (self.model_min, self.model_max))
        base = add_profile(g, sequence, pm_base, tp, 'base', no_silent=True, std_scale=tp['rep_std_scale'],
                           std_offset=tp['rep_std_offset'])
        mod = add_profile(g, sequence, pm_mod, tp, 'mod', no_silent=True,
                          std_scale=tp['rep_std_scale'] * pm_mod.scale2stdv(pm_base),
                          std_offset=tp['rep_std_offset'])
        g.add_transition(g.start, s0, 1)
        for p in (base, mod):
            g.add_transition(s0, p.s1, 0.25)
            g.add_transition(s0, p.s2, 0.25)
        for p in (base, mod):
            g.add_transition(p.e1, e0, 1)
            g.add_transition(p.e2, e0, 1)
        g.add_transition(e0, g.end, 1)
        lay = {}
        lane = 0
        for group in (base.match, base.insert, mod.match, mod.insert, [s0, e0]):
            for st in group:
                lay[st] = (0, lane); lane += 1
        if lane <= 64:
            g.layout = lay
        self.graph = g
        self.hub_states = (s0, e0)
        self.n_columns = len(base.match)
        self.baked = bake(g, count_states=(), tag_substring='mod', tag2_states=(s0, e0))


VARIANT_TAGS = (1, 3, 4)        # state tag of alt branch 1 / 2 / 3 (0 base, 2 hub: as the dual model of RepeatModModel)


def check_alt_units(repeat, alt_units):
    """The alt units of a variant model, upper-cased: 1 to 3 units over ACGT, as long as `repeat`, each different from it and from
    the others.  ValueError names the unit that is not."""
    repeat = repeat.upper()
    if isinstance(alt_units, str):
        alt_units = [alt_units]
    alts = [str(a).upper() for a in alt_units]
    if not 1 <= len(alts) <= len(VARIANT_TAGS):
        raise ValueError("alt units: between 1 and %d units per target, got %d (%s)" % (len(VARIANT_TAGS), len(alts), ",".join(alts)))
    for i, a in enumerate(alts):
        if not a or set(a) - set("ACGT"):
            raise ValueError("alt unit %r: only the letters A, C, G, T" % a)
        if len(a) != len(repeat):
            raise ValueError("alt unit %r: %d nt, the repeat unit %s has %d" % (a, len(a), repeat, len(repeat)))
        if a == repeat:
            raise ValueError("alt unit %r is the repeat unit itself" % a)
        if a in alts[:i]:
            raise ValueError("alt unit %r is given twice" % a)
    return alts


def variant_context_units(repeat, kmer):
    """m: the units in front of an alt unit whose k-mers reach into it."""
    return -(-(kmer - 1) // len(repeat))


class RepeatVariantModel(object):
    """The repeat-unit profile and one profile per alt unit side by side between two emitting hub states: the topology of
    RepeatModModel with up to four branches over one pore model.  Branch b >= 1 holds the k-mers of repeat * m + alt_b that start in
    the m context units in front of the alt unit and in the alt unit itself (m = variant_context_units), so one passage through it
    covers m + 1 units of signal.  HMM-config key `variant_prior` = p: every alt branch is entered with p, the base branch with
    1 - (NB - 1) p; without it all NB branches alike."""

    def __init__(self, repeat, alt_units, pm, config=None):
        tp = _layer({'rep_std_scale': 1.5, 'rep_std_offset': 0.0, 'leave_repeat': .002, 'variant_prior': None},
                    config if isinstance(config, dict) else None)
        repeat = repeat.upper()
        self.alt_units = check_alt_units(repeat, alt_units)
        K, L = pm.kmer, len(repeat)
        m = self.context_units = variant_context_units(repeat, K)
        NB = self.n_branches = 1 + len(self.alt_units)
        self.model_min, self.model_max = pm.model_min, pm.model_max
        g = Graph()
        s0 = g.add_state('s0', UNIFORM, (pm.model_min, pm.model_max))
        e0 = g.add_state('e0', UNIFORM, (pm.model_min, pm.model_max))
        kw = dict(no_silent=True, std_scale=tp['rep_std_scale'], std_offset=tp['rep_std_offset'])
        profiles = [add_profile(g, extend_repeat(repeat, K)[0], pm, tp, 'base', **kw)]
        for b, alt in enumerate(self.alt_units, 1):
            profiles.append(add_profile(g, (repeat * m + alt + repeat * K)[:(m + 1) * L + K - 1], pm, tp, 'alt%d' % b, **kw))
        p_alt = tp['variant_prior']
        if p_alt is None:
            prior = [1.0 / NB] * NB
        else:
            if not 0.0 < p_alt * (NB - 1) < 1.0:
                raise ValueError("variant_prior %r: the %d alt branches must leave the base branch a probability above 0" % (p_alt, NB - 1))
            prior = [1.0 - (NB - 1) * p_alt] + [p_alt] * (NB - 1)
        g.add_transition(g.start, s0, 1)
        for p, pr in zip(profiles, prior):
            g.add_transition(s0, p.s1, pr / 2)
            g.add_transition(s0, p.s2, pr / 2)
        for p in profiles:
            g.add_transition(p.e1, e0, 1)
            g.add_transition(p.e2, e0, 1)
        g.add_transition(e0, g.end, tp['leave_repeat'])
        g.add_transition(e0, s0, 1 - tp['leave_repeat'])
        lay = {}
        lane = 0
        for group in [q for p in profiles for q in (p.match, p.insert)] + [[s0, e0]]:
            for st in group:
                lay[st] = (0, lane); lane += 1
        if lane <= 64:
            g.layout = lay
        self.graph = g
        self.hub_states = (s0, e0)
        extra = {}
        for b, p in enumerate(profiles[1:]):
            for st in p.match + p.insert:
                extra[st] = VARIANT_TAGS[b]
        self.baked = bake(g, count_states=(), tag2_states=(s0, e0), extra_tags=extra)


# ---------------------------------------------------------------------------------------------
BakedHMM = namedtuple("BakedHMM", [
    "n_states", "silent_start", "start", "end",
    "in_ptr", "in_src", "in_logp",          # CSR of in-edges, sources ascending inside a state
    "emis_kind", "emis_a", "emis_b", "emis_c",
    "count_inc",                            # 1 for states whose visits are counted
    "tag",                                  # 1 for states whose name contains `tag_substring`
    "names", "orig_index",
    "hint_slot", "hint_lane",               # placement hints (-1 = none), see strq_model_create
    "pos_kind", "pos_index",                # position of every emitting state along the profile chain (None = unknown), see strq_model_set_positions
    "in_logp_sum",                          # per in-edge: log of the summed probability of the parallel edges it stands for (None = in_logp), see strq_model_set_forward_logp
], defaults=(None, None, None))


def bake(g, count_states=(), tag_substring=None, tag2_states=(), extra_tags=None):
    """`extra_tags`: state -> tag for states that are neither hubs (`tag2_states`) nor named after `tag_substring`."""
    n = len(g.names)
    alive = [True] * n
    edges = [(a, b, math.log(p) if p > 0 else -math.inf) for a, b, p in g.edges]
    # 1. orphans
    while True:
        indeg, outdeg = [0] * n, [0] * n
        for a, b, _ in edges:
            outdeg[a] += 1; indeg[b] += 1
        dead = [i for i in range(n) if alive[i] and
                ((indeg[i] == 0 and i != g.start) or (outdeg[i] == 0 and i != g.end))]
        if not dead:
            break
        for i in dead:
            alive[i] = False
        edges = [e for e in edges if alive[e[0]] and alive[e[1]]]
    # 2. out-edge normalisation in log space
    out = {}
    for idx, (a, b, lp) in enumerate(edges):
        out.setdefault(a, []).append(idx)
    for a, idxs in out.items():
        total = round(sum(math.e ** edges[i][2] for i in idxs), 8)
        if total != 1.0 and a != g.end:
            lt = math.log(total)
            for i in idxs:
                edges[i] = (edges[i][0], edges[i][1], edges[i][2] - lt)
    # 3. splice silent states with one certain out-edge
    while True:
        merged = 0
        out = {}
        for a, b, lp in edges:
            out.setdefault(a, []).append((b, lp))
        for a in range(n):
            if not alive[a] or g.kinds[a] != SILENT or a == g.start or a not in out:
                continue
            if len(out[a]) == 1 and out[a][0][1] == 0.0 and out[a][0][0] != a:
                b = out[a][0][0]
                edges = [(x, b if y == a else y, lp) for x, y, lp in edges if x != a]
                alive[a] = False
                merged += 1
                break
        if not merged:
            break
    # parallel edges (two spliced paths between the same pair of states, e.g. insert -> e1 -> e0
    # and insert -> e2 -> e0 in the modification model): Viterbi takes the better one, so keep a
    # single edge with the larger probability.  (pomegranate's networkx DiGraph would keep
    # whichever of the two it happened to re-insert last -- an order that depends on id() hashes
    # and differs between runs of the reference; see DESIGN.md "unpinned semantics".)
    # A sum over paths (the forward pass, strq_forward_batch) needs the summed probability of such a pair instead: kept per edge
    # beside the maximum, in the same order.
    best, mass, mult = {}, {}, {}
    for a, b, lp in edges:
        if (a, b) not in best or lp > best[(a, b)]:
            best[(a, b)] = lp
        mass[(a, b)] = mass.get((a, b), 0.0) + math.exp(lp)
        mult[(a, b)] = mult.get((a, b), 0) + 1
    total = {k: (math.log(mass[k]) if mult[k] > 1 else best[k]) for k in best}
    seen = set()
    dedup = []
    for a, b, lp in edges:
        if (a, b) not in seen:
            seen.add((a, b)); dedup.append((a, b, best[(a, b)]))
    edges = dedup
    # 4. ordering
    emitting = sorted((i for i in range(n) if alive[i] and g.kinds[i] != SILENT), key=lambda i: (g.names[i], i))
    silent = [i for i in range(n) if alive[i] and g.kinds[i] == SILENT]
    sil_set = set(silent)
    indeg = {i: 0 for i in silent}
    succ = {i: [] for i in silent}
    for a, b, _ in edges:
        if a in sil_set and b in sil_set:
            if a == b:
                raise ValueError("silent self loop")
            indeg[b] += 1; succ[a].append(b)
    ready = sorted((i for i in silent if indeg[i] == 0), key=lambda i: (g.names[i], i))
    order = []
    while ready:
        i = ready.pop(0)
        order.append(i)
        newly = []
        for b in succ[i]:
            indeg[b] -= 1
            if indeg[b] == 0:
                newly.append(b)
        ready = sorted(ready + newly, key=lambda i: (g.names[i], i))
    if len(order) != len(silent):
        raise ValueError("cycle of silent states")
    final = emitting + order
    new = {old: k for k, old in enumerate(final)}
    m = len(final)
    ins = [[] for _ in range(m)]
    for a, b, lp in edges:
        ins[new[b]].append((new[a], lp, total[(a, b)]))
    in_ptr = np.zeros(m + 1, np.int32)
    in_src, in_logp, in_logp_sum = [], [], []
    for k in range(m):
        ins[k].sort(key=lambda t: t[0])
        in_ptr[k + 1] = in_ptr[k] + len(ins[k])
        in_src += [t[0] for t in ins[k]]
        in_logp += [t[1] for t in ins[k]]
        in_logp_sum += [t[2] for t in ins[k]]
    ne = len(emitting)
    kind = np.zeros(ne, np.int32); ea = np.zeros(ne); eb = np.zeros(ne); ec = np.zeros(ne)
    for k, old in enumerate(emitting):
        kind[k] = g.kinds[old]
        p = g.params[old]
        if g.kinds[old] == NORMAL:
            mu, sigma = p
            ea[k] = mu
            eb[k] = 1.0 / (2 * sigma ** 2)
            ec[k] = -math.log(sigma * SQRT_2_PI)
        else:
            lo, hi = p
            ea[k], eb[k] = lo, hi
            ec[k] = -math.log(hi - lo)
    count_inc = np.zeros(m, np.int32)
    for s in count_states:
        count_inc[new[s]] = 1
    tag = np.array([2 if old in tag2_states else (1 if (tag_substring and tag_substring in g.names[old]) else 0)
                    for old in final], np.int32)
    for k, old in enumerate(final):
        if extra_tags and old in extra_tags:
            tag[k] = extra_tags[old]
    hint_slot = np.full(m, -1, np.int32); hint_lane = np.full(m, -1, np.int32)
    if g.layout and all(old in g.layout for old in emitting):
        for old in emitting:
            hint_slot[new[old]], hint_lane[new[old]] = g.layout[old]
    pos_kind = pos_index = None
    if getattr(g, 'positions', None) and all(old in g.positions for old in emitting):
        pos_kind = np.zeros(m, np.int32); pos_index = np.zeros(m, np.int32)
        for old in emitting:
            pos_kind[new[old]], pos_index[new[old]] = g.positions[old]
    return BakedHMM(m, ne, new[g.start], new[g.end], in_ptr, np.array(in_src, np.int32),
                    np.array(in_logp, np.float64), kind, ea, eb, ec, count_inc, tag,
                    [g.names[i] for i in final], np.array(final, np.int32), hint_slot, hint_lane, pos_kind, pos_index,
                    np.array(in_logp_sum, np.float64))
