"""Reference of the second normalisation step for the tests: the oracle's detect() (oracle/strique_oracle.py) restated with the three
'minmax' maps made explicit, so that strique_amd.renorm.apply can correct them between conditioning and everything behind it.  With
the rule left out (`Q` None) it is the oracle's detect() to the bit, which tests/test_renorm_host.py checks.  Also the reads the host
and the GPU tests share, built from sequences (inputs, not expectations), and what the reference makes of them, computed once per
process."""
import numpy as np

from oracle import strique_oracle as orc
from strique_amd import renorm


def minmax_maps(signal, pm):
    """((c1, h1), h2, c2) of PoreModel.normalize_minmax: out = (signal - c1) / h1 * h2 + c2."""
    signal = np.asarray(signal, dtype=np.float64)
    mv = pm.means
    with np.errstate(all='ignore'):
        q5_sig, q95_sig = np.percentile(signal, [1, 99])
        q5_mod, q95_mod = np.percentile(mv, [1, 99])
        lo_s, hi_s = signal[signal < q5_sig], signal[signal > q95_sig]
        m5_sig = np.median(lo_s) if len(lo_s) else np.nan
        m95_sig = np.median(hi_s) if len(hi_s) else np.nan
        m5_mod = np.median(mv[mv < q5_mod]); m95_mod = np.median(mv[mv > q95_mod])
    return (m5_sig + (m95_sig - m5_sig) / 2, (m95_sig - m5_sig) / 2), (m95_mod - m5_mod) / 2, m5_mod + (m95_mod - m5_mod) / 2


def normalize(signal, c1h1, h2, c2, pm):
    with np.errstate(all='ignore'):
        out = (np.asarray(signal, dtype=np.float64) - c1h1[0]) / c1h1[1]
        out = out * h2 + c2
    np.clip(out, pm.model_min + .5, pm.model_max - .5, out=out)
    return out


def kmer_stats(pm):
    return dict(pm.table)


def target_tables(pm, repeat, strand):
    r = repeat.upper()
    if strand == '-':
        r = orc.revcomp(r)
    return renorm.tables(kmer_stats(pm), pm.kmer, pm.model_min, pm.model_max, r)


def condition(raw_signal, pm, want_raw=False):
    """Steps 1-6 of detect with the maps made explicit: (maps, signals, status, med, mad)."""
    raw_signal = np.asarray(raw_signal)
    flt = orc.medfilt3(raw_signal)
    with np.errstate(all='ignore'):
        med = np.median(flt); mad = orc.mad(flt)
        z = (flt - med) / mad
        u8 = np.clip(np.nan_to_num(z * 24 + 127, nan=0.0), 0, 255).astype(np.uint8)
    u8 = orc.grey_open_close_1x8(u8)
    (m_map, h2, c2) = minmax_maps(u8, pm)
    f_map = minmax_maps(flt, pm)[0]
    maps = {'morph': m_map, 'filtered': f_map, 'h2': h2, 'c2': c2}
    signals = {'morph': u8, 'filtered': flt}
    if want_raw:
        maps['raw'] = minmax_maps(raw_signal, pm)[0]
        signals['raw'] = raw_signal
    ok = all(np.isfinite(maps[s][0]) and maps[s][1] > 0 and np.isfinite(maps[s][1]) for s in signals) and np.isfinite(med) and mad > 0
    return maps, signals, (0 if ok else 1), med, mad


def ref_fit(h, Q, A):
    """The fit restated with plain loops (for histograms of a few bins): (a, b, w, score) or None."""
    h = [int(v) for v in h]
    N = sum(h)
    if N == 0:
        return None
    nz = [(i, v) for i, v in enumerate(h) if v]

    def score(a, b, w):
        s = 0
        for i, v in nz:
            j = renorm.HALF + (a * (i - renorm.HALF)) // renorm.A_ONE + b
            s += v * (int(Q[w][j]) if 0 <= j < renorm.GRID else renorm.Q_OUT)
        return s + N * int(A[a])

    def best(a_list, b_list):
        top = None
        for a in a_list:
            for b in b_list:
                for w in range(renorm.N_W):
                    sc = score(a, b, w)
                    if top is None or sc > top[3]:          # ascending (a, b, w): the first maximum is the smallest
                        top = (a, b, w, sc)
        return top
    a0, b0, _, _ = best(range(renorm.A_MIN, renorm.A_MAX + 1, renorm.COARSE_A), range(-renorm.B_MAX, renorm.B_MAX + 1, renorm.COARSE_B))
    return best(range(max(renorm.A_MIN, a0 - renorm.FINE_A), min(renorm.A_MAX, a0 + renorm.FINE_A) + 1),
                range(max(-renorm.B_MAX, b0 - renorm.FINE_B), min(renorm.B_MAX, b0 + renorm.FINE_B) + 1))


def detect(raw_signal, tc, pm, params, QA=None, min_share=None, pm_mod=None):
    """(row, record, state): row as orc.detect returns it; record = (applied, {signal: None or (a, b, w, score)});
    state: the maps after the fold, the level values, the status and the geometry."""
    raw_signal = np.asarray(raw_signal)
    want_raw = pm_mod is not None and tc.get('mod') is not None
    maps, signals, status, med, mad = condition(raw_signal, pm, want_raw)
    u8, flt, h2, c2 = signals['morph'], signals['filtered'], maps['h2'], maps['c2']
    record = (0, {s: None for s in renorm.SIGNALS})
    if QA is not None:
        maps, record = renorm.apply(maps, signals, QA[0], QA[1], pm.model_min, pm.model_max, min_share, status)
    morph = normalize(u8, maps['morph'], h2, c2, pm)
    fltn = normalize(flt, maps['filtered'], h2, c2, pm)
    trim_prefix = len(tc['prefix_ext']) - len(tc['prefix'])
    trim_suffix = len(tc['suffix_ext']) - len(tc['suffix'])
    score_prefix, prefix_begin, prefix_end = orc.detect_range(morph, tc['prefix_ext'], params, pre_trim=trim_prefix)
    score_suffix, suffix_begin, suffix_end = orc.detect_range(morph, tc['suffix_ext'], params, post_trim=trim_suffix)
    n = 0; p = 0; mod_pattern = '-'
    if prefix_begin < suffix_end and score_prefix > 0.0 and score_suffix > 0.0:
        model = tc['hmm']
        logp, path, counted = orc.viterbi(model, fltn[prefix_begin:suffix_end])
        if path is not None:
            n = int(counted) + tc['count_bias']; p = logp
            if want_raw:
                names = [model.names[s] for s in path]
                nrm = normalize(raw_signal, maps['raw'], h2, c2, pm)
                mask = np.array(['repeat' in x for x in names], bool)
                mod_pattern = orc.mod_repeats(tc['mod'], tc['mod_range'], nrm[prefix_begin:suffix_end][mask])
        else:
            n, p = 0, 0
    row = (n, score_prefix, score_suffix, p, prefix_end, max(suffix_begin - prefix_end, 0), mod_pattern)
    state = dict(maps=maps, status=status, med=med, mad=mad, u8=u8,
                 level_val=renorm.level_values(maps['morph'][0], maps['morph'][1], h2, c2, pm.model_min + .5, pm.model_max - .5),
                 prefix_begin=prefix_begin, suffix_end=suffix_end)
    return row, record, state


# ---------------------------------------------------------------------------------------------
# the reads: backbone | prefix150 | repeat x n | suffix150 | backbone on the strand the signal is read in
# ---------------------------------------------------------------------------------------------
def make_read(table, make_signal, target, strand, n_units, backbone, seed, as_int16=True):
    """One read; its repeat share is n_units * len(repeat) / len(sequence)."""
    repeat, prefix, suffix = (s.upper() for s in target)
    rng = np.random.Generator(np.random.PCG64(seed))
    letters = np.array(list("ACGT"))
    left = "".join(letters[rng.integers(0, 4, backbone)]); right = "".join(letters[rng.integers(0, 4, backbone)])
    seq = left + prefix + repeat * n_units + suffix + right
    if strand == '-':
        seq = orc.revcomp(seq)
    return make_signal(rng, table, seq.encode(), as_int16, 0.0)


def setup(tables, cfg):
    """(product KmerTable, oracle pore model, align params)."""
    from strique_amd import synth
    from strique_amd.pore_model import pore_model
    t = (tables["base_kmer"], tables["base_mean"], tables["base_stdv"])
    return synth.KmerTable(pore_model(table=t)), orc.PoreModel(table=t), orc.align_params(cfg["align"])


MIN_SHARE = 0.3       # the threshold the shared reads are run with: between the fitted shares of the 0.04 reads (0.07) and of the others (0.7 and up)
SEED = 7

# (name, target, strand, units, backbone nt per side, int16?, repeat share of the sequence)
READS = [
    ("c9_p_004_i", "c9orf72", "+", 20, 1350, True, 0.04),
    ("c9_m_072_i", "c9orf72", "-", 1000, 1000, True, 0.72),
    ("c9_p_093_i", "c9orf72", "+", 2400, 400, True, 0.93),
    ("fm_m_004_i", "fmr1", "-", 40, 1290, True, 0.04),
    ("fm_p_072_i", "fmr1", "+", 1000, 433, True, 0.72),
    ("fm_m_093_i", "fmr1", "-", 4800, 400, True, 0.93),
    ("c9_m_004_f", "c9orf72", "-", 20, 1350, False, 0.04),
    ("c9_p_072_f", "c9orf72", "+", 1000, 1000, False, 0.72),
    ("fm_p_093_f", "fmr1", "+", 4800, 400, False, 0.93),
    ("fm_m_072_f", "fmr1", "-", 1000, 433, False, 0.72),
]
# the reads of the issue's table that detect() loses as it stands: C9orf72 x 2500 with 1 kb per side, FMR1 x 2500 with 0.4 kb (share 0.87)
LOST = [
    ("c9_p_087", "c9orf72", "+", 2500, 1000, True, 0.87),
    ("c9_m_087", "c9orf72", "-", 2500, 1000, True, 0.87),
    ("fm_p_087", "fmr1", "+", 2500, 400, True, 0.87),
    ("fm_m_087", "fmr1", "-", 2500, 400, True, 0.87),
]
_CACHE = {}


def share_of(spec, cfg):
    repeat, prefix, suffix = cfg["repeat"][spec[1]][3:6]
    return spec[3] * len(repeat) / (spec[3] * len(repeat) + len(prefix) + len(suffix) + 2 * spec[4])


def signal_of(spec, tables, cfg):
    from strique_amd import synth
    key = ("sig", spec[0])
    if key not in _CACHE:
        table, _, _ = setup(tables, cfg)
        _CACHE[key] = make_read(table, synth.make_signal, tuple(cfg["repeat"][spec[1]][3:6]), spec[2], spec[3], spec[4], SEED, spec[5])
    return _CACHE[key]


def with_outliers(sig):
    """A copy of an int16 read with 30 runs of three samples at each end of the int16 range (a run of three survives the median
    filter): fewer samples than the 1 % tails hold, far outside the grid."""
    out = np.array(sig, copy=True)
    at = np.arange(60) * (len(out) // 60) + 7
    for k in range(3):
        out[at[:30] + k] = 32767; out[at[30:] + k] = -32768
    return out


def run_specs(specs, tables, cfg, plain=False, opm_mod=None):
    """[(spec, signal, row, record, state)] of the reference with the rule at MIN_SHARE (plain: also 'plain_row', the oracle's detect()
    as it stands, as a sixth element), computed once per process, on a few threads."""
    from concurrent.futures import ThreadPoolExecutor
    _, opm, params = setup(tables, cfg)
    orc.lib()

    def one(spec):
        key = ("run", spec[0], plain, opm_mod is not None)
        if key in _CACHE:
            return _CACHE[key]
        target = tuple(cfg["repeat"][spec[1]][3:6])
        tc = orc.classifier(*target, spec[2], opm, opm_mod, cfg["HMM"])
        QA = target_tables(opm, target[0], spec[2])
        sig = signal_of(spec, tables, cfg)
        row, rec, st = detect(sig, tc, opm, params, QA, MIN_SHARE, pm_mod=opm_mod)
        out = (spec, sig, row, rec, st)
        if plain:
            out += (orc.detect(sig, tc, opm, params)[0],)
        _CACHE[key] = out
        return out
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(one, specs))
