"""Models, windows and two CPU references for the MARK, HUB and UNIT decodes of the Viterbi kernels (strique_amd/csrc/vit_model.h,
viterbi_kernels.hip) -- no GPU involved.  tests/test_vit_mode_cases_host.py checks the cases themselves (which kernel shape every
model lands on, that the two references agree, that the cases exercise what they claim), tests/test_gpu_viterbi_modes.py holds the
kernels against them through strq_debug_viterbi_mode.

Reference A comes from the oracle's state path (orc.viterbi: bit-exact log-probability, ties to the lowest source).  Reference B is
a float64 DP of its own, written from the contract in vit_model.h: it carries the three payloads along the winner of every state
(first of equal candidates, silent states in topological order) and so yields every record of every time step, also those off the
best path.

The last section gives the same models windows the way the detect pipeline hands them over -- int16 or float64 samples and a
per-window map -- for tests/test_gpu_viterbi_sources.py (strq_debug_viterbi_sourced): the kernels then take another instantiation of
their time loop than for plain float64 windows."""
import math
from collections import namedtuple

import numpy as np

VIT_COUNT, VIT_BACKPTR, VIT_MARK, VIT_HUB, VIT_UNIT = range(5)
SHAPE_CSR, SHAPE_G2, SHAPE_SS = 8, 9, 16
MODE_NAMES = {VIT_COUNT: "count", VIT_BACKPTR: "backptr", VIT_MARK: "mark", VIT_HUB: "hub", VIT_UNIT: "unit"}
BRANCH_OF_TAG = {1: 1, 3: 2, 4: 3}

# A test model: `row` / `ss` the kernel shape it was made for (row 8: the general kernel), `modes` the decode modes it is to
# exercise, `g2` whether strq_model_set_positions gives it a register-resident image, `windows` a list of (label, x); a label that
# starts with "nopath" marks a window built to have no path, `tie_prone` a model built to meet ties.
Case = namedtuple("Case", ["name", "baked", "row", "ss", "modes", "g2", "windows", "tie_prone"])

# ------------------------------------------------------------------------------------------------------------------------
# generated models
# ------------------------------------------------------------------------------------------------------------------------
# per row: emitting states, silent states, the in-degree of the emitting states of every group of 64 (unhinted states are dealt to
# slots by descending in-degree, so group g is slot g), the in-degree of the silent states without their chain edge, whether the
# states from 128 on are Uniform only, and whether the model has exactly two counted emitting states (the rows with UNIT)
ROW_SPECS = {
    0: dict(ne=200, ns=100, deg=(6, 5, 3, 3), sdeg=3, flat=False, unit=True),       # a silent in-degree of 3 keeps it off rows 7 and 5
    1: dict(ne=56, ns=30, deg=(7,), sdeg=3, flat=False, unit=False),
    2: dict(ne=100, ns=90, deg=(8, 6), sdeg=4, flat=False, unit=True),
    3: dict(ne=150, ns=140, deg=(8, 7, 5), sdeg=6, flat=False, unit=True),
    4: dict(ne=300, ns=70, deg=(8, 8, 6, 5, 4), sdeg=5, flat=False, unit=True),
    5: dict(ne=230, ns=80, deg=(6, 5, 3, 3), sdeg=2, flat=False, unit=True),
    6: dict(ne=48, ns=20, deg=(5,), sdeg=1, flat=False, unit=False),
    7: dict(ne=230, ns=80, deg=(6, 5, 3, 3), sdeg=2, flat=True, unit=True),
}
ROW_MODES = {0: (0, 1, 2, 4), 1: (0, 1, 2, 3), 2: (0, 1, 2, 3, 4), 3: (0, 1, 2, 4), 4: (0, 1, 2, 4), 5: (0, 1, 2, 4), 6: (0, 1, 2, 3), 7: (0, 1, 2, 4),
             SHAPE_CSR: (0, 1, 2), SHAPE_G2: (0, 2, 4)}
SPECIAL_MU = (28.0, 34.0, 146.0, 152.0)          # hub, recording hub, counted 0, counted 1: outside every other emission
UNI_LO, UNI_HI = 50.0, 130.0
UNI_WIDE = (20.0, 160.0)          # a support that holds the special means too: the models of the clipped, sourced windows (below)


def _baked(n, ne, start, end, ins, lps, kind, ea, eb, ec, count_inc, tag):
    from strique_amd.hmm import BakedHMM
    in_ptr = np.zeros(n + 1, np.int32); src, lp = [], []
    for l in range(n):
        ks = sorted(ins[l])
        in_ptr[l + 1] = in_ptr[l] + len(ks)
        src += ks; lp += [lps[(k, l)] for k in ks]
    return BakedHMM(n, ne, start, end, in_ptr, np.array(src, np.int32), np.array(lp, np.float64), np.asarray(kind, np.int32),
                    np.asarray(ea, np.float64), np.asarray(eb, np.float64), np.asarray(ec, np.float64), np.asarray(count_inc, np.int32),
                    np.asarray(tag, np.int32), ["s%d" % i for i in range(n)], np.arange(n, dtype=np.int32),
                    np.full(n, -1, np.int32), np.full(n, -1, np.int32))


def generated_model(row, multi, seed=0, fan=0, support=(UNI_LO, UNI_HI)):
    """A baked model steered onto lane row `row` (single-stage unless `multi`); with fan > 8 every third emitting state gets that
    many more in-edges and the model goes to the general kernel.  `support`: the range of its Uniform emissions (no random draw
    depends on it: models of two supports differ in those three emission arrays only)."""
    sp = ROW_SPECS[row]
    rng = np.random.default_rng(9000 + 100 * row + 10 * int(multi) + seed + fan)
    ne, ns = sp["ne"], sp["ns"]
    n = ne + ns; start, end = ne, n - 1
    specials = (5, 11, 17, 23)          # hub, recording hub, counted 0, counted 1: in the first group of 64
    rec = specials[1]
    ins = [set() for _ in range(n)]
    for l in range(ne):
        want = sp["deg"][l // 64]
        if l < 4:
            ins[l].add(start)
        ins[l].add((l - 1) % ne)          # a ring: every emitting state is reachable
        if len(ins[l]) < want and rng.random() < 0.4:
            ins[l].add(int(rng.integers(ne + 1, n - 1)))          # a silent state that is neither start nor end
        if len(ins[l]) < want and rng.random() < 0.6:
            ins[l].add(l)
        if len(ins[l]) < want and rng.random() < 0.5:
            ins[l].add(int(specials[int(rng.integers(0, 4))]))          # the special states lead somewhere
        while len(ins[l]) < want:
            ins[l].add(int(rng.integers(0, ne)))
    cap = sp["sdeg"]
    for l in range(ne + 1, n):
        ins[l].add(l - 1)                  # one chain through all silent states
        extra = multi and l - ne >= 3 and (l - ne) % 3 == 0
        if extra:
            ins[l].add(int(rng.integers(ne, l - 1)))          # a silent predecessor outside the chain: multi-stage
        k = cap - (1 if extra else 0) if l in (ne + 1, end) or (l - ne) % 3 == 0 else int(rng.integers(min(1, cap - 1), cap + 1))
        if l == end:
            ins[l].add(rec)
        if l == ne + 1:
            ins[l] |= set(range(min(k, 2)))          # the states behind start can end a window of one observation
        while len(ins[l]) - 1 - (1 if extra else 0) < k:
            ins[l].add(int(rng.integers(0, ne)))
    lps = {}
    for l in range(n):
        for k in ins[l]:
            lps[(k, l)] = math.log(rng.uniform(0.05, 0.9))
    kind = rng.integers(1, 3, ne).astype(np.int32)
    if sp["flat"]:
        kind[128:] = 2
    elif ne > 128:
        kind[128::3] = 1                   # Normal emissions in the low-degree slots too
    for s in specials:
        kind[s] = 1
    mu = rng.uniform(60, 120, ne); sigma = rng.uniform(1.0, 4.0, ne)
    for s, m in zip(specials, SPECIAL_MU):
        mu[s] = m; sigma[s] = 1.5
    ea = np.where(kind == 1, mu, support[0]); eb = np.where(kind == 1, 1.0 / (2 * sigma ** 2), support[1])
    ec = np.where(kind == 1, -np.log(sigma * 2.50662827463), -math.log(support[1] - support[0]))
    tag = rng.choice(np.array([0, 1, 3, 4]), n).astype(np.int32)
    tag[ne:] = 0
    tag[specials[0]] = tag[specials[1]] = 2
    tag[specials[2]] = 0; tag[specials[3]] = 1
    if sp["unit"] and not fan:
        count_inc = np.zeros(n, np.int32); count_inc[specials[2]] = count_inc[specials[3]] = 1
    else:
        count_inc = (rng.random(n) < 0.1).astype(np.int32)          # silent states too: the count of a mark decode adds them
    if fan:
        for l in range(0, ne, 3):
            for k in rng.choice(ne, size=fan, replace=False):
                if int(k) not in ins[l]:
                    ins[l].add(int(k)); lps[(int(k), l)] = math.log(rng.uniform(0.05, 0.9))
    return _baked(n, ne, start, end, ins, lps, kind, ea, eb, ec, count_inc, tag)


def _walk_signal(bk, rng, T):
    """Observations along a random walk through the emitting states that keeps coming back to the special states (the tag-2 hubs and
    the counted states), so that their records are on the best path: a Normal state emits near its mean, a Uniform one anywhere."""
    ne = bk.silent_start
    succ = [[] for _ in range(bk.n_states)]
    for l in range(ne):
        for e in range(bk.in_ptr[l], bk.in_ptr[l + 1]):
            succ[int(bk.in_src[e])].append(l)
    inc = np.asarray(bk.count_inc)
    special = [s for s in range(ne) if bk.tag[s] == 2 or (inc[s] == 1 and inc[:ne].sum() == 2)]

    def route(a, b):          # shortest walk a -> b through emitting states (without a), or None
        prev = {a: None}; q = [a]
        while q:
            nq = []
            for u in q:
                for w in succ[u]:
                    if w not in prev:
                        prev[w] = u; nq.append(w)
                        if w == b:
                            out = [b]
                            while prev[out[-1]] != a:
                                out.append(prev[out[-1]])
                            return out[::-1]
            q = nq
        return None

    cur = bk.start; path = []; turn = int(rng.integers(0, 4))
    while len(path) < T:
        leg = None
        if special and rng.random() < 0.7:
            leg = route(cur, special[turn % len(special)]); turn += 1
        if not leg:
            leg = [succ[cur][int(rng.integers(0, len(succ[cur])))]]
        path += leg; cur = path[-1]
    x = np.zeros(T)
    for t, s in enumerate(path[:T]):
        if bk.emis_kind[s] == 1:
            x[t] = bk.emis_a[s] + rng.normal(0.0, 0.3) / math.sqrt(2 * bk.emis_b[s])
        else:
            x[t] = rng.uniform(bk.emis_a[s] + 1, bk.emis_b[s] - 1)
    return x


T_LIST = (1, 2, 63, 64, 65, 150, 333)


def _standard_windows(make, rng, nopath_T=()):
    """The windows every model gets: make(T) gives a signal of T observations; nopath_T: the lengths too short for any path."""
    wins = [(("nopath_T%d" if T in nopath_T else "T%d") % T, make(T)) for T in T_LIST]
    x = make(150).copy(); x[::7] = np.nan
    wins.append(("nan7", x))
    wins.append(("allnan", np.full(57, np.nan)))
    x = make(20).copy(); x[5] = np.inf          # no distribution gives it a finite log-probability
    wins.append(("nopath", x))
    return wins


def _generated_case(name, row, multi, fan=0, support=(UNI_LO, UNI_HI)):
    bk = generated_model(row, multi, fan=fan, support=support)
    rng = np.random.default_rng(77 + 13 * row + int(multi))
    wins = _standard_windows(lambda T: _walk_signal(bk, rng, T), rng)
    shape = SHAPE_CSR if fan else row
    return Case(name, bk, shape, (not multi) and not fan, ROW_MODES[shape], False, wins, False)


# ------------------------------------------------------------------------------------------------------------------------
# the mark boundary model
# ------------------------------------------------------------------------------------------------------------------------
BOUNDARY_TIMES = ((7, 4095), (4095, 4096), (4096, 4097), (4097, 8192), (8192, 8193))          # (first tagged emission, first emission behind), 1-based
BOUNDARY_LEVELS = (70.0, 100.0, 130.0)


def boundary_model(variant):
    """Untagged -> tagged -> untagged, each a Normal emission with a self-loop.  variant "ss": a lane row, single-stage; "multi": a
    silent state with a silent predecessor outside its chain; "csr": nine more in-edges (from states nothing reaches) on the last
    state, so that only the general kernel takes it."""
    extra = 9 if variant == "csr" else 0
    ne = 3 + extra; ns = 4; n = ne + ns; start = ne; s1, s2 = ne + 1, ne + 2; end = n - 1
    ins = [set() for _ in range(n)]
    ins[0] = {0, start}; ins[1] = {0, 1}; ins[2] = {1, 2} | set(range(3, ne))
    for k in range(3, ne):
        ins[k] = {k}
    ins[s1] = {start}; ins[s2] = {s1, 2}; ins[end] = {s2, 2}
    if variant == "multi":
        ins[end] = {s2, s1}          # (the last state still reaches end through s2)
    lps = {(k, l): math.log(0.5) for l in range(n) for k in ins[l]}
    mu = np.concatenate([BOUNDARY_LEVELS, np.full(extra, 40.0)]); sigma = np.full(ne, 2.0)
    tag = np.zeros(n, np.int32); tag[1] = 1
    inc = np.zeros(n, np.int32); inc[1] = 1
    return _baked(n, ne, start, end, ins, lps, np.ones(ne, np.int32), mu, 1.0 / (2 * sigma ** 2), -np.log(sigma * 2.50662827463), inc, tag)


def boundary_windows():
    out = []
    for enter, leave in BOUNDARY_TIMES:
        T = min(leave + 9, 8300)
        x = np.full(T, BOUNDARY_LEVELS[2]); x[:leave - 1] = BOUNDARY_LEVELS[1]; x[:enter - 1] = BOUNDARY_LEVELS[0]
        out.append(("enter%d_leave%d" % (enter, leave), x))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# STRique's own models
# ------------------------------------------------------------------------------------------------------------------------
def _pm_signal(pm, rng, seq, samples, lo=None, hi=None):
    s = pm.generate_signal(seq, samples=samples, noise=True, rng=rng)
    return np.clip(s, (pm.model_min if lo is None else lo) + .5, (pm.model_max if hi is None else hi) - .5)


def _skip_window(bk, x, pm):
    """The window with the first k-mer of two repeat units cut out: behind the second and the third counted emission of its best
    path, that emission and the stay in the state behind it become two observations far from that state's mean.  The path then
    closes those rounds of the loop through the insert-type dummy state -- the other of the two counted states."""
    from oracle import strique_oracle
    _, path, _ = strique_oracle.viterbi(bk, x)
    us = unit_states(bk)
    visits = [t for t, s in enumerate(path) if int(s) in us]
    parts = []; pos = 0
    for a in visits[1:3]:
        nxt = path[a + 1]; b = a + 1
        while path[b] == nxt:
            b += 1
        far = pm.model_min + 1.0 if bk.emis_a[nxt] > (pm.model_min + pm.model_max) / 2 else pm.model_max - 1.0
        parts += [x[pos:a], np.array([far, far])]; pos = b
    return np.concatenate(parts + [x[pos:]])


def _strique_cases(pm, pm_mod, cfg):
    from strique_amd import hmm
    from test_g2_layout import tie_prone
    out = []
    # (flanks of 30 nt leave three emitting slots: the hinted layout lands on row 5; 50 nt fill four, the last two with inserts only: row 7)
    for label, name, rep_override, fl, row in (("c9orf72", "c9orf72", None, 30, 5), ("fmr1", "fmr1", None, 50, 7), ("cagca", "c9orf72", "CAGCA", 30, 5)):
        chrom, b, e, repeat, prefix, suffix = cfg["repeat"][name]
        repeat = rep_override or repeat
        fm = hmm.FlankedRepeatModel(repeat, prefix[-fl:], suffix[:fl], pm, cfg["HMM"])
        rng = np.random.default_rng(500 + len(out))
        full = [_pm_signal(pm, rng, prefix[-fl:] + repeat * k + suffix[:fl], 4) for k in (2, 5, 9)]
        wins = [("rep%d" % k, x) for k, x in zip((2, 5, 9), full)] + [("skip", _skip_window(fm.baked, full[2], pm))]
        # (every path emits in both flanks and in the repeat: no window of one or two observations has one)
        wins += _standard_windows(lambda T: full[2][:T], rng, nopath_T=(1, 2))
        out.append(Case("flanked_" + label, fm.baked, row, True, ROW_MODES[SHAPE_G2], True, wins, False))
        for seed in (0, 1):
            trng = np.random.default_rng(100 + seed)
            bk = tie_prone(fm.baked, trng if seed else None)
            twins = [("T%d" % T, trng.uniform(10.0, 150.0, T)) for T in (40, 75, 130, 333)]
            out.append(Case("tie_%s_%d" % (label, seed), bk, None, True, ROW_MODES[SHAPE_G2], True, twins, True))
    mm = hmm.RepeatModModel("GGCCCC", pm, pm_mod, cfg["HMM"])
    rng = np.random.default_rng(600)
    full = _pm_signal(pm, rng, "GGCCCC" * 12 + "GGCCC", 8, mm.model_min, mm.model_max)
    wins = [("units12", full)] + _standard_windows(lambda T: full[:T], rng, nopath_T=(1, 2))          # (s0, a unit, e0: at least three observations)
    out.append(Case("dual_ggcccc", mm.baked, 6, None, (0, 1, 2, 3), False, wins, False))
    return out


# the names cases() gives, for parametrised tests (the host test holds the two against each other)
CASE_NAMES = (["row%d_%s" % (row, v) for row in range(8) for v in ("ss", "multi")] + ["general", "boundary_ss", "boundary_multi", "boundary_csr"] +
              [n for label in ("c9orf72", "fmr1", "cagca") for n in ("flanked_" + label, "tie_%s_0" % label, "tie_%s_1" % label)] + ["dual_ggcccc"])

_CASES = {}


def cases(pm, pm_mod, cfg):
    """Every case, built once per process."""
    if not _CASES:
        lst = []
        for row in sorted(ROW_SPECS):
            for multi in (False, True):
                lst.append(_generated_case("row%d_%s" % (row, "multi" if multi else "ss"), row, multi))
        lst.append(_generated_case("general", 1, True, fan=14))
        for variant, row, ss in (("ss", 6, True), ("multi", 6, False), ("csr", SHAPE_CSR, False)):
            lst.append(Case("boundary_" + variant, boundary_model(variant), row, ss, (0, 1, 2), False, boundary_windows(), False))
        lst += _strique_cases(pm, pm_mod, cfg)
        for c in lst:
            _CASES[c.name] = c
    return _CASES


# ------------------------------------------------------------------------------------------------------------------------
# Reference A: from the oracle's path
# ------------------------------------------------------------------------------------------------------------------------
_REF_A = {}
_REF_B = {}


def rec_state(bk):
    """The hub state (tag 2) with an edge into `end`: the last of them in in-edge order; -1 none."""
    r = -1
    for e in range(bk.in_ptr[bk.end], bk.in_ptr[bk.end + 1]):
        k = int(bk.in_src[e])
        if k < bk.silent_start and bk.tag[k] == 2:
            r = k
    return r


def unit_states(bk):
    """The two counted states of a unit decode: exactly two emitting states with count_inc 1 and no other counted state."""
    nz = [int(l) for l in np.nonzero(np.asarray(bk.count_inc))[0]]
    if len(nz) != 2 or any(l >= bk.silent_start or bk.count_inc[l] != 1 for l in nz):
        return (-1, -1)
    return (nz[0], nz[1])


def reference_a(orc, case, label, x):
    """{'logp', 'path' (None: no path), 'counted', 'enter', 'leave', 'hub' [(time, branch)], 'unit' [(observation, k)]}."""
    key = (case.name, label)
    if key in _REF_A:
        return _REF_A[key]
    bk = case.baked
    logp, path, counted = orc.viterbi(bk, x)
    out = {"logp": logp, "path": path, "counted": counted, "enter": 0, "leave": 0, "hub": [], "unit": []}
    if path is not None:
        tag = np.asarray(bk.tag)[path]
        inside = np.nonzero(tag == 1)[0]
        if len(inside):
            out["enter"] = int(inside[0]) + 1
            behind = np.nonzero(tag[inside[0]:] != 1)[0]
            if len(behind):
                out["leave"] = int(inside[0] + behind[0]) + 1
        rec = rec_state(bk); branch = 0
        for t, s in enumerate(path):
            if bk.tag[s] != 2:
                branch = BRANCH_OF_TAG.get(int(bk.tag[s]), 0)
            if s == rec:
                out["hub"].append((t + 1, branch))
        us = unit_states(bk)
        out["unit"] = [(t, us.index(int(s))) for t, s in enumerate(path) if int(s) in us and us[0] >= 0]
    _REF_A[key] = out
    return out


def hub_chain(dbg0, records):
    """The (time, branch) of every recorded hub emission on the best path, by hopping back from the end state's payload."""
    out = []; cur = int(dbg0)
    while cur:
        assert 0 < cur < len(records) and len(out) <= len(records), "a hub record points outside the window"
        r = int(records[cur])
        out.append((cur, r >> 32))
        assert (r & 0xFFFFFFFF) < cur, "hub records must lead backwards"
        cur = r & 0xFFFFFFFF
    return out[::-1]


def unit_chain(dbg0, records):
    """The (observation, k) of every counted emission on the best path; records[t][k]."""
    out = []; cur = int(dbg0)
    while cur:
        t, k = (cur >> 1) - 1, cur & 1
        assert 0 <= t < len(records), "a unit record points outside the window"
        out.append((t, k))
        nxt = int(records[t][k])
        assert nxt == 0 or (nxt >> 1) - 1 < t, "unit records must lead backwards"
        cur = nxt
    return out[::-1]


# ------------------------------------------------------------------------------------------------------------------------
# Reference B: an independent DP that carries the payloads
# ------------------------------------------------------------------------------------------------------------------------
def reference_b(case, label, x):
    """Float64 Viterbi with the three payloads riding along the winner of every state.  Returns {'logp', 'counted', 'enter',
    'leave', 'hub_last', 'unit_last', 'hub_rec' (T + 1 uint64), 'hub_live' (T + 1 bool: the recording state had a finite value),
    'unit_rec' (T, 2 uint32), 'unit_live' (T, 2 bool), 'tied' (T, n_emit bool: the winner of the state had a finite equal rival)}."""
    key = (case.name, label)
    if key in _REF_B:
        return _REF_B[key]
    bk = case.baked
    n, ne = bk.n_states, bk.silent_start
    T = len(x)
    NEG = -np.inf
    in_ptr = np.asarray(bk.in_ptr); in_src = np.asarray(bk.in_src); in_lp = np.asarray(bk.in_logp, np.float64)
    deg = np.diff(in_ptr)
    D = max(1, int(deg[:ne].max()))
    E_src = np.full((ne, D), n, np.int64); E_lp = np.zeros((ne, D))
    for l in range(ne):
        d = int(deg[l])
        E_src[l, :d] = in_src[in_ptr[l]:in_ptr[l + 1]]; E_lp[l, :d] = in_lp[in_ptr[l]:in_ptr[l + 1]]
    silent = [(l, [(int(in_src[e]), float(in_lp[e])) for e in range(in_ptr[l], in_ptr[l + 1])]) for l in range(ne, n)]
    inc = np.asarray(bk.count_inc, np.int64); tag = np.asarray(bk.tag)
    tag1 = tag[:ne] == 1; hubst = tag[:ne] == 2
    branch = np.array([BRANCH_OF_TAG.get(int(t), 0) for t in tag[:ne]], np.int64)
    rec = rec_state(bk); us = unit_states(bk)
    kind = np.asarray(bk.emis_kind); ea = np.asarray(bk.emis_a, np.float64); eb = np.asarray(bk.emis_b, np.float64); ec = np.asarray(bk.emis_c, np.float64)
    rows = np.arange(ne)
    # value and payloads of every state (+ the cell that padding edges read), as lists for the silent pass
    v = [NEG] * (n + 1)
    pay = {k: [0] * (n + 1) for k in ("cnt", "ent", "lev", "hlo", "hhi", "up")}
    sinc = [int(i) for i in inc]

    def silent_pass(pin):
        for l, edges in silent:
            if pin and l == bk.start:
                v[l] = 0.0
                for k in pay:
                    pay[k][l] = 0
                continue
            best = NEG; arg = -1
            for k, lp in edges:
                c = v[k] + lp
                if c > best:
                    best = c; arg = k
            v[l] = best
            if arg >= 0:
                for k in pay:
                    pay[k][l] = pay[k][arg]
                pay["cnt"][l] += sinc[l]
            else:
                for k in pay:
                    pay[k][l] = 0

    silent_pass(True)
    hub_rec = np.zeros(T + 1, np.uint64); hub_live = np.zeros(T + 1, bool)
    unit_rec = np.zeros((T, 2), np.uint32); unit_live = np.zeros((T, 2), bool)
    tied = np.zeros((T, ne), bool)
    for t in range(T):
        xt = float(x[t]); tt1 = t + 1
        pv = np.array(v); P = {k: np.array(a, np.int64) for k, a in pay.items()}
        cand = pv[E_src] + E_lp
        win = np.argmax(cand, axis=1)          # the first of equal candidates
        best = cand[rows, win]; wsrc = E_src[rows, win]
        tied[t] = ((cand == best[:, None]).sum(axis=1) > 1) & np.isfinite(best)
        if xt != xt:
            em = np.zeros(ne)
        else:
            d = xt - ea
            with np.errstate(invalid="ignore", over="ignore"):
                en = ec - (d * d) * eb
            eu = np.where((xt >= ea) & (xt <= eb), ec, NEG)
            em = np.where(kind == 1, en, eu)
        nv = best + em
        cnt = P["cnt"][wsrc] + inc[:ne]
        ent = P["ent"][wsrc]; lev = P["lev"][wsrc]
        set_e = tag1 & (ent == 0); set_l = ~tag1 & (ent != 0) & (lev == 0)
        ent = np.where(set_e, tt1, ent); lev = np.where(set_l, tt1, lev)
        hlo = P["hlo"][wsrc]; hhi = np.where(hubst, P["hhi"][wsrc], branch)
        if rec >= 0:
            hub_rec[tt1] = (int(hhi[rec]) << 32) | int(hlo[rec]); hub_live[tt1] = nv[rec] > NEG
            hlo[rec] = tt1
        up = P["up"][wsrc]
        for k in (0, 1):
            if us[k] >= 0:
                unit_rec[t, k] = int(up[us[k]]); unit_live[t, k] = nv[us[k]] > NEG
                up[us[k]] = (tt1 << 1) | k
        v = nv.tolist() + [NEG] * (n - ne) + [NEG]
        for k, a in (("cnt", cnt), ("ent", ent), ("lev", lev), ("hlo", hlo), ("hhi", hhi), ("up", up)):
            pay[k] = a.tolist() + [0] * (n - ne + 1)
        silent_pass(False)
    e = bk.end
    has = v[e] > NEG
    out = {"logp": v[e], "counted": pay["cnt"][e] if has else 0, "enter": pay["ent"][e], "leave": pay["lev"][e], "hub_last": pay["hlo"][e],
           "unit_last": pay["up"][e], "hub_rec": hub_rec, "hub_live": hub_live, "unit_rec": unit_rec, "unit_live": unit_live, "tied": tied}
    _REF_B[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------------------
# Sourced windows: samples and a per-window map, the way the detect pipeline hands its windows to the kernels
# ------------------------------------------------------------------------------------------------------------------------
# The kernels read observation x' = clip((s - c1) / h1 * h2 + c2, lo, hi) from int16 or float64 samples s (hmm_wave.h:
# vit_observation) and, once per window, evaluate
#     fast = lo >= max(lower bounds of the Uniform emissions) and hi <= min(upper bounds) and c1 == c1 and h1 == h1
# -- true: the branch-free instantiation of the whole time loop, false: the general one that plain float64 windows take.  The
# generated models above keep their special states outside the Uniform support 50..130; a clip range inside it would tear every
# window off those states.  Their "wide" twins (support 20..160, everything else equal) keep hub and unit chains under a clip of
# 20.5..159.5.
VIT_SRC_F64_AFFINE, VIT_SRC_I16_AFFINE = 1, 2
WIDE_CLIP = (UNI_WIDE[0] + 0.5, UNI_WIDE[1] - 0.5)
BOUNDARY_CLIP = (40.0, 160.0)          # (the boundary models have no Uniform emission: any range gives the branch-free code)
# non-dyadic constants of the pipeline's magnitude: a sample step is h2 / h1 = 0.21 pA
MAP_C1, MAP_H1, MAP_H2, MAP_C2 = 417.3, 61.7, 13.1, 90.2
WIDE_NAMES = ["wide_row%d_%s" % (row, v) for row in range(8) for v in ("ss", "multi")] + ["wide_general"]
STRIQUE_NAMES = [n for n in CASE_NAMES if n.startswith(("flanked_", "tie_", "dual_"))]
BOUNDARY_NAMES = ["boundary_ss", "boundary_multi", "boundary_csr"]
SOURCED_NAMES = WIDE_NAMES + BOUNDARY_NAMES + STRIQUE_NAMES
# one model per kernel family meets the edges of the predicate: a lane row single-stage, one multi-stage, row 7 (the variant that
# skips the arithmetic of its upper slots), the general kernel and a flanked model on the register-resident kernel
EDGE_NAMES = ("wide_row2_ss", "wide_row4_multi", "wide_row7_ss", "wide_general", "flanked_c9orf72")

# `fast`: what the predicate is to give for the window; x_prime is the window both references decode
Sourced = namedtuple("Sourced", ["label", "kind", "samples", "consts", "x_prime", "fast"])

_WIDE = {}
_SOURCED = {}


def narrow_name(name):
    return name[len("wide_"):]


def wide_cases():
    """The generated cases once more, on models whose Uniform emissions span UNI_WIDE."""
    if not _WIDE:
        for row in sorted(ROW_SPECS):
            for multi in (False, True):
                c = _generated_case("wide_row%d_%s" % (row, "multi" if multi else "ss"), row, multi, support=UNI_WIDE)
                _WIDE[c.name] = c
        _WIDE["wide_general"] = _generated_case("wide_general", 1, True, fan=14, support=UNI_WIDE)
    return _WIDE


def sourced_cases(pm, pm_mod, cfg):
    """name -> Case of every model that decodes sourced windows (SOURCED_NAMES)."""
    both = dict(cases(pm, pm_mod, cfg)); both.update(wide_cases())
    return {n: both[n] for n in SOURCED_NAMES}


def uniform_bounds(bk):
    """(largest lower bound, smallest upper bound) of the model's Uniform emissions; (-inf, inf) without one."""
    uni = np.asarray(bk.emis_kind) == 2
    if not uni.any():
        return -np.inf, np.inf
    return float(np.asarray(bk.emis_a)[uni].max()), float(np.asarray(bk.emis_b)[uni].min())


def predicate(bk, consts):
    """The kernels' choice of the branch-free code for a window of an affine source."""
    c1, h1, h2, c2, lo, hi = consts
    ulo, uhi = uniform_bounds(bk)
    return bool(lo >= ulo and hi <= uhi and c1 == c1 and h1 == h1)


def observations(samples, consts):
    """x' of the samples, in the kernel's order of operations, every one rounded on its own."""
    c1, h1, h2, c2, lo, hi = (np.float64(v) for v in consts)
    v = (np.asarray(samples).astype(np.float64) - c1) / h1
    v = v * h2 + c2
    v = np.where(v < lo, lo, v)          # (a NaN stays: both comparisons are false)
    v = np.where(v > hi, hi, v)
    return v


def sourced(case, label, x, kind, consts, clip_at=None):
    """(samples, x_prime) of window `x`: samples from the inverse of the map, rounded to int16 or kept as float64, with -- windows of
    at least 63 observations -- two samples that clip at lo and two at hi, the first of each an extreme of int16; clip_at: their
    positions ((lo, lo), (hi, hi)).  NaN constants are inverted as the standard ones (the window is all NaN whatever the samples)."""
    c1, h1, h2, c2, lo, hi = consts
    ic1, ih1 = (c1 if c1 == c1 else MAP_C1), (h1 if h1 == h1 else MAP_H1)
    inv = lambda v: (np.asarray(v, np.float64) - c2) / h2 * ih1 + ic1
    s = inv(x)
    T = len(x)
    if T >= 63:
        (la, lb), (ha, hb) = clip_at or ((3, T // 3), (T - 4, 2 * T // 3))
        s[la] = -32768.0; s[lb] = inv(lo - 3.0); s[ha] = 32767.0; s[hb] = inv(hi + 3.0)
    if kind == VIT_SRC_I16_AFFINE:
        s = np.clip(np.rint(s), -32768, 32767).astype(np.int16)
    return s, observations(s, consts)


def _dual_mixed_window(bk):
    """A window of the dual model whose units alternate between the two branches -- the means of the branch's match states, six
    observations each, a little noise -- so that marks and hub records of both branches are on the best path (the case's own
    windows are unmodified signal: one branch)."""
    import re
    def means(prefix):
        st = sorted((int(re.fullmatch(prefix + r"(\d+)m", n).group(1)), i) for i, n in enumerate(bk.names) if re.fullmatch(prefix + r"\d+m", n))
        return [float(bk.emis_a[i]) for _, i in st]
    rng = np.random.default_rng(601)
    mu = {"b": means("base"), "m": means("mod")}
    return np.concatenate([np.repeat(mu[u], 6) + rng.normal(0.0, 0.4, 6 * len(mu[u])) for u in "bmmbmbbm"])


def _sourced_windows(c):
    bk = c.baked
    w = dict(c.windows)
    ulo, uhi = uniform_bounds(bk)
    boundary = c.name in BOUNDARY_NAMES
    clip = BOUNDARY_CLIP if boundary else (ulo + 0.5, uhi - 0.5)          # the pipeline's: model_min + 0.5 .. model_max - 0.5
    if c.tie_prone:          # (every emission Uniform over 0..200) the range of the flanked model they were made from
        flo, fhi = uniform_bounds(_CASES["flanked_" + c.name.split("_")[1]].baked)
        clip = (flo + 0.5, fhi - 0.5)
    short = (1, 2) if c.name in STRIQUE_NAMES else ()                     # no path that short in STRique's models
    out = []

    def add(label, x, kind, lo, hi, fast, c1=None, h1=None, clip_at=None):
        i = len(out)          # every window its own map
        consts = (MAP_C1 + 1.9 * i if c1 is None else c1, MAP_H1 + 0.3 * i if h1 is None else h1, MAP_H2, MAP_C2, lo, hi)
        s, xp = sourced(c, label, x, kind, consts, clip_at)
        out.append(Sourced(label, kind, s, consts, xp, fast))

    if boundary:
        for label, x in c.windows:          # clipped samples where they move no mark: low ones on the first level, high ones on the last
            add("i16_" + label, x, VIT_SRC_I16_AFFINE, clip[0], clip[1], True, clip_at=((1, 3), (len(x) - 4, len(x) - 2)))
        return out
    base = w["T333"]
    at = lambda T: w["T%d" % T] if ("T%d" % T) in w else (w["nopath_T%d" % T] if ("nopath_T%d" % T) in w else base[:T])
    for T in T_LIST:
        add(("nopath_i16_T%d" if T in short else "i16_T%d") % T, at(T), VIT_SRC_I16_AFFINE, clip[0], clip[1], True)
    for T in (65, 333):
        add("f64_T%d" % T, at(T), VIT_SRC_F64_AFFINE, clip[0], clip[1], True)
    if c.name in STRIQUE_NAMES:          # their own windows, those that samples can hold (no NaN, no infinity)
        for label, x in c.windows:
            if not label.startswith(("T", "nopath")) and np.isfinite(x).all():
                add("i16_" + label, x, VIT_SRC_I16_AFFINE, clip[0], clip[1], True)
        for label in ("T40", "T75", "T130"):
            if label in w:
                add("i16_own_" + label, w[label], VIT_SRC_I16_AFFINE, clip[0], clip[1], True)
    if c.name == "dual_ggcccc":
        x = _dual_mixed_window(bk)
        add("i16_mixed", x, VIT_SRC_I16_AFFINE, clip[0], clip[1], True)
        add("f64_mixed", x, VIT_SRC_F64_AFFINE, clip[0], clip[1], True)
    if c.name in EDGE_NAMES:
        # the clip range equal to the tightest Uniform support; one ulp wider on either side -- the observations that sit on that
        # limit are then outside an emission: the one way an affine source meets the general code; NaN constants: all NaN
        x = at(150)
        add("edge_eq_i16_T150", x, VIT_SRC_I16_AFFINE, ulo, uhi, True)
        add("edge_eq_f64_T150", x, VIT_SRC_F64_AFFINE, ulo, uhi, True)
        add("edge_lo_ulp_i16_T150", x, VIT_SRC_I16_AFFINE, np.nextafter(ulo, -np.inf), uhi, False)
        add("edge_hi_ulp_f64_T150", x, VIT_SRC_F64_AFFINE, ulo, np.nextafter(uhi, np.inf), False)
        add("edge_hi_ulp_i16_T150", x, VIT_SRC_I16_AFFINE, ulo, np.nextafter(uhi, np.inf), False)
        add("edge_nan_c1_i16_T65", at(65), VIT_SRC_I16_AFFINE, clip[0], clip[1], False, c1=np.nan)
        add("edge_nan_h1_f64_T65", at(65), VIT_SRC_F64_AFFINE, clip[0], clip[1], False, h1=np.nan)
        add("edge_nan_h1_i16_T64", at(64), VIT_SRC_I16_AFFINE, clip[0], clip[1], False, h1=np.nan)
    return out


def sourced_windows(c):
    """The sourced windows of a case (a list of Sourced), built once.  Labels are unique within the case and serve, behind "src:", as
    the cache labels of the references on x_prime; a label that starts with "nopath" marks a window too short for any path."""
    if c.name not in _SOURCED:
        _SOURCED[c.name] = _sourced_windows(c)
    return _SOURCED[c.name]


def ref_label(sw):
    return ("nopath_src:" if sw.label.startswith("nopath") else "src:") + sw.label
