"""Case lists and the reference of tests/test_passage_cases_host.py and tests/test_gpu_passage_scores.py: the per-passage scores of
the variant pass (csrc/variant_kernels.h) and the per-unit scores of the modification pass (csrc/mod_llr_kernels.h) on their own,
without the detect pipeline around them.  Plain numpy plus the CPU oracle; of the product only baked model arrays.

  V[j, b] = oracle.viterbi(masked_b, x[u_j : w_j + 1], want_path=False)[0],  u_0 = 0, u_j = w_{j-1} + 1,

masked_b the model with in_logp = -inf on every edge that has an emitting state of another branch at either end; -inf for every b
where the bounds are unusable (not 0 <= u_j <= w_j < T).  The definition of the two headers and of tests/variant_ref.py, restated on
baked arrays so that crafted models can be scored too.

Two tag vocabularies: "var" (0 base, 1 / 3 / 4 alt branch 1 / 2 / 3, 2 hub) and "llr" (0 base, 1 modified, 2 hub).
"""
import types

import numpy as np

from oracle import strique_oracle as orc

NEG = -np.inf
VAR_PAD, LLR_PAD = 1024, 256
HUB = -2
_BRANCH = {"var": {0: 0, 1: 1, 3: 2, 4: 3, 2: HUB}, "llr": {0: 0, 1: 1, 2: HUB}}
_TAG = {"var": (0, 1, 3, 4), "llr": (0, 1)}

# repeat unit, alt units, silent_start per alt count, (mode, NB) per alt count -- with the bundled k = 6 pore model
PRODUCT_VARIANTS = [
    ("C", ["A", "G"], {1: 16, 2: 28}, {1: (0, 2), 2: (0, 3)}),
    ("CGG", ["AGG", "CAG", "CGA"], {1: 26, 2: 44, 3: 62}, {1: (0, 2), 2: (1, 3), 3: (1, 4)}),
    ("GGCCCC", ["GGCCTC", "GGACCC", "AGCCCC"], {1: 38, 2: 62, 3: 86}, {1: (1, 2), 2: (1, 3), 3: (2, 4)}),
    ("ACGTTGC", ["ACGTTGA", "TCGTTGC"], {2: 72}, {2: (2, 3)}),
    ("ACGTTGCAAGTC", ["ACGTTGCAAGTA", "ACGTTGCATGTC"], {1: 74, 2: 122}, {1: (2, 2), 2: (2, 3)}),
]
# one product model per compiled variant instance but (mode 0, NB 4), which only a crafted model reaches
INSTANCE_MODELS = {(0, 2): ("CGG", 1), (0, 3): ("C", 2), (1, 2): ("GGCCCC", 1), (1, 3): ("CGG", 2), (1, 4): ("CGG", 3),
                   (2, 2): ("ACGTTGCAAGTC", 1), (2, 3): ("ACGTTGC", 2), (2, 4): ("GGCCCC", 3)}
# units of 3, 7, 15, 16 and 31 nt for the dual model of the modification pass: 2 + 4 L emitting states
MOD_UNITS = {3: "CGG", 7: "ACGTCGC", 15: "ACGTCGCATCGGTAC", 16: "ACGTCGCATCGGTACG", 31: "ACGTCGCATCGGTACGTTCGAACCGATCGTA"}
MOD_MODES = {3: 0, 7: 0, 15: 1, 16: 2, 31: 2}

SHORT = (1, 2, 3, 4, 5, 8)
LONG = (31, 32, 33, 63, 64, 65, 127, 128, 129, 150, 200)


def product_variant_cases():
    """[(repeat, alt units, silent_start, (mode, NB))] of every product model of PRODUCT_VARIANTS."""
    return [(rep, alts[:k], ne[k], inst[k]) for rep, alts, ne, inst in PRODUCT_VARIANTS for k in sorted(ne)]


def branches(baked, tags="var"):
    """Per state: 0 .. 3 its branch, HUB for a hub, -1 for a silent state."""
    out = np.full(baked.n_states, -1, np.int64)
    for l in range(baked.silent_start):
        out[l] = _BRANCH[tags][int(baked.tag[l])]
    return out


def as_model(baked, **changes):
    """The array fields of a baked model as a plain namespace (what oracle.viterbi and Context.model_create read)."""
    m = types.SimpleNamespace(n_states=int(baked.n_states), silent_start=int(baked.silent_start), start=int(baked.start), end=int(baked.end),
                              in_ptr=np.array(baked.in_ptr, np.int32), in_src=np.array(baked.in_src, np.int32),
                              in_logp=np.array(baked.in_logp, np.float64), emis_kind=np.array(baked.emis_kind, np.int32),
                              emis_a=np.array(baked.emis_a, np.float64), emis_b=np.array(baked.emis_b, np.float64),
                              emis_c=np.array(baked.emis_c, np.float64), count_inc=np.array(baked.count_inc, np.int32),
                              tag=np.array(baked.tag, np.int32))
    m.__dict__.update(changes)
    return m


def masked(baked, keep, tags="var"):
    """The model without the other branches: in_logp = -inf on every edge with an emitting state of another branch at either end."""
    br = branches(baked, tags)
    m = as_model(baked)
    other = (br >= 0) & (br != keep)
    dst = np.repeat(np.arange(m.n_states), np.diff(m.in_ptr))
    m.in_logp[other[dst] | other[m.in_src]] = NEG
    return m


_MASKED = {}


def _masked_copies(baked, nb, tags):
    key = (id(baked), nb, tags)
    if key not in _MASKED:
        _MASKED[key] = (baked, [masked(baked, b, tags) for b in range(nb)])          # (the model is kept alive: its id stays its own)
    return _MASKED[key][1]


def usable(w, T):
    """[(u_j, w_j) or None] of bounds w on T observations."""
    out = []
    for j in range(len(w)):
        u = 0 if j == 0 else int(w[j - 1]) + 1
        out.append((u, int(w[j])) if 0 <= u <= int(w[j]) < T else None)
    return out


def reference_scores(baked, nb, x, w, tags="var"):
    """(len(w), nb) float64: the masked Viterbi log-probability of every passage under every branch, from the oracle."""
    x = np.ascontiguousarray(x, np.float64)
    copies = _masked_copies(baked, nb, tags)
    out = np.full((len(w), nb), NEG)
    for j, uw in enumerate(usable(w, len(x))):
        if uw is not None:
            for b in range(nb):
                out[j, b] = orc.viterbi(copies[b], x[uw[0]:uw[1] + 1], want_path=False)[0]
    return out


def same_bits(got, want):
    got = np.ascontiguousarray(got, np.float64); want = np.ascontiguousarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------------------
# the image on the CPU
def interpret_image(image, nb, x, tags="var"):
    """nb float64: the recurrence of the kernel headers over the cell codes of an edge image (ffi.debug_variant_image /
    ffi.debug_mod_llr_image), rows in edge order: best = max_k(v_prev[src_k] + lp_k) and the start edge, v = best + emission."""
    x = np.ascontiguousarray(x, np.float64)
    out = np.full(nb, NEG)
    if len(x) == 0:
        return out
    var = tags == "var"
    pad = VAR_PAD if var else LLR_PAD
    deg, deg2 = image["deg"], image["deg2"]
    src, lp, kind, hub = image["src"][:, :deg], image["lp"][:, :deg], image["kind"], image["hub"] != 0
    ea, eb, ec = image["ea"], image["eb"], image["ec"]
    own = np.arange(128).reshape(2, 64)
    live = kind != 0
    if var:
        src2, lp2 = image["src2"][:, :, :deg2], image["lp2"][:, :, :deg2]
        slp = [image["start_lp"]] * nb
    else:
        src2, lp2 = image["src2"][None, :, :deg2], image["lp2"][None, :, :deg2]
        slp = [image["start_lp"][0], image["start_lp"][1]]
    V = np.full(pad + 1, NEG)
    for t, xt in enumerate(x):
        vstart = 0.0 if t == 0 else NEG
        d = xt - ea
        with np.errstate(invalid="ignore"):
            em = np.where(kind == 1, ec - (d * d) * eb, np.where((xt >= ea) & (xt <= eb), ec, NEG))
        if xt != xt:
            em = np.zeros((2, 64))
        new = np.full(pad + 1, NEG)
        best = np.maximum((V[src] + lp).max(axis=1, initial=NEG), vstart + slp[0])
        new[own[live]] = (best + em)[live]
        for c in range(1, nb):
            best = np.maximum((V[src2[c - 1]] + lp2[c - 1]).max(axis=1, initial=NEG), vstart + slp[c])
            new[128 * c + own[hub]] = (best + em)[hub]
        V = new
    for c in range(nb):
        k = image["end_deg"][c]
        if k:
            out[c] = (V[image["end_src"][c, :k]] + image["end_lp"][c, :k]).max()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted models
CRAFT_LO, CRAFT_HI = 50.0, 130.0          # Uniform support of the hubs of a crafted model


def crafted_model(rng, ne, nb, own_deg=5, copy_deg=3, end_deg=3, tags="var"):
    """A random baked model that keeps the structural contract of the image builders: `ne` emitting states and only start (ne) and
    end (ne + 1) silent; with ne >= nb + 2 every branch and at least two hubs tagged (below that every state is a hub: the variant
    builder refuses such a model, the dual builder takes it); Normal and Uniform emissions mixed; in-edges sorted by source, edges among
    the emitting states in any direction (their numbering is shuffled).  One branch state has `own_deg` in-edges inside its own branch
    and no state more, one hub `copy_deg` inside one further branch and none more, the end state `end_deg` in-edges from hubs and the
    base branch -- as far as the model has that many states to draw from: the degrees reached are in .degrees.  A backbone (hub 0 ->
    every state of a branch -> the next one / itself -> hub 1 -> hub 0 | end) keeps windows of three observations and more alive;
    no path emits fewer than two."""
    assert own_deg >= 3 and copy_deg >= 3 and end_deg >= 1 and ne >= 1
    edges = {}          # (src, dst) -> probability, logical numbering: hubs first, then branch 0, 1, ...

    def link(a, b):
        if (a, b) not in edges:
            edges[(a, b)] = float(rng.uniform(0.05, 1.0))
            return True
        return False

    start, end = ne, ne + 1
    if ne < nb + 2:
        hubs, members = list(range(ne)), [[] for _ in range(nb)]
        for h in hubs:
            link(start, h); link(h, end); link(h, h)
            if ne > 1:
                link(hubs[h - 1], h)
    else:
        n_hub = max(2, ne // 8)
        hubs = list(range(n_hub))
        rest = np.array_split(np.arange(n_hub, ne), nb)
        members = [[int(v) for v in part] for part in rest]
        link(start, hubs[0]); link(hubs[1], hubs[0]); link(hubs[1], end)
        for b in range(nb):
            for i, l in enumerate(members[b]):
                link(hubs[0], l); link(l, l)
                if i:
                    link(members[b][i - 1], l)
            link(members[b][-1], hubs[1])
        for k, h in enumerate(hubs[2:]):
            link(hubs[0], h); link(h, h)
            if k == 0:
                link(h, hubs[1])
    br = np.full(ne, HUB, np.int64)
    for b in range(nb):
        br[members[b]] = b

    def own_count(l):          # in-edges of l that survive in its own value (copy 0 of a hub)
        keep = 0 if br[l] == HUB else br[l]
        return sum(1 for (a, d) in edges if d == l and a < ne and (br[a] == HUB or br[a] == keep))

    def copy_count(l, c):
        return sum(1 for (a, d) in edges if d == l and a < ne and (br[a] == HUB or br[a] == c))

    def top_up(l, pool, count, want):
        pool = [int(a) for a in rng.permutation(pool)]
        while count() < want and pool:
            link(pool.pop(), l)

    if ne >= nb + 2:
        soft = min(own_deg, 5)
        for b in range(nb):
            for l in members[b]:
                top_up(l, hubs + members[b], lambda: own_count(l), int(rng.integers(own_count(l), soft + 1)))
        for h in hubs:          # a source or none from every branch into the hub's copy of it
            for c in range(nb):
                if rng.random() < 0.5 and (own_count(h) < min(own_deg, 3) if c == 0 else copy_count(h, c) < 3):
                    link(int(rng.choice(members[c])), h)
        # the three degrees the caller asked for
        b_big = max(range(nb), key=lambda b: len(members[b]))
        l_big = int(rng.choice(members[b_big]))
        top_up(l_big, hubs + members[b_big], lambda: own_count(l_big), own_deg)
        c_big = int(rng.integers(1, nb))
        top_up(hubs[1], members[c_big], lambda: copy_count(hubs[1], c_big), copy_deg)
        n_end = lambda: sum(1 for (a, d) in edges if d == end)
        for pool in [hubs[1:], members[0]] + members[1:]:          # (not hub 0: the start state leads there)
            top_up(end, pool, n_end, end_deg)
        late = [l for part in members[1:] for l in part]          # further ways in from the start state (none of them next to the end state)
        for l in rng.choice(late, size=min(3, len(late)), replace=False):
            link(start, int(l))
    # shuffled numbering, CSR by destination with ascending sources
    perm = np.concatenate([rng.permutation(ne), [start, end]]).astype(np.int64)          # logical -> final
    n_states = ne + 2
    ins = [[] for _ in range(n_states)]
    for (a, d), p in edges.items():
        ins[perm[d]].append((int(perm[a]), float(np.log(p))))
    in_ptr = np.zeros(n_states + 1, np.int32); in_src, in_logp = [], []
    for l in range(n_states):
        ins[l].sort()
        in_ptr[l + 1] = in_ptr[l] + len(ins[l])
        in_src += [s for s, _ in ins[l]]; in_logp += [p for _, p in ins[l]]
    tag = np.zeros(n_states, np.int32); kind = np.zeros(n_states, np.int32)
    ea, eb, ec = np.zeros(n_states), np.zeros(n_states), np.zeros(n_states)
    for l in range(ne):
        f = perm[l]
        tag[f] = 2 if br[l] == HUB else _TAG[tags][br[l]]
        if br[l] == HUB or rng.random() < 0.2:
            lo, hi = (CRAFT_LO, CRAFT_HI) if br[l] == HUB else (CRAFT_LO + float(rng.uniform(0, 10)), CRAFT_HI - float(rng.uniform(0, 10)))
            kind[f], ea[f], eb[f], ec[f] = 2, lo, hi, -np.log(hi - lo)
        else:
            sd = float(rng.uniform(1.0, 4.0))
            kind[f], ea[f], eb[f], ec[f] = 1, float(rng.uniform(60, 120)), 1.0 / (2.0 * sd * sd), -np.log(sd * 2.50662827463)
    m = types.SimpleNamespace(n_states=n_states, silent_start=ne, start=start, end=end, in_ptr=in_ptr, in_src=np.array(in_src, np.int32),
                              in_logp=np.array(in_logp, np.float64), emis_kind=kind, emis_a=ea, emis_b=eb, emis_c=ec,
                              count_inc=np.zeros(n_states, np.int32), tag=tag, model_min=CRAFT_LO, model_max=CRAFT_HI)
    own = max([own_count(l) for l in range(ne) if br[l] != HUB] + [0])
    m.degrees = dict(own=own, own_hub=max(own_count(h) for h in hubs),
                     copy=max([copy_count(h, c) for h in hubs for c in range(1, nb)] + [0]),
                     end=sum(1 for (a, d) in edges if d == end), hubs=[int(perm[h]) for h in hubs])
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# windows and bounds
def signal(rng, n, lo, hi):
    """n observations inside (lo, hi)."""
    return lo + (hi - lo) * rng.uniform(0.02, 0.98, size=n)


def host_windows(rng, lo, hi):
    """[(name, x)] of the windows the host test interprets: in-range signal of every length of SHORT and LONG, every fifth
    observation missing, a first observation (a hub's: every path starts in one) just outside the support, observations exactly at
    its two ends."""
    out = [("len%d" % n, signal(rng, n, lo, hi)) for n in SHORT + LONG]
    x = signal(rng, 64, lo, hi); x[::5] = np.nan
    out.append(("nan5", x))
    x = signal(rng, 40, lo, hi); x[0] = np.nextafter(hi, np.inf)
    out.append(("outside_hi", x))
    x = signal(rng, 40, lo, hi); x[0] = np.nextafter(lo, -np.inf)
    out.append(("outside_lo", x))
    x = signal(rng, 40, lo, hi); x[0] = lo; x[-1] = hi
    out.append(("ends_lo_hi", x))
    x = signal(rng, 40, lo, hi); x[0] = hi; x[-1] = lo
    out.append(("ends_hi_lo", x))
    return out


def instance_lengths(W):
    """Passage lengths around the chunk of W observations the time loop of a score kernel works in."""
    return [3, 4, 5, 8, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 150]


def bounds_of(lengths):
    """w of consecutive passages of these lengths from observation 0 on."""
    return (np.cumsum(lengths) - 1).astype(np.int32)


def hub_records(T, ps):
    """(T + 1 hub records, index of the last one) of the passages [(u, w, branch)] of a decode: record w + 1 belongs to the e0
    emission at observation w -- the record index of the e0 emission before it in the low word, the branch in the high word."""
    rec = np.zeros(T + 1, np.uint64)
    prev = 0
    for _, w, b in ps:
        rec[w + 1] = (int(b) << 32) | prev
        prev = w + 1
    return rec, prev


def path_with_ends(ends, T, s0, e0, inner):
    """A state path of T observations whose passages end (their e0 emission) at the observations `ends`: s0 right behind the e0
    before, states of inner[j % len(inner)] (one branch each) in between, e0 / s0 alternating behind the last one."""
    path = np.zeros(T, np.int32)
    t = 0
    for j, w in enumerate(ends):
        assert w - t >= 2
        states = inner[j % len(inner)]
        path[t] = s0
        for k in range(t + 1, w):
            path[k] = states[(k - t - 1) % len(states)]
        path[w] = e0
        t = w + 1
    for k in range(t, T):
        path[k] = s0 if (k - t) % 2 == 0 else e0
    return path
