"""Case lists of tests/test_gpu_tables.py and a plain restatement of what the score-table kernel (csrc/lut_kernels.hip) decides
for them: which rows a table has, which of its entries are "borderline" and where those sit.  No GPU, nothing of the product:
numpy, the C library's pow through ctypes, and the oracle's strq_oracle_cell_score.  tests/test_table_cases_host.py counts the
kinds of cases these lists reach.

A table entry is the score of one (class value c, level value v) pair: max(dist_offset - (float)pow((double)|v - c|, 1.2), dist_min).
The kernel evaluates pow on the device and lists an entry for the host when the 29 bits the float cast drops lie within 64 of the
rounding midpoint 0x10000000 -- unless both candidate floats clip to dist_min.  The model below uses the HOST pow and two windows:
`sure` (+-32: a device pow up to 32 ulp away from the host's still flags the entry) and `gray` (+-96: an entry outside it is not
flagged by such a pow).  The case lists keep the two sets equal, which makes what the kernel must report a function of the case.

Borderline float32 distances are rare (a chance of 65 / 2^29 each), so the cases are built from the list below -- found by
tools/find_borderline_distances.py, all positive float32 below 10.08, 262 of them (7 in [0.5, 8), 214 below 2^-20) -- with a class
at 0.0, where the distance is the level value itself.  None exists among the differences of pA values in 64 ... 128.
"""
import ctypes
import ctypes.util
from collections import namedtuple

import numpy as np

SURE, GRAY, KERNEL_WINDOW, LOCAL_HARD, MAX_K = 32, 96, 64, 64, 158

BORDERLINE_BITS = [
    0x0057c30a, 0x006264ec, 0x0070d5f6, 0x00809434, 0x008e5f8b, 0x012d5288, 0x016bebd1, 0x01c3b617, 0x0246dd8d, 0x0250978a,
    0x02af8614, 0x02c4c9d8, 0x02e1abec, 0x03009434, 0x03ad5288, 0x03ebebd1, 0x0443b617, 0x04c6dd8d, 0x04d0978a, 0x052f8614,
    0x0544c9d8, 0x0561abec, 0x05809434, 0x062d5288, 0x066bebd1, 0x06c3b617, 0x0746dd8d, 0x0750978a, 0x07af8614, 0x07c4c9d8,
    0x07e1abec, 0x08009434, 0x08ad5288, 0x08ebebd1, 0x0943b617, 0x09c6dd8d, 0x09d0978a, 0x0a2f8614, 0x0a44c9d8, 0x0a61abec,
    0x0a809434, 0x0b2d5288, 0x0b6bebd1, 0x0bc3b617, 0x0c46dd8d, 0x0c50978a, 0x0caf8614, 0x0cc4c9d8, 0x0ce1abec, 0x0d009434,
    0x0dad5288, 0x0debebd1, 0x0e434fff, 0x0e435001, 0x0e43b617, 0x0ec6dd8d, 0x0ed0978a, 0x0f2f8614, 0x0f44c9d8, 0x0f61abec,
    0x0f809434, 0x102d5288, 0x106bebd1, 0x10c34fff, 0x10c35001, 0x10c3b617, 0x1146dd8d, 0x1150978a, 0x11af8614, 0x11e1abec,
    0x12009434, 0x12ad5288, 0x12ebebd1, 0x13434fff, 0x13435001, 0x1343b617, 0x13c6dd8d, 0x13d0978a, 0x142f8614, 0x1461abec,
    0x14809434, 0x152d5288, 0x156bebd1, 0x15c34fff, 0x15c35001, 0x15c3b617, 0x1646dd8d, 0x1650978a, 0x16af8614, 0x16e1abec,
    0x17009434, 0x17ad5288, 0x17ebebd1, 0x18434fff, 0x18435001, 0x1843b617, 0x18c6dd8d, 0x18d0978a, 0x192f8614, 0x1961abec,
    0x19809434, 0x1a2d5288, 0x1a6bebd1, 0x1ac34fff, 0x1ac35001, 0x1ac3b617, 0x1b46dd8d, 0x1b50978a, 0x1baf8614, 0x1be1abec,
    0x1c009434, 0x1cad5288, 0x1cebebd1, 0x1d434fff, 0x1d435001, 0x1d43b617, 0x1dc6dd8d, 0x1dd0978a, 0x1e2f8614, 0x1e61abec,
    0x1e809434, 0x1f2d5288, 0x1f6bebd1, 0x1fc34fff, 0x1fc35001, 0x1fc3b617, 0x2046dd8d, 0x2050978a, 0x20af8614, 0x20e1abec,
    0x21009434, 0x21ad5288, 0x21ebebd1, 0x22434fff, 0x22435001, 0x2243b617, 0x22c6dd8d, 0x22d0978a, 0x232f8614, 0x2361abec,
    0x23809434, 0x242d5288, 0x246bebd1, 0x24c34fff, 0x24c35001, 0x24c3b617, 0x2546dd8d, 0x2550978a, 0x25af8614, 0x25e1abec,
    0x26009434, 0x26ad5288, 0x26ebebd1, 0x27434fff, 0x27435001, 0x2743b617, 0x27c6dd8d, 0x27d0978a, 0x282f8614, 0x2861abec,
    0x28809434, 0x292d5288, 0x296bebd1, 0x29c34fff, 0x29c35001, 0x29c3b617, 0x2a46dd8d, 0x2a50978a, 0x2aaf8614, 0x2ae1abec,
    0x2b009434, 0x2bad5288, 0x2bebebd1, 0x2c434fff, 0x2c435001, 0x2c43b617, 0x2cc6dd8d, 0x2cd0978a, 0x2d2f8614, 0x2d61abec,
    0x2d809434, 0x2e2d5288, 0x2e6bebd1, 0x2ec34fff, 0x2ec35001, 0x2ec3b617, 0x2f46dd8d, 0x2f50978a, 0x2fa09c02, 0x2faf8614,
    0x2fe1abec, 0x30009434, 0x30ad5288, 0x30ebebd1, 0x31434fff, 0x31435001, 0x3143b617, 0x31c6dd8d, 0x31d0978a, 0x32209c02,
    0x322f8614, 0x3261abec, 0x32809434, 0x332d5288, 0x336bebd1, 0x33c34fff, 0x33c35001, 0x33c3b617, 0x3446dd8d, 0x3450978a,
    0x34a09c02, 0x34af8614, 0x34e1abec, 0x35009434, 0x35ad5288, 0x35ebebd1, 0x36434fff, 0x36435001, 0x3643b617, 0x36c6dd8d,
    0x36d0978a, 0x37209c02, 0x372f8614, 0x3761abec, 0x382d5288, 0x386bebd1, 0x38c34fff, 0x38c35001, 0x38c3b617, 0x3946dd8d,
    0x3950978a, 0x39a09c02, 0x39af8614, 0x39e1abec, 0x3aad5288, 0x3aebebd1, 0x3b434fff, 0x3b435001, 0x3b43b617, 0x3bc6dd8d,
    0x3bd0978a, 0x3c209c02, 0x3c2f8614, 0x3c61abec, 0x3d2d5288, 0x3d6bebd1, 0x3dc34fff, 0x3dc35001, 0x3dc3b617, 0x3e46dd8d,
    0x3e50978a, 0x3ea09c02, 0x3eaf8614, 0x3ee1abec, 0x3fad5288, 0x3febebd1, 0x40434fff, 0x40435001, 0x4043b617, 0x40c6dd8d,
    0x40d0978a, 0x41209c02,
]

P0 = (-1.0, -1.0, -16.0, -16.0, 16.0, 0.0)          # STRique's alignment parameters (scripts/STRique.py:507-513)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
_cell = None


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def bits_of(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


BORDERLINE = f32(BORDERLINE_BITS)                    # ascending
D_CENTRE = f32(0x3d2d5288)                           # 0.0423...: fits between two levels of a 0.05 ramp around 0
D_INTERIOR = f32(0x3fad5288)                         # 1.354...
D_EDGE = f32(0x41209c02)                             # 10.038...: pow = 15.9..., rounded UP to float (low bits +22)


def c_pow12(d):
    """pow((double)d, 1.2) with the C library's pow for every float32 of d, and the distance of the 29 bits a float cast drops
    from the rounding midpoint."""
    d = np.ascontiguousarray(d, np.float32).ravel().astype(np.float64)
    p = _libm.pow
    y = np.array([p(x, 1.2) for x in d.tolist()], np.float64)
    return y, (y.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64) - 0x10000000


def scores(params, v, c):
    """strq_oracle_cell_score for every (class, level): float32[k, 256]."""
    global _cell
    if _cell is None:
        from oracle import strique_oracle
        lib = ctypes.CDLL(strique_oracle.lib()._name)          # a handle of its own: argtypes set here stay here
        lib.strq_oracle_cell_score.restype = ctypes.c_float
        lib.strq_oracle_cell_score.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_float]
        _cell = lib.strq_oracle_cell_score
    p = np.ascontiguousarray(params, np.float32)
    pp, f = p.ctypes.data, _cell
    vl = [float(x) for x in np.asarray(v, np.float32)]
    rows = {}
    for b, cv in zip(bits_of(c).tolist(), np.asarray(c, np.float32).tolist()):
        if b not in rows:
            rows[b] = [f(pp, h, cv) for h in vl]
    return np.array([rows[b] for b in bits_of(c).tolist()], np.float32)


Model = namedtuple("Model", "rebuilt why scores best el er dup n_hard packed sure gray where determinate")


def _flagged(y, low, off, dmin, window):
    """cell_score_dev's `hard`, with the host's pow: close to the midpoint, and not clipped whichever way the cast goes."""
    if abs(int(low)) > window:
        return False
    x = np.float32(y)
    xb = int(np.array([x], np.float32).view(np.uint32)[0])
    x2 = f32(xb + 1 if float(x) < float(y) else (xb - 1 if xb else 0))
    s, s2 = np.float32(off - x), np.float32(off - x2)
    return bool(s > dmin) or bool(s2 > dmin)


def model(params, v, c):
    """What lut_build_kernel + the host make of one table.  `sure` / `gray`: {(class, level): position} of the borderline entries at
    the two windows, position one of 'centre' (the level nearest the class: the kernel gives the table up), 'edge' (a clipped
    edge entry: likewise), 'interior' (listed for the host and patched) and 'duplicate' (an entry of a class that shares the row
    of an earlier class with the same bits: evaluated once, for the first)."""
    v = np.ascontiguousarray(v, np.float32); c = np.ascontiguousarray(c, np.float32)
    k = len(c)
    assert v.shape == (256,) and 1 <= k <= MAX_K
    off, dmin = np.float32(params[4]), np.float32(params[5])
    S = scores(params, v, c)
    with np.errstate(invalid="ignore"):
        monotone = bool(np.all(v[:-1] <= v[1:]))
    if not monotone:
        return Model(True, "levels", S, None, np.zeros(k, int), np.full(k, 255), None, -1, 0, {}, {}, set(), True)
    vb = bits_of(v)
    ne = np.nonzero(vb != vb[0])[0]
    plat_lo = int(ne.min()) - 1 if len(ne) else 255
    ne = np.nonzero(vb != vb[255])[0]
    plat_hi = int(ne.max()) + 1 if len(ne) else 0
    if plat_hi < plat_lo:                                     # every level has the same bits: one entry per row
        plat_hi = plat_lo
    best = np.zeros(k, int); el = np.zeros(k, int); er = np.zeros(k, int); clip_l = np.zeros(k, bool); clip_r = np.zeros(k, bool)
    for x in range(k):
        cv = c[x]
        a = int(np.searchsorted(v, cv, "left"))
        b = a if a < 256 else 255
        if 0 < a < 256 and np.float32(cv - v[a - 1]) <= np.float32(v[a] - cv):
            b = a - 1
        inb = S[x] > dmin
        lo, hi = 256, -1
        if inb[b]:
            p, q = 0, b
            while p < q:
                m = (p + q) >> 1
                if inb[m]: q = m
                else: p = m + 1
            lo = p
            p, q = b, 255
            while p < q:
                m = (p + q + 1) >> 1
                if inb[m]: p = m
                else: q = m - 1
            hi = p
        none = hi < lo
        best[x] = b
        el[x] = 0 if none else (plat_lo if lo <= plat_lo else lo - 1)
        er[x] = 0 if none else (plat_hi if hi >= plat_hi else hi + 1)
        clip_l[x] = none or lo > plat_lo
        clip_r[x] = none or hi < plat_hi
    cb = bits_of(c).tolist()
    dup = np.array([cb.index(b) for b in cb])
    # the pow of every entry the kernel evaluates for its `hard` flag: the stored rows and the centres
    pairs = [(x, lv) for x in range(k) for lv in sorted(set(range(el[x], er[x] + 1)) | {int(best[x])})]
    px = np.array([p[0] for p in pairs]); pl = np.array([p[1] for p in pairs])
    hv, cv = v[pl], c[px]
    d = np.where(hv > cv, hv - cv, cv - hv).astype(np.float32)
    y, low = c_pow12(d)
    sure, gray = {}, {}
    for i in np.nonzero(np.abs(low) <= GRAY)[0]:
        x, lv = pairs[i]
        for window, into in ((SURE, sure), (GRAY, gray)):
            if _flagged(y[i], low[i], off, dmin, window):
                if lv == best[x]: pos = "centre"
                elif not (el[x] <= lv <= er[x]): continue
                elif dup[x] != x: pos = "duplicate"
                elif (lv == el[x] and clip_l[x]) or (lv == er[x] and clip_r[x]): pos = "edge"
                else: pos = "interior"
                into[(x, lv)] = pos
    n_int = sum(1 for p in sure.values() if p == "interior")
    give_up = any(p in ("centre", "edge") for p in sure.values()) or n_int > LOCAL_HARD
    n_hard = -1 if give_up else n_int
    first = dup == np.arange(k)
    packed = 0
    if n_hard == 0:
        st = np.concatenate([S[x, el[x]:er[x] + 1] for x in range(k) if first[x]])
        r = st * np.float32(1048576.0)
        with np.errstate(invalid="ignore"):
            ok = (r >= 0) & (r < 16777216.0) & (r == np.floor(r)) & (bits_of(r) != 0x80000000)
        packed = int(ok.all())
    why = "centre" if "centre" in sure.values() else "edge" if "edge" in sure.values() else "count" if give_up else ""
    return Model(give_up, why, S, best, el, er, dup, n_hard, packed, sure, gray, set(sure.values()), sure == gray)


def effective(t, k):
    """The entry the forward DP reads for every (class, level) of a table as strq_debug_score_tables returns it, decoded from the
    documented layout: band_lo = e_l | (e_r - e_l) << 8 | row offset << 16, entry = table[row offset + clamp(q, e_l, e_r) - e_l].
    Returns (float32[k, 256], index[k, 256])."""
    d = t["band_lo"].astype(np.int64) & 0xFFFFFFFF
    e_l, w, ro = d & 255, (d >> 8) & 255, d >> 16
    q = np.arange(256)[None, :]
    idx = ro[:, None] + np.clip(q, e_l[:, None], (e_l + w)[:, None]) - e_l[:, None]
    assert len(d) == k and idx.min() >= 0 and idx.max() < t["entries"], (idx.min(), idx.max(), t["entries"])
    return t["table"][idx], idx


# ---- cases
Case = namedtuple("Case", "name kind params levels classes expect special")      # special: (class, level) the DP tests walk through


def ramp(lo, step):
    return (lo + step * np.arange(256)).astype(np.float32)


def _case(name, kind, params, levels, classes, special=None, **expect):
    levels = np.ascontiguousarray(levels, np.float32); classes = np.ascontiguousarray(classes, np.float32)
    assert levels.shape == (256,) and 1 <= len(classes) <= MAX_K, name
    return Case(name, kind, tuple(float(x) for x in params), levels, classes, expect, special)


def strique_like(seed, k=145, step=0.45, lo=40.0):
    rng = np.random.default_rng(seed)
    return ramp(lo, step), rng.uniform(60, 120, k).astype(np.float32)


def zero_table(seed, k, zero_at, levels, others=(0.5, 9.5)):
    """k classes, 0.0 at `zero_at`: the distance of a level from that class is the level's value."""
    rng = np.random.default_rng(seed)
    cls = rng.uniform(others[0], others[1], k).astype(np.float32)
    cls[zero_at] = 0.0
    return np.asarray(levels, np.float32), cls


def dist_min_for_edge(d=None, dist_offset=16.0):
    """The dist_min of case d: the host's score at distance D_EDGE itself."""
    d = D_EDGE if d is None else d
    y, _ = c_pow12(np.array([d], np.float32))
    return float(np.float32(dist_offset) - np.float32(y[0]))


def many_borderline(n, seed=5, k=145, zero_at=60):
    """Class 0.0 against level 0 = 0.0 (the centre), the n largest borderline distances as levels 1 ... n, and levels beyond every
    band behind them."""
    lv = np.concatenate([[0.0], BORDERLINE[len(BORDERLINE) - n:], 11.0 + 0.01 * np.arange(255 - n)]).astype(np.float32)
    return zero_table(seed, k, zero_at, lv, others=(11.2, 12.8))


def cases_a():
    lv, cl = strique_like(1)
    return [_case("a/strique", "a", P0, lv, cl, n_hard=0, packed=1)]


def _interior_levels():
    lv = ramp(-1.0, 0.05)
    lv[47] = D_INTERIOR
    return lv


def cases_b():
    lv, cl = zero_table(2, 145, 70, _interior_levels())
    return [_case("b/interior", "b", P0, lv, cl, special=(70, 47), n_hard=1, packed=0, where={"interior"})]


def batch_b():
    """Three jobs of one call; the borderline entry belongs to the last one."""
    return [_case("b/batch0", "a", P0, *strique_like(21)), _case("b/batch1", "a", P0, *strique_like(22, k=100)), cases_b()[0]]


def cases_c():
    lv = ramp(-6.0, 0.05)
    lv[120] = D_CENTRE
    lv, cl = zero_table(3, 145, 33, lv, others=(-5.0, 5.0))
    return [_case("c/centre", "c", P0, lv, cl, special=(33, 120), n_hard=-1, packed=0, where={"centre"})]


def cases_d():
    lv = ramp(-1.0, 0.05)
    lv[221] = D_EDGE
    lv, cl = zero_table(4, 145, 101, lv)
    p = P0[:5] + (dist_min_for_edge(),)
    return [_case("d/edge", "d", p, lv, cl, special=(101, 221), n_hard=-1, packed=0, where={"edge"})]


def cases_e():
    lv, cl = many_borderline(65)
    out = [_case("e/65", "e", P0, lv, cl, special=(60, 40), n_hard=-1, packed=0, where={"interior"})]
    lv, cl = many_borderline(64, k=30, zero_at=7)
    out.append(_case("e/64", "e", P0, lv, cl, special=(7, 40), n_hard=64, packed=0, where={"interior"}))
    return out


def cases_f():
    lv, cl = strique_like(6)
    cl[3] = lv[100]
    out = [_case("f/equal_bits", "f", P0, lv, cl, special=(3, 100), n_hard=0, packed=0)]
    lv, cl = strique_like(7)
    out.append(_case("f/negative_dist_min", "f", P0[:5] + (-16.0,), lv, cl, n_hard=0, packed=0))
    out.append(_case("f/offset_12.5", "f", P0[:4] + (12.5, 0.0), lv, cl, n_hard=0))
    out.append(_case("f/offset_20", "f", P0[:4] + (20.0, 0.0), lv, cl, n_hard=0))
    return out


def cases_g():
    out = []
    lv, cl = strique_like(8, k=40)
    cl[5] = cl[4]; cl[20] = cl[3]; cl[39] = cl[3]
    out.append(_case("g/duplicates", "g", P0, lv, cl, n_hard=0))
    lv, cl = zero_table(2, 145, 70, _interior_levels())
    cl[90] = 0.0                                               # the borderline entry again, in a row that is shared: listed once
    out.append(_case("g/duplicate_borderline", "g", P0, lv, cl, n_hard=1, packed=0))
    plateau = np.clip(ramp(40.0, 0.45), 55.0, 125.0).astype(np.float32)
    for k in (1, 2, 128, 157, 158):
        cl = np.random.default_rng(80 + k).uniform(50, 130, k).astype(np.float32)       # classes on, inside and beyond the plateaus
        if k >= 2:
            cl[0] = 55.0; cl[1] = 125.0
        out.append(_case("g/plateaus_k%d" % k, "g", P0, plateau, cl, n_hard=0))
    # every level with the same bits (a read clipped to one plateau): classes inside, at the edge of and beyond the band
    out.append(_case("g/constant", "g", P0, np.full(256, 90.0, np.float32), np.array([88.5, 90.0, 99.9, 100.2, 200.0, 88.5], np.float32), n_hard=0))
    return out


def cases_h():
    lv, cl = strique_like(9)
    perm = np.random.default_rng(90).permutation(256)
    out = [_case("h/permuted", "h", P0, lv[perm], cl, n_hard=-1, packed=0)]
    lv = lv.copy(); lv[77] = np.nan
    out.append(_case("h/nan_level", "h", P0, lv, cl, n_hard=-1, packed=0))
    return out


SWEEP_OFFSETS, SWEEP_MINS = (8.0, 16.0, 12.5), (0.0, -2.0, -16.0)         # the distance parameters of test_randomised_sweep


def cases_i(n=99):
    rng = np.random.default_rng(2027)
    out = []
    for it in range(n):
        k = int(rng.integers(1, MAX_K + 1)) if it >= 4 else (1, 2, 157, 158)[it]
        step = float(rng.uniform(0.05, 0.45))
        p = P0[:4] + (SWEEP_OFFSETS[it % 3], SWEEP_MINS[(it // 3) % 3])
        lo = float(rng.uniform(30, 80))
        lv = ramp(lo, step)
        if it % 5 == 0:
            lv = np.clip(lv, lo + 20 * step, lo + 230 * step).astype(np.float32)
        cl = rng.uniform(lo - 5, lo + 256 * step + 5, k).astype(np.float32)
        if k > 3 and it % 4 == 0:
            cl[k - 1] = cl[0]
        out.append(_case("i/%02d" % it, "i", p, lv, cl))
    return out


def all_cases():
    return cases_a() + cases_b() + cases_c() + cases_d() + cases_e() + cases_f() + cases_g() + cases_h() + cases_i()


_MODELS = {}


def model_of(case):
    """The model of a case, computed once per process."""
    if case.name not in _MODELS:
        _MODELS[case.name] = model(case.params, case.levels, case.classes)
    return _MODELS[case.name]


def by_params(cases):
    """Cases grouped by alignment parameters (one hook call builds the tables of one parameter set)."""
    groups = {}
    for c in cases:
        groups.setdefault(c.params, []).append(c)
    return list(groups.items())


# ---- reads for the DP tests
def read_for(case, n, seed, plant=True):
    """Levels of a read of n samples that contains the flank of `case` (runs of 6 ... 9 samples of the level nearest every class
    -- of the special level for the special class)."""
    rng = np.random.default_rng(seed)
    v, c = case.levels, case.classes
    k = len(c)
    with np.errstate(invalid="ignore"):
        dist = np.abs(v[None, :].astype(np.float64) - c[:, None])
    dist[np.isnan(dist)] = np.inf
    near = dist.argmin(axis=1)
    if case.special is not None:
        near[case.special[0]] = case.special[1]
    used = np.unique(near)
    lv = np.repeat(rng.choice(used, n // 5 + 1), rng.integers(3, 10, n // 5 + 1))[:n].astype(np.uint8)
    if plant:
        # case d's special entry scores dist_min: only a read without a spare sample keeps the best path on it
        emb = np.repeat(near.astype(np.uint8), 6 if case.kind == "d" else rng.integers(6, 10, k))
        pos = int(rng.integers(0, max(1, n - len(emb))))
        emb = emb[:max(0, n - pos)]
        lv[pos:pos + len(emb)] = emb
    return lv


def flank_of(case, samples=6):
    return np.repeat(case.classes, samples)


def crosses_special(case, lv, rec, samples=6):
    """The best path aligns a row of the special class diagonally with a sample at the special level."""
    x, q = case.special
    for row in range(samples * x, samples * (x + 1)):
        r = int(rec[row])
        if not r & 1 and r >> 1 >= 1 and lv[(r >> 1) - 1] == q:
            return True
    return False
