"""The two LDS layouts of the two-flank screen kernels' score tables (csrc/screen_kernels.hip: screen2_body<.., LANES>, csrc/screen_lds_layout.h,
DESIGN.md 4.2e): the lane-major image (STRQ_SCREEN_LDS=lanes, the default: every lane reads its own 16-bit column, no bank conflicts)
and the class rows (STRQ_SCREEN_LDS=rows, and every launch whose image would not fit the LDS budget).  The scores, the DP and every
chunk value are the same integers in both.

Checked on the dumped chunk values (STRQ_SCREEN_DUMP) of both kernels (coarse: align_screen3_kernel, fine: align_screen1_kernel) under
both layouts: equal to the numpy restatement of the kernel's integer recurrence (tests/screen_step_ref.py) integer for integer, the
two layouts' dumps byte for byte equal, the alignments the oracle's bits -- for pieces of 255, 256, 257 and 511 columns (before, at and
behind the first full chunk, a ragged tail), flanks of 145/145 and 100/140 classes (a partly filled last lane, idle lanes), a k-mer
repeated inside one lane (one table row, two columns of the image), class values within a few levels of level 0 and of level 255
(band ends cut by the clamp), a read of several cold-started pieces, and a level map so flat that the image exceeds the LDS limit:
that call must report the class rows although the lane-major image was asked for."""
import numpy as np
import pytest

import screen_step_ref as ref
from test_gpu_screen import _read_dump

pytestmark = pytest.mark.gpu

CMG = 2                                   # STRQ_SCREEN3_CMG of csrc/screen_kernels.hip
KERNELS = {"coarse": dict(sc=512, merge=3, cmg=CMG), "fine": dict(sc=1024, merge=1, cmg=1)}
MAX_ROWS, CPL = 264, 5                    # screen_lanes::MAX_ROWS, classes per lane (csrc/screen_lds_layout.h)
LVAL = (40 + 0.45 * np.arange(256)).astype(np.float32)
LVAL_FLAT = (60 + 0.15 * np.arange(256)).astype(np.float32)          # 0.15 per level: bands three times as wide


def _levels_of(classes, lval):
    return np.abs(lval[None, :] - classes[:, None]).argmin(axis=1).astype(np.uint8)


def _background(rng, n):
    return np.repeat(rng.integers(30, 200, n // 3 + 1), rng.integers(3, 10, n // 3 + 1))[:n].astype(np.uint8)


def _band_levels(cls_a, cls_b, lval, params):
    """Levels that score above dist_min, widest class of either flank: the table's widest band holds these and at most one clipped
    entry at either end (csrc/lut_kernels.hip)."""
    return max(int((ref.scores(lval, c, params) > np.float32(params[5])).sum()) for c in np.concatenate([cls_a, cls_b]))


def _screen(monkeypatch, tmp_path, params, mode, layout, reads, cls_a, cls_b, lval):
    """Both flank alignments of every read through a fresh context (its first call cuts pieces with an 8192-column overlap: reads below
    24 k columns are one piece) with the screen forced on; returns the raw dump, the results and strq_last_screen."""
    from strique_amd import ffi
    fa, fb = np.repeat(cls_a, 6), np.repeat(cls_b, 6)
    monkeypatch.setenv("STRQ_SCREEN_MIN_N", "0")
    monkeypatch.setenv("STRQ_SCREEN_MODE", mode)
    monkeypatch.setenv("STRQ_SCREEN_LDS", layout)
    dump = str(tmp_path / ("screen_%s_%s.bin" % (mode, layout)))
    monkeypatch.setenv("STRQ_SCREEN_DUMP", dump)
    nr = len(reads)
    flanks = np.concatenate([np.concatenate([fa, fb])] * nr)
    foff = np.zeros(2 * nr + 1, np.int64)
    foff[1:] = np.cumsum([len(fa), len(fb)] * nr)
    roff = np.zeros(nr + 1, np.int64)
    roff[1:] = np.cumsum([len(r) for r in reads])
    c = ffi.Context(0)
    try:
        c.set_align_params(*[float(v) for v in params])
        got = c.align_batch(np.concatenate(reads), roff, np.tile(lval, (nr, 1)), np.repeat(np.arange(nr, dtype=np.int32), 2), flanks, foff)
        s = c.last_screen()
    finally:
        c.close()
    assert s["mode"] == mode and s["screened"] == 2 * nr, s
    return open(dump, "rb").read(), dump, got, s, foff


def _check_values(d, params, reads, cls_a, cls_b, lval, sc, merge, cmg):
    """Every chunk value of the dump against the restatement, integer for integer; returns (chunks, full chunks, live pieces per alignment)."""
    assert d["sc"] == sc and d["mode"] == 2
    hh, v = d["hh"], d["v"]
    n_chunks = n_full = 0
    live = []
    for g in d["groups"]:
        r, f = g["a"] // 2, g["a"] % 2
        cls = (cls_a, cls_b)[f]
        lM = g["lane_last"]
        assert lM == f * 32 + (len(cls) - 1) // CPL
        live.append(sum(pc["n"] > 0 for pc in g["pieces"]))
        for pc in g["pieces"]:
            if pc["n"] <= 0:
                continue
            n, off = pc["n"], pc["col_off"]
            T = ref.last_row(lval[reads[r][off:off + n]], cls, params, sc, hh, v, merge)
            want = ref.chunk_values(T, hh, lM, len(pc["vals"]), cmg)
            x = pc["vals"].astype(np.int64)
            print("read %d flank %d piece at %d, %d columns: %d chunks, %d differ from the restatement" % (r, f, off, n, len(x), int((x != want).sum())))
            assert np.array_equal(x, want), (g["a"], off)
            n_chunks += len(x)
            n_full += sum(ref.is_full(c, n) for c in range(len(x)))
    return n_chunks, n_full, live


def _both_layouts(orc, monkeypatch, tmp_path, reads, cls_a, cls_b, lval, expect_lanes):
    """Coarse and fine kernel under both layouts; `expect_lanes`: whether a call that asks for the lane-major image gets it."""
    from conftest import oracle_map
    params = orc.align_params(None)
    fa, fb = np.repeat(cls_a, 6), np.repeat(cls_b, 6)
    nr = len(reads)
    want = oracle_map(lambda job: orc.align_overlap(lval[reads[job[0]]], (fa, fb)[job[1]], params, want_idx=False), [(i, f) for i in range(nr) for f in range(2)])
    out = {}
    for mode, k in KERNELS.items():
        raws = {}
        for layout in ("lanes", "rows"):
            raw, path, got, s, foff = _screen(monkeypatch, tmp_path, params, mode, layout, reads, cls_a, cls_b, lval)
            raws[layout] = raw
            assert s["lds_layout"] == ("lanes" if layout == "lanes" and expect_lanes else "rows"), (mode, layout, s)
            assert s["merge"] == k["merge"]
            for a, o in enumerate(want):
                assert np.float32(o[0]).tobytes() == np.float32(got[0][a]).tobytes(), (mode, layout, a)
                assert (o[4], o[5]) == (int(got[1][a]), int(got[2][a])), (mode, layout, a)
                assert np.array_equal(o[3], got[3][foff[a]:foff[a + 1]]), (mode, layout, a)
            d = _read_dump(path)
            assert len(d["groups"]) == 2 * nr
            out[mode, layout] = _check_values(d, params, reads, cls_a, cls_b, lval, k["sc"], k["merge"], k["cmg"])
        assert raws["lanes"] == raws["rows"], mode
    return out, params


def _classes(rng, ka, kb):
    """Class values of both flanks: a k-mer repeated inside one lane (classes 5 and 7: lane 1) and across lanes (3 and 11), and classes
    within a few levels of level 0 (40.0) and of level 255 (154.75) of LVAL, whose bands the clamp cuts."""
    cls_a = rng.uniform(60, 120, ka).astype(np.float32); cls_b = rng.uniform(60, 120, kb).astype(np.float32)
    for cls in (cls_a, cls_b):
        if len(cls) >= 16:
            cls[7] = cls[5]; cls[11] = cls[3]
            cls[8] = 40.0; cls[9] = 41.2; cls[12] = 154.75; cls[13] = 153.1; cls[14] = 38.0; cls[15] = 157.0
    return cls_a, cls_b


@pytest.mark.parametrize("ka,kb", [(145, 145), (100, 140)])
def test_both_layouts_at_the_edges_of_the_full_path(orc, monkeypatch, tmp_path, ka, kb):
    rng = np.random.default_rng(9100 + ka)
    cls_a, cls_b = _classes(rng, ka, kb)
    reads = [_background(rng, n) for n in (255, 256, 257, 511)]
    # an occurrence of the prefix flank's start (with the classes at the ends of the level range) in the longest read
    emb = np.repeat(_levels_of(cls_a[:40], LVAL), 6)
    reads[-1][100:100 + len(emb)] = emb
    params = orc.align_params(None)
    assert 1 + CPL * (_band_levels(cls_a, cls_b, LVAL, params) + 2) <= MAX_ROWS          # the image fits whatever the clipped ends add
    out, _ = _both_layouts(orc, monkeypatch, tmp_path, reads, cls_a, cls_b, LVAL, True)
    for key, (n_chunks, n_full, live) in out.items():
        # chunks per alignment: (n + 1) / 2 + 63 steps in chunks of 64 -> 3, 3, 3, 5; full chunks: 255 -> 0, 256 / 257 -> 1, 511 -> 2
        assert n_chunks == 2 * (3 + 3 + 3 + 5) and n_full == 2 * (0 + 1 + 1 + 2), key
        assert live == [1] * 8, key


def test_both_layouts_over_several_pieces(orc, monkeypatch, tmp_path):
    """33 000 columns are cut into three cold-started pieces (a piece owns at least the 8192 columns of the overlap; waves of one
    workgroup: they share the one image)."""
    rng = np.random.default_rng(9160)
    cls_a, cls_b = _classes(rng, 145, 140)
    reads = [_background(rng, 33000)]
    for cls, p in ((cls_a, 5000), (cls_b, 20500)):
        emb = np.repeat(_levels_of(cls, LVAL), rng.integers(6, 10, len(cls)))
        reads[0][p:p + len(emb)] = emb
    out, _ = _both_layouts(orc, monkeypatch, tmp_path, reads, cls_a, cls_b, LVAL, True)
    for key, (n_chunks, n_full, live) in out.items():
        assert min(live) == 3 and n_full > 500, (key, live, n_full)


def test_flat_level_map_falls_back_to_the_class_rows(orc, monkeypatch, tmp_path):
    """0.15 units per level: the widest band alone makes a lane's column taller than the limit, so the call that asks for the
    lane-major image runs on the class rows (strq_last_screen_mode [6]) -- with the same values."""
    rng = np.random.default_rng(9200)
    cls_a = rng.uniform(63, 95, 145).astype(np.float32); cls_b = rng.uniform(63, 95, 100).astype(np.float32)
    params = orc.align_params(None)
    assert 1 + CPL * _band_levels(cls_a, cls_b, LVAL_FLAT, params) > MAX_ROWS
    reads = [_background(rng, n) for n in (257, 700)]
    emb = np.repeat(_levels_of(cls_a[:60], LVAL_FLAT), 7)
    reads[1][150:150 + len(emb)] = emb
    out, _ = _both_layouts(orc, monkeypatch, tmp_path, reads, cls_a, cls_b, LVAL_FLAT, False)
    for key, (n_chunks, n_full, live) in out.items():
        assert n_full == 2 * (1 + 4), key
