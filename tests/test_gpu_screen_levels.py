"""The level image of the coarse two-flank screen (csrc/screen_kernels.hip: screen2_body<.., STRQ_SCREEN_LDS_LEVELS, 8>,
csrc/screen_levels_layout.h): one LDS row per level of the span of the read's bands, byte entries at the kernel's byte
scale (6 for STRique's parameters) in units of T / 3, eight waves = eight pieces per read, STRQ_SCREEN_LDS=levels.  What leaves the
kernel is converted up to the coarse screen's usual frame (scale 512): value = ceil(value at the byte scale x 512 / 6).

On the dumped chunk values (STRQ_SCREEN_DUMP):
* every value equals the numpy restatement of the merged-row recurrence at the byte scale (tests/screen_step_ref.py), converted,
  integer for integer, and is therefore -- and is checked to be -- at least the exact last-row maximum (float64 DP of the piece's
  own columns, cold start included) of the chunk's columns;
* every value is at most the lane-major kernel's value at the same scale (STRQ_SCREEN_LDS=lanes with STRQ_SCREEN2_BYTE_SCALE=1, which
  runs that kernel in the frame of the byte scale) plus the rounding allowance rows x MERGE / sc, both converted; the frame is linear
  in MERGE, so the two are in fact equal, which is asserted too.
Reads: flanks of 145/145 and 100/145 classes; a read cut into the workgroup's eight pieces of ~300 columns (a predicated first chunk, one
full chunk, a ragged tail per piece: STRQ_OVERLAP=64 cuts that small), whose levels run from 0 to 255 -- below and above the image's
range and the band of every class of every lane --, a read of one level, single-piece reads of 255 .. 511 columns.
On rows: detect_batch of twelve reads of ~64 k samples gives byte-equal rows under levels, lanes and rows, each reporting its layout;
flanks whose bands span all 256 levels exceed the image's limit and run on the lane-major image, and strq_last_screen says so."""
import numpy as np
import pytest

import screen_step_ref as ref
from test_gpu_screen import _exact_last_row, _read_dump
from test_gpu_screen_lds_layout import CMG, CPL, LVAL, _background, _check_values, _classes, _levels_of, _screen

pytestmark = pytest.mark.gpu

SC, MERGE, SEG, MAX_ROWS = 6, 3, 8, 183          # screen_levels::byte_scale of (-1, -16, 16), MERGE, SEG, MAX_ROWS
FRAME = 512                                      # the scale of the coarse screen's chunk values (screen2_plan)


def _up(x):
    """Values at the byte scale in the frame the level-image kernel writes them in: ceil(x FRAME / SC)."""
    return -((-np.asarray(x, np.int64) * FRAME) // SC)


def _check_level_values(d, params, reads, cls_a, cls_b):
    """Every chunk value of a level-image dump against the restatement at the byte scale, converted; as _check_values otherwise."""
    assert d["sc"] == FRAME and d["hh"] == FRAME and d["v"] == 16 * FRAME and d["mode"] == 2
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
            T = ref.last_row(LVAL[reads[r][off:off + n]], cls, params, SC, SC, 16 * SC, MERGE)
            want = _up(ref.chunk_values(T, SC, lM, len(pc["vals"]), CMG))
            x = pc["vals"].astype(np.int64)
            print("read %d flank %d piece at %d, %d columns: %d chunks, %d differ from the restatement" % (r, f, off, n, len(x), int((x != want).sum())))
            assert np.array_equal(x, want), (g["a"], off)
            n_chunks += len(x)
            n_full += sum(ref.is_full(c, n) for c in range(len(x)))
    return n_chunks, n_full, live


def _inner_classes(rng, ka, kb):
    """Class values whose bands (+-10.08 units = +-22.4 levels of LVAL) stay inside levels 26 .. 196: an image of ~172 rows."""
    cls_a = rng.uniform(62, 118, ka).astype(np.float32); cls_b = rng.uniform(62, 118, kb).astype(np.float32)
    for cls in (cls_a, cls_b):
        cls[7] = cls[5]; cls[11] = cls[3]          # a k-mer repeated inside a lane and across lanes
        cls[0] = 62.0; cls[1] = 118.0              # the ends of the span
    return cls_a, cls_b


def _span(cls_a, cls_b, params):
    """Levels that score above dist_min for any class, one clipped entry at either end (csrc/lut_kernels.hip: LutInfo::lvl)."""
    inside = np.zeros(256, bool)
    for c in np.concatenate([cls_a, cls_b]):
        inside |= ref.scores(LVAL, c, params) > np.float32(params[5])
    idx = np.flatnonzero(inside)
    return max(idx[0] - 1, 0), min(idx[-1] + 1, 255)


def _bounds_exact(d, params, reads, cls_a, cls_b):
    """Every chunk value decodes to at least the exact last-row maximum of the chunk's columns (the piece's own DP)."""
    checked = 0
    for g in d["groups"]:
        r, f = g["a"] // 2, g["a"] % 2
        flank = np.repeat((cls_a, cls_b)[f], 6)
        lM = g["lane_last"]
        for pc in g["pieces"]:
            if pc["n"] <= 0:
                continue
            exact = _exact_last_row(LVAL[reads[r][pc["col_off"]:pc["col_off"] + pc["n"]]], flank, params)
            for c, x in enumerate(pc["vals"]):
                lo, hi = ref.chunk_columns(c, lM, pc["n"])
                if hi < lo:
                    continue
                ub = (int(x) - len(flank) * d["v"]) / d["sc"]
                # (a value of 0 in the dump -- nothing above the cold start's floor -- decodes to m e_v, which still bounds the row)
                ex = exact[lo:hi + 1].max()
                assert ub >= ex - 1e-6, (g["a"], pc["col_off"], c, ub, ex)
                checked += 1
    return checked


@pytest.mark.parametrize("ka,kb", [(145, 145), (100, 145)])
def test_level_image_values_bound_the_exact_row_and_match_the_lane_major_kernel(orc, monkeypatch, tmp_path, ka, kb):
    rng = np.random.default_rng(9300 + ka)
    params = orc.align_params(None)
    cls_a, cls_b = _inner_classes(rng, ka, kb)
    lvl0, lvl1 = _span(cls_a, cls_b, params)
    assert lvl1 - lvl0 + 1 <= MAX_ROWS and lvl0 > 0 and lvl1 < 255, (lvl0, lvl1)

    # --- a read in eight pieces of 300 columns (overlap 64), levels over the whole 0 .. 255; a read of one level
    monkeypatch.setenv("STRQ_OVERLAP", "64")
    n = 8 * 300 - 7 * 64
    wide = np.repeat(rng.integers(0, 256, n // 4 + 1), rng.integers(2, 7, n // 4 + 1))[:n].astype(np.uint8)
    wide[5:9] = 0; wide[40:44] = 255; wide[60] = lvl0; wide[61] = lvl1; wide[62] = lvl0 - 1; wide[63] = lvl1 + 1
    emb = np.repeat(_levels_of(cls_a[:30], LVAL), 6)
    wide[700:700 + len(emb)] = emb
    flat = np.full(n, 100, np.uint8)
    reads = [wide, flat]
    raw, path, got, s, foff = _screen(monkeypatch, tmp_path, params, "coarse", "levels", reads, cls_a, cls_b, LVAL)
    assert s["lds_layout"] == "levels" and s["scale"] == FRAME and s["byte_scale"] == SC and s["merge"] == MERGE, s
    d = _read_dump(path)
    n_chunks, n_full, live = _check_level_values(d, params, reads, cls_a, cls_b)
    assert live == [SEG] * 4 and n_full == 4 * SEG and n_chunks == 4 * SEG * 4, (live, n_full, n_chunks)
    for g in d["groups"]:
        assert all(256 < pc["n"] < 384 for pc in g["pieces"]), [pc["n"] for pc in g["pieces"]]          # one full chunk and a ragged one
    assert _bounds_exact(d, params, reads, cls_a, cls_b) > 100

    # --- single-piece reads through both kernels at the same scale
    monkeypatch.delenv("STRQ_OVERLAP")
    singles = [_background(rng, m) for m in (255, 256, 257, 511)]
    singles[1][::7] = 0; singles[2][::5] = 255
    singles[3][100:100 + len(emb)] = emb
    raw_v, path_v, got_v, s_v, _ = _screen(monkeypatch, tmp_path, params, "coarse", "levels", singles, cls_a, cls_b, LVAL)
    monkeypatch.setenv("STRQ_SCREEN2_BYTE_SCALE", "1")
    raw_l, path_l, got_l, s_l, _ = _screen(monkeypatch, tmp_path, params, "coarse", "lanes", singles, cls_a, cls_b, LVAL)
    assert s_v["lds_layout"] == "levels" and s_l["lds_layout"] == "lanes", (s_v, s_l)
    assert (s_v["scale"], s_v["byte_scale"], s_l["scale"], s_l["byte_scale"]) == (FRAME, SC, SC, 0), (s_v, s_l)
    dv, dl = _read_dump(path_v), _read_dump(path_l)
    _check_level_values(dv, params, singles, cls_a, cls_b)
    _check_values(dl, params, singles, cls_a, cls_b, LVAL, SC, MERGE, CMG)
    assert _bounds_exact(dv, params, singles, cls_a, cls_b) > 20
    allowance = 2 * CPL * 29 * MERGE          # rows x MERGE / sc score units = rows x MERGE scaled units; 290 merged rows
    worst = 0
    for gv, gl in zip(dv["groups"], dl["groups"]):
        pv = [pc for pc in gv["pieces"] if pc["n"] > 0]; pl = [pc for pc in gl["pieces"] if pc["n"] > 0]
        assert len(pv) == len(pl) == 1 and pv[0]["n"] == pl[0]["n"]
        xv, xl = pv[0]["vals"].astype(np.int64), pl[0]["vals"].astype(np.int64)
        worst = max(worst, int(np.abs(xv - _up(xl)).max()))
        assert np.all(xv <= _up(xl + allowance)), (gv["a"], int((xv - _up(xl)).max()))
        assert np.array_equal(xv, _up(xl)), gv["a"]
    print("level image against the lane-major kernel at scale %d, both in the frame of %d: largest difference %d (allowance %d at scale %d)" % (SC, FRAME, worst, allowance, SC))
    for a in range(len(got_v[0])):
        assert np.float32(got_v[0][a]).tobytes() == np.float32(got_l[0][a]).tobytes()


def test_an_image_over_the_limit_runs_on_the_lane_major_kernel(orc, monkeypatch, tmp_path):
    """Classes within a few levels of level 0 and of level 255: the span of the bands is all 256 levels, more rows than the image may
    have -- the call that asks for the level image runs the lane-major kernel at its own scale and says so."""
    rng = np.random.default_rng(9400)
    params = orc.align_params(None)
    cls_a, cls_b = _classes(rng, 145, 100)
    lvl0, lvl1 = _span(cls_a, cls_b, params)
    assert lvl1 - lvl0 + 1 > MAX_ROWS
    reads = [_background(rng, m) for m in (257, 700)]
    raw, path, got, s, foff = _screen(monkeypatch, tmp_path, params, "coarse", "levels", reads, cls_a, cls_b, LVAL)
    assert s["lds_layout"] == "lanes" and s["scale"] == 512 and s["merge"] == MERGE, s
    d = _read_dump(path)
    _check_values(d, params, reads, cls_a, cls_b, LVAL, 512, MERGE, CMG)


def test_detect_rows_are_the_same_under_the_three_layouts(pm, cfg, targets, monkeypatch):
    from strique_amd import synth
    from strique_amd.counter import repeatCounter
    table = synth.KmerTable(pm)
    nreps = [(20, 50, 100, 200, 300)[i % 5] for i in range(12)]
    made = [synth.make_read(table, 3, i, 8800, targets["c9orf72"], nreps[i]) for i in range(12)]          # the benchmark's recipe, ~64 k samples each
    sigs, strands = [m[0] for m in made], [m[1] for m in made]
    assert min(len(s) for s in sigs) > 40000 and set(strands) == {"+", "-"}
    rows = {}
    for layout in ("levels", "lanes", "rows"):
        monkeypatch.setenv("STRQ_SCREEN_LDS", layout)
        rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
        rc.add_target("c9orf72", *targets["c9orf72"])
        try:
            rows[layout] = rc.detect_batch([("c9orf72", s, st) for s, st in zip(sigs, strands)])
            scr = rc.ctx.last_screen()
        finally:
            rc.ctx.close()
        assert scr["mode"] == "coarse" and scr["lds_layout"] == layout and scr["screened"] == 24, (layout, scr)
        assert scr["scale"] == FRAME and scr["byte_scale"] == (SC if layout == "levels" else 0), scr
    for layout in ("lanes", "rows"):
        for a, b in zip(rows["levels"], rows[layout]):
            assert tuple(a[:6]) == tuple(b[:6]), (layout, a, b)
            assert all(np.float64(x).tobytes() == np.float64(y).tobytes() for x, y in zip(a[1:4], b[1:4])), (layout, a, b)
    assert all(abs(r[0] - n) <= 2 for r, n in zip(rows["levels"], nreps))
