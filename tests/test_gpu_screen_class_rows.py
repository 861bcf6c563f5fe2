"""One DP row per k-mer class on the coarse screen's level image (csrc/screen_kernels.hip: align_screen6_kernel = screen2_body<1, ..,
STRQ_SCREEN_LDS_LEVELS, 8>): the same image of byte entries as align_screen3_kernel's, stored values T / 6, potential step
hh_b / 6 = 1 at the byte scale 6, and what leaves the kernel converted up to the usual frame: ceil(x 6 512 / 6).  STRQ_SCREEN2_MERGE=6 with
STRQ_SCREEN_LDS=levels runs it on any read size.

On the dumped chunk values (STRQ_SCREEN_DUMP), with the helpers of tests/test_gpu_screen_levels.py at MERGE = 6: every value equals the
numpy restatement of the merged-row recurrence (tests/screen_step_ref.py: last_row(.., merge=6) at the byte scale), converted, integer for
integer, and is at least the exact float64 last-row maximum of its columns.  The reads are those of the level image's own test: flanks of
145/145 and 100/145 classes, a read in the workgroup's eight pieces of ~300 columns (a predicated chunk, a full one and a ragged tail per
piece) whose levels run over 0 .. 255, a read of one level, single-piece reads of 255 .. 511 columns.
On rows: detect_batch of twelve reads of ~64 k samples gives byte-equal rows with six rows per DP row, with three, and without a screen.
A loose case: flanks planted with three samples per k-mer -- a merged row matches all six of a class's rows at one column -- end in the
second look or the second round and return the oracle's bits."""
import numpy as np
import pytest

import screen_step_ref as ref
import test_gpu_screen_levels as lv3
from test_gpu_screen import _align_pairs, _check_pairs_against_the_oracle, _pair_reads, _read_dump
from test_gpu_screen_lds_layout import LVAL, _background, _levels_of, _screen

pytestmark = pytest.mark.gpu

MERGE = 6
SC, SEG, FRAME = lv3.SC, lv3.SEG, lv3.FRAME          # byte scale 6 (hh_b = 6: a multiple of 6 as well), eight pieces, scale 512 outside


@pytest.fixture
def class_rows(monkeypatch):
    """The level-image helpers restate the recurrence with their module's MERGE; the kernel is pinned to the same."""
    monkeypatch.setattr(lv3, "MERGE", MERGE)
    monkeypatch.setenv("STRQ_SCREEN2_MERGE", str(MERGE))


def _reports_class_rows(s):
    assert s["mode"] == "coarse" and s["merge"] == MERGE and s["lds_layout"] == "levels" and s["scale"] == FRAME and s["byte_scale"] == SC, s


@pytest.mark.parametrize("ka,kb", [(145, 145), (100, 145)])
def test_class_row_values_equal_the_restatement_and_bound_the_exact_row(orc, monkeypatch, tmp_path, class_rows, ka, kb):
    rng = np.random.default_rng(9300 + ka)
    params = orc.align_params(None)
    cls_a, cls_b = lv3._inner_classes(rng, ka, kb)
    lvl0, lvl1 = lv3._span(cls_a, cls_b, params)
    assert lvl1 - lvl0 + 1 <= lv3.MAX_ROWS and lvl0 > 0 and lvl1 < 255, (lvl0, lvl1)

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
    _reports_class_rows(s)
    d = _read_dump(path)
    n_chunks, n_full, live = lv3._check_level_values(d, params, reads, cls_a, cls_b)
    assert live == [SEG] * 4 and n_full == 4 * SEG and n_chunks == 4 * SEG * 4, (live, n_full, n_chunks)
    for g in d["groups"]:
        assert all(256 < pc["n"] < 384 for pc in g["pieces"]), [pc["n"] for pc in g["pieces"]]          # one full chunk and a ragged one
    assert lv3._bounds_exact(d, params, reads, cls_a, cls_b) > 100
    # the restatement is what the issue states: the chunk value of last_row(.., merge=6) at the byte scale, x 512 / 6, rounded up
    g = next(g for g in d["groups"] if g["a"] == 0)          # the wide read's prefix alignment (the groups come longest read first)
    pc = g["pieces"][3]
    T = ref.last_row(LVAL[wide[pc["col_off"]:pc["col_off"] + pc["n"]]], cls_a, params, SC, SC, 16 * SC, 6)
    want = -((-ref.chunk_values(T, SC, g["lane_last"], len(pc["vals"]), lv3.CMG) * 512) // 6)
    assert np.array_equal(pc["vals"].astype(np.int64), want)

    # --- single-piece reads
    monkeypatch.delenv("STRQ_OVERLAP")
    singles = [_background(rng, m) for m in (255, 256, 257, 511)]
    singles[1][::7] = 0; singles[2][::5] = 255
    singles[3][100:100 + len(emb)] = emb
    raw_v, path_v, got_v, s_v, _ = _screen(monkeypatch, tmp_path, params, "coarse", "levels", singles, cls_a, cls_b, LVAL)
    _reports_class_rows(s_v)
    dv = _read_dump(path_v)
    n_chunks, n_full, live = lv3._check_level_values(dv, params, singles, cls_a, cls_b)
    assert live == [1] * 8 and n_full == 2 * (0 + 1 + 1 + 2), (live, n_full)
    assert lv3._bounds_exact(dv, params, singles, cls_a, cls_b) > 20


def test_detect_rows_are_the_same_with_six_rows_three_rows_and_no_screen(pm, cfg, targets, monkeypatch):
    from strique_amd import synth
    from strique_amd.counter import repeatCounter
    table = synth.KmerTable(pm)
    nreps = [(20, 50, 100, 200, 300)[i % 5] for i in range(12)]
    made = [synth.make_read(table, 3, i, 8800, targets["c9orf72"], nreps[i]) for i in range(12)]          # the benchmark's recipe, ~64 k samples each
    sigs, strands = [m[0] for m in made], [m[1] for m in made]
    assert min(len(s) for s in sigs) > 40000 and set(strands) == {"+", "-"}
    monkeypatch.setenv("STRQ_SCREEN_LDS", "levels")          # ... with which the merge factor holds on any read size
    rows = {}
    for name, env in (("six", {"STRQ_SCREEN2_MERGE": "6"}), ("three", {"STRQ_SCREEN2_MERGE": "3"}), ("none", {"STRQ_NO_SCREEN": "1"})):
        for k in ("STRQ_SCREEN2_MERGE", "STRQ_NO_SCREEN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rc = repeatCounter(pm, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
        rc.add_target("c9orf72", *targets["c9orf72"])
        try:
            rows[name] = rc.detect_batch([("c9orf72", s, st) for s, st in zip(sigs, strands)])
            scr = rc.ctx.last_screen()
        finally:
            rc.ctx.close()
        if name == "none":
            assert scr["screened"] == 0, scr
        else:
            assert scr["mode"] == "coarse" and scr["lds_layout"] == "levels" and scr["merge"] == int(env["STRQ_SCREEN2_MERGE"]), (name, scr)
            assert scr["screened"] == 24 and scr["scale"] == FRAME and scr["byte_scale"] == SC, (name, scr)
    for name in ("three", "none"):
        for a, b in zip(rows["six"], rows[name]):
            assert tuple(a[:6]) == tuple(b[:6]), (name, a, b)
            assert all(np.float64(x).tobytes() == np.float64(y).tobytes() for x, y in zip(a[1:4], b[1:4])), (name, a, b)
    assert all(abs(r[0] - n) <= 2 for r, n in zip(rows["six"], nreps))


def test_three_samples_per_kmer_end_in_the_second_look_or_round(orc):
    """As tests/test_gpu_screen.py: test_coarse_margin_too_small_ends_in_the_second_round, on align_screen6_kernel: a merged row needs
    one column for the six rows of its class, the exact DP has to skip half of them -- the bound lies far above the exact score, the
    certificate of the first look fails, and the results are still the oracle's."""
    from strique_amd import ffi
    c = ffi.Context(0)
    try:
        params = orc.align_params(None)
        c.set_align_params(*[float(v) for v in params])
        for k, v in (("STRQ_SCREEN_MIN_N", "0"), ("STRQ_SCREEN_MODE", "coarse"), ("STRQ_SCREEN2_MARGIN", "1"), ("STRQ_SCREEN_LDS", "levels"), ("STRQ_SCREEN2_MERGE", "6")):
            c.set_option(k, v)
        rng = np.random.default_rng(77)
        n, k = 50000, 145
        reads, lval, fa, fb = _pair_reads(rng, n, k, k, [[], [], []], [[], [], []])
        for lv, pa, pb in zip(reads, (3000, 20000, 44000), (30000, 5000, 10000)):
            for flank, p in ((fa, pa), (fb, pb)):
                emb = np.repeat(np.clip(np.round((flank[::6] - 40) / 0.45), 0, 255).astype(np.uint8), 3)
                lv[p:p + len(emb)] = emb
        got, foff = _align_pairs(c, reads, lval, fa, fb)
        s, sr = c.last_screen(), c.last_second_round()
        print("second look %d, second round %d of %d alignments" % (s["second_look"], sr[0], sr[1]))
        _reports_class_rows(s)
        assert s["screened"] == 6 and s["second_look"] + sr[0] >= 1, (s, sr)
        _check_pairs_against_the_oracle(orc, params, reads, lval, fa, fb, got, foff)
    finally:
        c.close()
