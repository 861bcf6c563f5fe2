"""The step of the two-flank screen kernels (csrc/screen_kernels.hip: Screen2) at the edges of its full path.

The coarse kernel (align_screen3_kernel) takes the maximum of a FULL chunk -- 64 steps none of whose lanes needs a predicate: from
step 64 on, while 2 (t0s + 64) <= n -- from one sample per group of CMG steps (the last row at the group's last column minus the
potential of its first); every other chunk, and the fine kernel (align_screen1_kernel), take every column.  Checked on the dumped
chunk values (STRQ_SCREEN_DUMP), against the float64 last row of the exact DP (an upper bound of it) and against the numpy
restatement of the kernel's own integer recurrence (tests/screen_step_ref.py): never below the per-column rule, at most
(2 CMG - 1) hh above it, equal to the grouped rule -- for reads that end right at, before and behind the first full chunk, ragged
tails of 1 and 127 columns, a read of several cold-started pieces (alone in its call: beside short reads it would be one), and
occurrences whose best column is the first / last column of a group and of a chunk, for both flanks (their last lanes differ, so their chunks are skewed differently).  The alignments
return the oracle's bits.  Fine mode: the dumped values are the per-column restatement's, integer for integer."""
import numpy as np
import pytest

import screen_step_ref as ref
from test_gpu_screen import _exact_last_row, _read_dump

pytestmark = pytest.mark.gpu

CMG = 2              # STRQ_SCREEN3_CMG of csrc/screen_kernels.hip
COARSE = dict(sc=512, merge=3)
LVAL = (40 + 0.45 * np.arange(256)).astype(np.float32)


def _levels_of(classes):
    return np.clip(np.round((classes - 40) / 0.45), 0, 255).astype(np.uint8)


def _background(rng, n):
    return np.repeat(rng.integers(30, 200, n // 3 + 1), rng.integers(3, 10, n // 3 + 1))[:n].astype(np.uint8)


def _run(orc, monkeypatch, tmp_path, mode, reads, cls_a, cls_b):
    """Both flank alignments of every read through a fresh context (its first call cuts pieces with an 8192-column overlap: reads below
    16 k columns are one piece) with the screen forced on; returns the dump and checks the results against the oracle."""
    from conftest import oracle_map
    from strique_amd import ffi
    params = orc.align_params(None)
    fa, fb = np.repeat(cls_a, 6), np.repeat(cls_b, 6)
    monkeypatch.setenv("STRQ_SCREEN_MIN_N", "0")
    monkeypatch.setenv("STRQ_SCREEN_MODE", mode)
    dump = str(tmp_path / "screen_step.bin")
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
        got = c.align_batch(np.concatenate(reads), roff, np.tile(LVAL, (nr, 1)), np.repeat(np.arange(nr, dtype=np.int32), 2), flanks, foff)
        s = c.last_screen()
    finally:
        c.close()
    assert s["mode"] == mode and s["screened"] == 2 * nr, s
    d = _read_dump(dump)
    assert len(d["groups"]) == 2 * nr and d["mode"] == 2
    want = oracle_map(lambda job: orc.align_overlap(LVAL[reads[job[0]]], (fa, fb)[job[1]], params, want_idx=False), [(i, f) for i in range(nr) for f in range(2)])
    for a, o in enumerate(want):
        assert np.float32(o[0]).tobytes() == np.float32(got[0][a]).tobytes(), a
        assert (o[4], o[5]) == (int(got[1][a]), int(got[2][a])), a
        assert np.array_equal(o[3], got[3][foff[a]:foff[a + 1]]), a
    return d, params


def _check_dump(d, params, reads, cls_a, cls_b, sc, merge, cmg, exact_for=None):
    """Every chunk value of the dump against the restatement (and, for the reads in `exact_for`, against the exact last row).
    Returns (full chunks, full chunks whose value differs from the per-column one, chunks compared with the exact row)."""
    assert d["sc"] == sc
    hh, v = d["hh"], d["v"]
    n_full = n_differ = n_exact = 0
    for g in d["groups"]:
        r, f = g["a"] // 2, g["a"] % 2
        cls = (cls_a, cls_b)[f]
        lv = reads[r]
        m = 6 * len(cls)
        lM = g["lane_last"]
        assert lM == f * 32 + (len(cls) - 1) // 5
        exact = _exact_last_row(LVAL[lv], np.repeat(cls, 6), params) if exact_for is None or r in exact_for else None
        for pc in g["pieces"]:
            if pc["n"] <= 0:
                continue
            n, off = pc["n"], pc["col_off"]
            T = ref.last_row(LVAL[lv[off:off + n]], cls, params, sc, hh, v, merge)
            per_column = ref.chunk_values(T, hh, lM, len(pc["vals"]))
            grouped = ref.chunk_values(T, hh, lM, len(pc["vals"]), cmg)
            x = pc["vals"].astype(np.int64)
            print("read %d flank %d piece at %d, %d columns: %d chunks, %d above the per-column value, largest excess %d (allowed %d)"
                  % (r, f, off, n, len(x), int((x > per_column).sum()), int((x - per_column).max()), (2 * cmg - 1) * hh if cmg > 1 else 0))
            assert np.all(x >= per_column), (g["a"], off)
            assert np.all(x <= per_column + (2 * cmg - 1) * hh * (cmg > 1)), (g["a"], off)
            assert np.array_equal(x, grouped), (g["a"], off)
            for c in range(len(x)):
                if ref.is_full(c, n):
                    n_full += 1
                    n_differ += int(x[c] != per_column[c])
                elif cmg > 1:
                    assert x[c] == per_column[c], (g["a"], off, c)          # the predicated path keeps the per-column rule
                lo, hi = ref.chunk_columns(c, lM, n)
                if exact is None or hi < lo:
                    continue
                ub = (int(x[c]) - m * v) / sc
                ex = exact[off + lo:off + hi + 1].max()
                # cold-started pieces: a bound of the whole matrix only above the score their overlap was sized for, and only behind
                # their overlap zone (8192 columns in the first call of a context)
                if ex * sc >= g["bound"] and (off == 0 or lo > 8192):
                    assert ub >= ex - 1e-3, (g["a"], off, c, ub, ex)
                    n_exact += 1
        if exact is not None:
            assert exact.max() <= g["win"]["upper"]
    return n_full, n_differ, n_exact


def _edge_reads(rng):
    """Pieces at the edges of the full path: 256 columns is the shortest with a full chunk (chunk 1: 2 (64 + 64) <= n), 384 the
    shortest with two; 385 / 511 leave a ragged tail of 1 / 127 columns behind them."""
    return [_background(rng, n) for n in (255, 256, 257, 385, 511)]


@pytest.mark.parametrize("ka,kb", [(145, 145), (100, 140)])
def test_coarse_chunk_values_at_the_edges_of_the_full_path(orc, monkeypatch, tmp_path, ka, kb):
    rng = np.random.default_rng(7000 + ka)
    cls_a = rng.uniform(60, 120, ka).astype(np.float32); cls_b = rng.uniform(60, 120, kb).astype(np.float32)
    reads = _edge_reads(rng)
    d, params = _run(orc, monkeypatch, tmp_path, "coarse", reads, cls_a, cls_b)
    n_full, n_differ, n_exact = _check_dump(d, params, reads, cls_a, cls_b, COARSE["sc"], COARSE["merge"], CMG)
    # full chunks per alignment: 255 -> 0, 256 / 257 -> 1, 385 / 511 -> 2
    assert n_full == 2 * (0 + 1 + 1 + 2 + 2)
    assert n_differ > 0
    assert n_exact > 20


def test_coarse_chunk_values_over_several_pieces(orc, monkeypatch, tmp_path):
    """60 000 columns are cut into several cold-started pieces: every piece starts with a predicated chunk and ends ragged."""
    rng = np.random.default_rng(7060)
    cls_a = rng.uniform(60, 120, 145).astype(np.float32); cls_b = rng.uniform(60, 120, 145).astype(np.float32)
    reads = [_background(rng, 60000)]
    # an occurrence of each flank: inside a piece, and near a seam
    for cls, p in ((cls_a, 21000), (cls_b, 29000)):
        emb = np.repeat(_levels_of(cls), rng.integers(6, 10, len(cls)))
        reads[0][p:p + len(emb)] = emb
    d, params = _run(orc, monkeypatch, tmp_path, "coarse", reads, cls_a, cls_b)
    for g in d["groups"]:
        assert sum(pc["n"] > 0 for pc in g["pieces"]) > 1
    n_full, n_differ, n_exact = _check_dump(d, params, reads, cls_a, cls_b, COARSE["sc"], COARSE["merge"], CMG)
    assert n_full > 800 and n_differ > 0 and n_exact > 500


def _place(rng, n, cls, lane, chunk, kind, sc, hh, v, params, lv):
    """Plants an occurrence of `cls` into lv so that the best column of `chunk` (as `lane` sees it) is the first / last column of a
    group or of the chunk -- moved until the restatement's per-column values say so.  Groups of eight columns (CMG = 4) start and end
    groups of four (CMG = 2) as well."""
    lo, hi = ref.chunk_columns(chunk, lane, n)
    target = {"group_first": lo + 8 * 5, "group_last": lo + 8 * 5 + 7, "chunk_first": lo, "chunk_last": hi}[kind]
    emb = np.repeat(_levels_of(cls), rng.integers(6, 10, len(cls)))
    clean = lv[max(0, lo - 3000):hi + 200].copy()
    p = target - len(emb)
    for _ in range(6):
        lv[max(0, lo - 3000):hi + 200] = clean
        lv[p:p + len(emb)] = emb
        T = ref.last_row(LVAL[lv], cls, params, sc, hh, v, COARSE["merge"])
        dec = T - np.arange(n + 1, dtype=np.int64) * hh
        best = int(dec.argmax())          # the end of the planted occurrence: nothing else in the read scores as high
        if best == target:
            return
        p += target - best
    raise AssertionError("could not place the occurrence: %s" % kind)


def test_coarse_chunk_values_with_the_best_column_at_group_and_chunk_edges(orc, monkeypatch, tmp_path):
    rng = np.random.default_rng(7345)
    ka, kb = 145, 140
    cls_a = rng.uniform(60, 120, ka).astype(np.float32); cls_b = rng.uniform(60, 120, kb).astype(np.float32)
    params = orc.align_params(None)
    sc, hh, v = COARSE["sc"], 512, 16 * 512
    n = 6000
    kinds = ("group_first", "group_last", "chunk_first", "chunk_last")
    reads = []
    for kind in kinds:
        lv = _background(rng, n)
        _place(rng, n, cls_a, (ka - 1) // 5, 17, kind, sc, hh, v, params, lv)
        _place(rng, n, cls_b, 32 + (kb - 1) // 5, 40, kind, sc, hh, v, params, lv)
        reads.append(lv)
    d, params = _run(orc, monkeypatch, tmp_path, "coarse", reads, cls_a, cls_b)
    assert d["hh"] == hh and d["v"] == v
    for g in d["groups"]:
        live = [pc for pc in g["pieces"] if pc["n"] > 0]
        assert len(live) == 1 and live[0]["n"] == n and live[0]["col_off"] == 0          # what _place planned for
    n_full, n_differ, n_exact = _check_dump(d, params, reads, cls_a, cls_b, sc, COARSE["merge"], CMG)
    assert n_full > 300 and n_differ > 0 and n_exact > 300


def test_fine_chunk_values_are_the_per_column_rule(orc, monkeypatch, tmp_path):
    """align_screen1_kernel shares the step: its values are those of the per-column rule, integer for integer (the restatement is
    exact there: one DP row per flank row, every column sampled)."""
    rng = np.random.default_rng(7100)
    cls_a = rng.uniform(60, 120, 145).astype(np.float32); cls_b = rng.uniform(60, 120, 130).astype(np.float32)
    reads = _edge_reads(rng) + [_background(rng, 3000)]
    emb = np.repeat(_levels_of(cls_a), rng.integers(6, 10, len(cls_a)))
    reads[-1][1200:1200 + len(emb)] = emb
    d, params = _run(orc, monkeypatch, tmp_path, "fine", reads, cls_a, cls_b)
    n_full, n_differ, n_exact = _check_dump(d, params, reads, cls_a, cls_b, 1024, 1, 1)
    assert n_full > 40 and n_differ == 0 and n_exact > 80          # 43 chunks per flank, one of them without columns
