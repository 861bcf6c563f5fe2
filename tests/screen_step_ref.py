"""The two-flank screen kernels' arithmetic (csrc/screen_kernels.hip: Screen2, screen2_body), restated in numpy -- no GPU.

`last_row` is the integer recurrence of one cold-started piece: T = S sc + i |e_v| sc + j |e_h| sc, `merge` identical flank rows per
DP row whose diagonal step gains merge (ceil(s sc) + hh + v) at one column (merge = 1: the fine bound; tests/test_screen_math.py shows
the form).  `chunk_values` is what a lane writes per chunk of 64 steps (128 columns, skewed by two columns per lane): the maximum
of T - j hh over the chunk's columns ("per column": the fine kernel, and every chunk that runs the predicated path), or, in the
full chunks of the coarse kernel, over one sample per group of `cmg` steps -- the last row at the group's last column minus the
potential of its first."""
import numpy as np

SAMPLES = 6          # rows per k-mer class


def scores(vals, level, params):
    """float32 scores of one class against the read's values, as the library's table holds them (src/score_distance.h:115-122)."""
    off, dmin = np.float32(params[4]), np.float32(params[5])
    d = np.abs(vals.astype(np.float32) - np.float32(level)).astype(np.float32)
    s = off - np.power(d.astype(np.float64), 1.2).astype(np.float32)
    return np.maximum(s, dmin).astype(np.float32)


def last_row(vals, classes, params, sc, hh, v, merge):
    """T of the last DP row over the piece's columns 0 .. n (int64; column 0 and the top row start cold: S = i e_v, S = 0)."""
    n = len(vals)
    T = np.arange(n + 1, dtype=np.int64) * hh
    for level in classes:
        e = merge * (np.ceil(scores(vals, level, params).astype(np.float64) * sc).astype(np.int64) + hh + v)
        for _ in range(SAMPLES // merge):
            cur = np.empty(n + 1, np.int64)
            cur[0] = 0
            cur[1:] = np.maximum(T[:-1] + e, T[1:])
            T = np.maximum.accumulate(cur)          # the horizontal move is free in T
    return T


def chunk_columns(c, lane, n):
    """Columns (1-based, piece coordinates) of chunk c in `lane`, clipped to the piece; empty when hi < lo."""
    return max(128 * c - 2 * lane + 1, 1), min(128 * c - 2 * lane + 128, n)


def is_full(c, n):
    """Chunks that run the kernel's unpredicated path: every lane's columns of steps 64 c + 1 .. 64 c + 64 exist."""
    return c >= 1 and 128 * (c + 1) <= n


def chunk_values(T, hh, lane, n_chunks, cmg=1):
    """Chunk values of `lane` (as the dump holds them: no bias).  cmg > 1: grouped samples on the full chunks."""
    n = len(T) - 1
    dec = T - np.arange(n + 1, dtype=np.int64) * hh
    out = np.zeros(n_chunks, np.int64)
    for c in range(n_chunks):
        if cmg > 1 and is_full(c, n):
            first = 64 * c + 1 + cmg * np.arange(64 // cmg)            # first step of every group
            j_first = 2 * (first - lane) - 1
            j_last = 2 * (first + cmg - 1 - lane)
            out[c] = max(0, int((T[j_last] - j_first * hh).max()))
        else:
            lo, hi = chunk_columns(c, lane, n)
            if hi >= lo:
                out[c] = max(0, int(dec[lo:hi + 1].max()))
    return out
