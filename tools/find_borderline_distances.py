#!/usr/bin/env python
"""Search for the float32 distances whose score-table entry is "borderline" (csrc/lut_kernels.hip: cell_score_dev).

The table kernel evaluates pow((double)d, 1.2) on the device and casts it to float.  Two pow implementations that differ by a few
ulp(double) give the same float unless the double lies next to a float rounding boundary, i.e. unless the 29 bits the cast drops
are close to 0x10000000.  The kernel hands every entry within 64 of it to the host (STRQ_HARD_ULPS); this script lists the
distances within WINDOW = 32, half of that, so that a device pow a few ulp away from the host's still flags them.

All positive float32 below LIMIT = 10.08 are scanned (10.08 ** 1.2 > 16: beyond it every score clips to dist_min under
the parameter sets the tests use).  numpy's pow only pre-selects (window PRE); the C library's pow, through ctypes, decides.

    python tools/find_borderline_distances.py [--jobs N]

prints one `0x........,  # value  low-bits offset` line per distance -- the literal list BORDERLINE_BITS of tests/table_cases.py --
and the counts by range.  tests/test_table_cases_host.py re-verifies every committed constant with the C pow.
"""
import argparse
import ctypes
import ctypes.util
import sys

import numpy as np

WINDOW = 32
PRE = 48                      # pre-selection window of the numpy pass (numpy's pow is within a few ulp of libm's)
LIMIT = np.float32(10.08)
CHUNK = 1 << 22

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]


def low_offset(d):
    """Distance of the 29 bits a float cast drops from the rounding midpoint, for the C library's pow(d, 1.2)."""
    y = _libm.pow(float(np.float32(d)), 1.2)
    bits = int(np.array([y], np.float64).view(np.uint64)[0])
    return (bits & 0x1FFFFFFF) - 0x10000000


def scan(span):
    b0, b1 = span
    found = []
    for s in range(b0, b1, CHUNK):
        bits = np.arange(s, min(s + CHUNK, b1), dtype=np.uint32)
        y = np.power(bits.view(np.float32).astype(np.float64), 1.2)
        low = (y.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64) - 0x10000000
        for b in bits[np.abs(low) <= PRE]:
            off = low_offset(np.array([b], np.uint32).view(np.float32)[0])
            if abs(off) <= WINDOW:
                found.append((int(b), off))
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    end = int(np.array([LIMIT], np.float32).view(np.uint32)[0])
    step = (end + 8 * a.jobs - 1) // (8 * a.jobs)
    spans = [(max(1, s), min(s + step, end)) for s in range(0, end, step)]
    if a.jobs > 1:
        import multiprocessing
        with multiprocessing.Pool(a.jobs) as pool:
            parts = pool.map(scan, spans)
    else:
        parts = [scan(s) for s in spans]
    found = sorted(x for p in parts for x in p)
    for b, off in found:
        print("    0x%08x,  # %-16r %+d" % (b, float(np.array([b], np.uint32).view(np.float32)[0]), off))
    vals = np.array([b for b, _ in found], np.uint32).view(np.float32)
    sys.stderr.write("%d distances below %r within +-%d; %d in [0.5, 8); %d below 2**-20\n"
                     % (len(found), float(LIMIT), WINDOW, int(((vals >= 0.5) & (vals < 8)).sum()), int((vals < 2.0 ** -20).sum())))


if __name__ == "__main__":
    main()
