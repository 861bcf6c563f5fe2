"""Repeat-unit positions (strq_set_units / strq_batch_fetch_units, `count --units`, `plot --units`): the host side, no GPU."""
import ctypes
import io
import os
import re
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np

from conftest import ROOT

UNIT_ENTRIES = ("strq_set_units", "strq_batch_fetch_units", "strq_last_units")


def test_unit_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    declared = set(re.findall(r"\b(strq_[a-z_0-9]+)\s*\(", header))
    assert set(UNIT_ENTRIES) <= declared
    assert "int strq_batch_fetch_units(strq_ctx* ctx, int64_t* pool, int64_t pool_cap, int64_t* off, int32_t* decoded);" in header
    from strique_amd import ffi
    lib = ffi.load_library()
    for name in UNIT_ENTRIES:
        getattr(lib, name)
    assert lib.strq_abi_version() == 13          # the entries are additive


def test_argument_errors_without_a_context():
    from strique_amd import ffi
    lib = ffi.load_library()
    lib.strq_set_units.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.strq_batch_fetch_units.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.strq_last_units.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.strq_set_units(None, 1) == ffi.STRQ_ERR_ARG
    off = np.zeros(2, np.int64)
    assert lib.strq_batch_fetch_units(None, None, 0, off.ctypes.data, None) == ffi.STRQ_ERR_ARG
    assert lib.strq_last_units(None, None) == ffi.STRQ_ERR_ARG


def test_units_rows_are_formatted_and_parsed():
    from strique_amd import cli
    rows = [cli.format_units("r1", "c9orf72", "+", 7, np.array([105, 160, 221], np.int64)),
            cli.format_units("r2", "fmr1", "-", 0, None),                 # not decoded
            cli.format_units("r3", "fmr1", "-", 4, [])]                   # decoded, no unit on the path
    assert rows[0] == "r1\tc9orf72\t+\t7\t3\t105,160,221"
    assert rows[1] == "r2\tfmr1\t-\t0\t0\t-" and rows[2] == "r3\tfmr1\t-\t4\t0\t-"
    buf = io.StringIO()
    cli.write_rows(buf, list(enumerate(rows)), header=cli.UNITS_HEADER)
    text = buf.getvalue()
    assert text.splitlines()[0] == "ID\ttarget\tstrand\tcount\tn_units\tunits"
    assert cli.parse_units(io.StringIO(text)) == [("r1", "c9orf72", "+", 7, [105, 160, 221]), ("r2", "fmr1", "-", 0, []), ("r3", "fmr1", "-", 4, [])]


UNITS_WORKER = r'''
import io, json, os, sys
import numpy as np
sys.path.insert(0, %r)
from strique_amd import cli, dist as sdist
rank, world, local = sdist.init_process_group(backend="gloo")
cfg = json.load(open(os.path.join(%r, "tests", "golden", "config.json")))
loci = {}
for name, (chrom, b, e, *_r) in cfg["repeat"].items():
    loci.setdefault(chrom, []).append((name, b, e))
lines = ["@HD\tVN:1.0"]
for i in range(29):
    chrom, pos = ("chr9", 27570000) if i %% 3 else ("chrX", 146990000)
    lines.append("\t".join(["read%%d" %% i, "16" if i %% 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))

class FakeCounter(object):                               # stands in for the GPU engine: rows and positions depend on the inputs only
    def detect_batch(self, items, units=False):
        out = []
        for t, raw, s in items:
            row = (len(raw) %% 97, 1.5, 2.5, -3.0 * len(t), int(raw[0]), 7, "01"[len(raw) %% 2] * (len(raw) %% 5))
            pos = None if len(raw) %% 5 == 0 else np.arange(len(raw) %% 7, dtype=np.int64) * 13 + int(raw[0])
            out.append((row, pos) if units else row)
        return out

def get_raw(qname):
    i = int(qname[4:])
    return np.arange(100 + i, 300 + 2 * i)

log = cli.Log("error")
stats = {}
mine = cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, rank, world, stats=stats, units=True)
got = cli.gather_rows(mine, stats["items"], sdist, units=True)       # still one gather: records + one blob per row
merged, merged_units = got.rows, got.units
import torch.distributed as dist
if rank == 0:
    buf = io.StringIO(); cli.write_rows(buf, merged)
    ubuf = io.StringIO(); cli.write_rows(ubuf, merged_units, header=cli.UNITS_HEADER)
    one = io.StringIO(); uone = io.StringIO(); st1 = {}
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, one, stats=st1, units=True, units_out=uone)
    plain = io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, plain)
    assert buf.getvalue() == one.getvalue() == plain.getvalue()
    assert ubuf.getvalue() == uone.getvalue(), (ubuf.getvalue(), uone.getvalue())
    assert len(uone.getvalue().splitlines()) == len(one.getvalue().splitlines()) == 30
    assert [r[1] for r in st1["unit_rows"]] == uone.getvalue().splitlines()[1:]
    print("UNITS_GATHER_OK")
else:
    assert merged is None and merged_units is None
dist.barrier(); dist.destroy_process_group()
''' % (ROOT, ROOT)


def test_two_rank_gather_carries_the_unit_positions(tmp_path):
    """`count --units` under torchrun: the positions ride in the byte pool of the one gather (next to the modification string),
    and rank 0's rows and unit rows equal the single-process ones (which the flag leaves byte-identical)."""
    script = tmp_path / "units_worker.py"
    script.write_text(UNITS_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "UNITS_GATHER_OK" in outs[0]


def test_plot_marks_the_unit_positions(tmp_path):
    import h5write
    from matplotlib.figure import Figure
    from strique_amd import cli, plotting
    rng = np.random.default_rng(5)
    rid = "bbbbbbbb-0001-4000-8000-000000000000"
    sig = rng.integers(200, 900, 6000).astype(np.int16)
    tree = {"attrs": {"file_version": "2.0"}, "groups": {"read_" + rid: {"groups": {
        "Raw": {"attrs": {"read_id": rid, "duration": len(sig), "read_number": 1, "start_time": 1, "median_before": 200.0},
                "datasets": {"Signal": (sig, {})}},
        "channel_id": {"attrs": {"channel_number": "1", "digitisation": 8192.0, "offset": 10.0, "range": 1400.5, "sampling_rate": 4000.0}}}}}}
    src = tmp_path / "src"; src.mkdir()
    (src / "batch.fast5").write_bytes(h5write.write_tree(tree))
    buf = io.StringIO()
    with redirect_stdout(buf):
        cli.main(["index", str(src)])
    (src / "reads.fofn").write_text(buf.getvalue())
    counts = tmp_path / "counts.tsv"
    counts.write_text("\t".join(cli.HEADER) + "\n" + "\t".join([rid, "c9orf72", "+", "5", "6.5", "6.1", "-1234.5", "1000", "2500", "-"]) + "\n")
    units = [1010, 1500, 2000, 2600, 3450]
    ufile = tmp_path / "units.tsv"
    ufile.write_text("\t".join(cli.UNITS_HEADER) + "\n" + cli.format_units(rid, "c9orf72", "+", 5, units) + "\n")
    plain = cli.plot([str(src / "reads.fofn"), "--counts", str(counts), "--output", str(tmp_path / "p0"), "--width", "6", "--height", "4"])
    marked = cli.plot([str(src / "reads.fofn"), "--counts", str(counts), "--output", str(tmp_path / "p1"), "--width", "6", "--height", "4",
                       "--units", str(ufile)])
    assert len(plain) == len(marked) == 1 and os.path.getsize(marked[0]) > 2000
    assert open(plain[0], "rb").read() != open(marked[0], "rb").read()
    row = next(iter(plotting.parse_counts(open(counts))))
    axes = plotting.draw(Figure(figsize=(6, 4)), sig, row, zoom=500, units=units)
    assert list(axes["overview"].strique_units) == units
    lo, hi = plotting.Windows(len(sig), row.offset, row.ticks, 0.1, 500).left
    assert list(axes["left"].strique_units) == [u for u in units if lo <= u < hi]
    assert not hasattr(plotting.draw(Figure(figsize=(6, 4)), sig, row, zoom=500)["overview"], "strique_units")
