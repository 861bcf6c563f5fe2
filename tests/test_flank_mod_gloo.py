"""`count --flank-mod` over two gloo ranks on the CPU: the flank rows travel in the one gather of the run and equal the single-process
output, as the count rows do (tests/test_dist_gloo.py); the counter is a stand-in whose records depend on the inputs only."""
import os
import subprocess
import sys

from conftest import ROOT

WORKER = r'''
import io, json, os, sys
import numpy as np
sys.path.insert(0, %r)
from strique_amd import cli, dist as sdist, flank_mod
from strique_amd.counter import Detected
rank, world, local = sdist.init_process_group(backend="gloo")
cfg = json.load(open(os.path.join(%r, "tests", "golden", "config.json")))
loci = {}
for name, (chrom, b, e, *_r) in cfg["repeat"].items():
    loci.setdefault(chrom, []).append((name, b, e))
lines = ["@HD\tVN:1.0"]
for i in range(29):
    chrom, pos = ("chr9", 27570000) if i %% 3 else ("chrX", 146990000)
    lines.append("\t".join(["read%%d" %% i, "16" if i %% 2 else "0", chrom, str(pos), "60", "5S8000M3S", "*", "0", "0", "ACGT", "*"]))

class FakeCounter(object):                               # stands in for the GPU engine: records depend on the inputs only
    on = False
    def set_flank_mod(self, on):
        self.on = bool(on)
    def detect_batch(self, items, records=False):
        assert records and self.on
        out = []
        for t, raw, s in items:
            n = len(raw)
            row = (n %% 97, 1.5, 2.5, -3.0 * len(t), int(raw[0]), 7, "-")
            calls = None if n %% 5 == 0 else [(k %% 2, 3 * k + n %% 7, 1 + k %% 3, 5, 0 if (k + n) %% 4 else 2, 10, 20, (n * 0.37 - k) / 3.0) for k in range(n %% 4)]
            out.append(Detected(row, None, None, None, flank_mod=calls))
        return out

def get_raw(qname):
    i = int(qname[4:])
    return np.arange(100 + i, 300 + 2 * i)

log = cli.Log("error")
stats = {}
c = FakeCounter()
mine = cli.run_count(iter(lines), loci, get_raw, c, log, 5, rank, world, stats=stats, flank_mod=True)
assert not c.on                                          # the switch belongs to the run
import torch.distributed as dist
merged = cli.gather_rows(mine, stats["items"], sdist, flank_mod=True)
if rank == 0:
    buf, fbuf = io.StringIO(), io.StringIO()
    cli.write_rows(buf, merged.rows); cli.write_rows(fbuf, merged.flank_mod, header=flank_mod.HEADER)
    one, fone = io.StringIO(), io.StringIO()
    cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 5, 0, 1, one, flank_mod=True, flank_mod_out=fone)
    assert buf.getvalue() == one.getvalue()
    assert fbuf.getvalue() == fone.getvalue(), (fbuf.getvalue(), fone.getvalue())
    rows = flank_mod.parse(io.StringIO(fbuf.getvalue()))
    assert len(rows) == 29 and any(r[4] for r in rows) and any(not r[4] for r in rows) and any(x[3] is None for r in rows for x in r[4])
    print("FLANK_GATHER_OK")
else:
    assert merged.rows is None and merged.flank_mod is None
dist.barrier(); dist.destroy_process_group()
''' % (ROOT, ROOT)


def test_two_ranks_gather_the_flank_rows(tmp_path):
    script = tmp_path / "flank_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29523", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "FLANK_GATHER_OK" in outs[0]
