"""Count confidence (strq_forward_batch, strq_set_confidence, `count --confidence`): the host side, no GPU."""
import ctypes
import io
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT
from forward_ref import forward_ref

CONF_ENTRIES = ("strq_forward_batch", "strq_set_confidence", "strq_batch_fetch_confidence", "strq_last_confidence")


def test_confidence_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "strique_hip.h")).read()
    declared = set(re.findall(r"\b(strq_[a-z_0-9]+)\s*\(", header))
    assert set(CONF_ENTRIES) <= declared
    from strique_amd import ffi
    lib = ffi.load_library()
    for name in CONF_ENTRIES:
        getattr(lib, name)
    assert lib.strq_abi_version() == 13          # the entries are additive
    lib.strq_forward_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 7
    lib.strq_set_confidence.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.strq_batch_fetch_confidence.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.strq_last_confidence.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.strq_model_set_forward_logp.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    buf = np.zeros(8)
    assert lib.strq_forward_batch(None, 0, 0, None, None, None, None, None, None, None) == ffi.STRQ_ERR_ARG
    assert lib.strq_set_confidence(None, 1) == ffi.STRQ_ERR_ARG
    assert lib.strq_batch_fetch_confidence(None, buf.ctypes.data, None) == ffi.STRQ_ERR_ARG
    assert lib.strq_last_confidence(None, buf.ctypes.data) == ffi.STRQ_ERR_ARG
    assert lib.strq_model_set_forward_logp(None, 0, buf.ctypes.data) == ffi.STRQ_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# forward_ref against every path of a toy HMM
#   emitting: 0 = M0 Normal, 1 = C Uniform (counted, loops on itself and through the silent chain), 2 = M1 Normal
#   silent  : 3 = start, 4..6 = the chain S1 -> S2 -> S3, 7 = end
TOY_EDGES = [(3, 0, 1.0),
             (0, 0, .3), (0, 1, .4), (0, 4, .3),
             (4, 5, .5), (4, 1, .5),
             (5, 6, .4), (5, 2, .6),
             (6, 2, .7), (6, 1, .3),
             (1, 1, .5), (1, 2, .3), (1, 4, .2),
             (2, 2, .4), (2, 7, .6)]
TOY_NORMAL = {0: (80.0, 3.0), 2: (95.0, 2.0)}
TOY_UNIFORM = {1: (70.0, 110.0)}


def _toy():
    n, ne = 8, 3
    ins = [[] for _ in range(n)]
    for a, b, p in TOY_EDGES:
        ins[b].append((a, math.log(p)))
    t = SimpleNamespace(n_states=n, silent_start=ne, start=3, end=7)
    t.in_ptr = np.zeros(n + 1, np.int32)
    src, lp = [], []
    for l in range(n):
        t.in_ptr[l + 1] = t.in_ptr[l] + len(ins[l])
        src += [a for a, _ in ins[l]]; lp += [q for _, q in ins[l]]
    t.in_src = np.array(src, np.int32); t.in_logp = np.array(lp)
    t.emis_kind = np.array([1, 2, 1], np.int32)
    t.emis_a = np.array([80.0, 70.0, 95.0]); t.emis_b = np.array([1 / (2 * 3.0 ** 2), 110.0, 1 / (2 * 2.0 ** 2)])
    t.emis_c = np.array([-math.log(3.0 * 2.50662827463), -math.log(40.0), -math.log(2.0 * 2.50662827463)])
    t.count_inc = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32)
    return t


def _emission(state, x):
    if x != x:
        return 1.0
    if state in TOY_NORMAL:
        mu, sigma = TOY_NORMAL[state]
        return math.exp(-math.log(sigma * 2.50662827463) - (x - mu) ** 2 / (2 * sigma ** 2))
    lo, hi = TOY_UNIFORM[state]
    return 1.0 / (hi - lo) if lo <= x <= hi else 0.0


def _enumerate(x):
    """{visits of the counted state: summed probability} over every path start -> end that emits x."""
    out_edges = {}
    for a, b, p in TOY_EDGES:
        out_edges.setdefault(a, []).append((b, p))
    dist = {}

    def walk(state, t, prob, v):
        if state == 7:
            if t == len(x):
                dist[v] = dist.get(v, 0.0) + prob
            return
        for b, p in out_edges.get(state, []):
            if b < 3:
                if t < len(x):
                    e = _emission(b, x[t])
                    if e > 0:
                        walk(b, t + 1, prob * p * e, v + (1 if b == 1 else 0))
            else:
                walk(b, t, prob * p, v)
    walk(3, 0, 1.0, 0)
    return dist


@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_forward_ref_equals_the_sum_over_every_path_of_a_toy_model(dtype):
    """1e-12: a few hundred float64 operations on O(1) values (the enumeration itself is float64)."""
    toy = _toy()
    xs = {1: [82.0], 2: [79.0, 96.0], 3: [81.5, 90.0, 94.0], 4: [80.0, 75.0, 104.0, 95.5], 5: [78.0, 88.0, np.nan, 101.0, 93.0],
          6: [83.0, 72.0, 108.5, 91.0, 97.0, 94.5]}
    xs["outside"] = [80.0, 115.0, 96.0, 94.0]          # 115 is outside the Uniform's support: C cannot emit it
    seen_none = False
    for key, x in xs.items():
        dist = _enumerate(x)
        ll, mean, sd, status = forward_ref(toy, np.array(x), dtype)
        total = sum(dist.values())
        if total == 0.0:
            assert status == 1 and ll == -np.inf and np.isnan(mean) and np.isnan(sd)
            seen_none = True
            continue
        m1 = sum(v * p for v, p in dist.items()) / total
        var = sum((v - m1) ** 2 * p for v, p in dist.items()) / total
        assert status == 0
        assert abs(float(ll) - math.log(total)) <= 1e-12 * abs(math.log(total)), key
        assert abs(float(mean) - m1) <= 1e-12 and abs(float(sd) - math.sqrt(var)) <= 1e-12, key
        if key == 6:
            assert len(dist) >= 4 and var > 0.1          # a real spread of counts, not a point mass
    assert seen_none                                      # T = 1: M0 cannot reach M1 without a second emission


def test_confidence_rows_are_formatted_and_parsed():
    from strique_amd import cli
    conf = (-1016.8643276707, 6.99563963, 0.0659207)
    rows = [cli.format_confidence("r1", "c9orf72", "+", 7, -1020.25, conf),
            cli.format_confidence("r2", "fmr1", "-", 0, 0, None)]                 # not decoded: the integer 0 of the count row, three dashes
    assert rows[0] == "r1\tc9orf72\t+\t7\t-1020.25\t-1016.8643276707\t6.99563963\t0.0659207"
    assert rows[1] == "r2\tfmr1\t-\t0\t0\t-\t-\t-"
    buf = io.StringIO()
    cli.write_rows(buf, list(enumerate(rows)), header=cli.CONF_HEADER)
    text = buf.getvalue()
    assert text.splitlines()[0] == "ID\ttarget\tstrand\tcount\tlog_p\tlog_lik\tcount_mean\tcount_sd"
    assert cli.parse_confidence(io.StringIO(text)) == [("r1", "c9orf72", "+", 7, -1020.25, conf), ("r2", "fmr1", "-", 0, 0.0, None)]
    # str() of a float64 round-trips: the file holds the bits
    odd = (-12345.678901234567, 733.0000000000001, 1e-9)
    assert cli.parse_confidence(io.StringIO(cli.format_confidence("r", "t", "+", 733, -12350.5, odd)))[0][5] == odd


CONF_WORKER = r'''
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

class FakeCounter(object):                               # stands in for the GPU engine: everything depends on the inputs only
    def detect_batch(self, items, units=False, confidence=False):
        out = []
        for t, raw, s in items:
            row = (len(raw) %% 97, 1.5, 2.5, -3.0 * len(t), int(raw[0]), 7, "01"[len(raw) %% 2] * (len(raw) %% 5))
            pos = None if len(raw) %% 5 == 0 else np.arange(len(raw) %% 7, dtype=np.int64) * 13 + int(raw[0])
            conf = None if len(raw) %% 5 == 0 else (-3.0 * len(t) + 1.0 / len(raw), len(raw) %% 97 + 0.1 / 3, 1.0 / (1 + int(raw[0])))
            out.append(((row, pos) if units else (row,)) + (conf,) if confidence else ((row, pos) if units else row))
        return out
    def detect(self, t, raw, s, **kw):
        return self.detect_batch([(t, raw, s)], **kw)[0]

def get_raw(qname):
    i = int(qname[4:])
    return np.arange(100 + i, 300 + 2 * i)

log = cli.Log("error")
import torch.distributed as dist
for units in (False, True):
    stats = {}
    mine = cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, rank, world, stats=stats, units=units, confidence=True)
    got = cli.gather_rows(mine, stats["items"], sdist, units=units, confidence=True)      # still one gather
    merged, merged_units, merged_conf = got.rows, got.units, got.confidence
    if rank == 0:
        buf = io.StringIO(); cli.write_rows(buf, merged)
        cbuf = io.StringIO(); cli.write_rows(cbuf, merged_conf, header=cli.CONF_HEADER)
        one = io.StringIO(); cone = io.StringIO(); uone = io.StringIO(); st1 = {}
        cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, one, stats=st1, units=units, units_out=uone if units else None,
                      confidence=True, conf_out=cone)
        plain = io.StringIO()
        cli.run_count(iter(lines), loci, get_raw, FakeCounter(), log, 4, 0, 1, plain)
        assert buf.getvalue() == one.getvalue() == plain.getvalue()
        assert cbuf.getvalue() == cone.getvalue(), (cbuf.getvalue(), cone.getvalue())
        assert len(cone.getvalue().splitlines()) == len(one.getvalue().splitlines()) == 30
        assert [r[1] for r in st1["conf_rows"]] == cone.getvalue().splitlines()[1:]
        parsed = cli.parse_confidence(io.StringIO(cbuf.getvalue()))
        assert sum(r[5] is None for r in parsed) >= 3 and sum(r[5] is not None for r in parsed) >= 20
        if units:
            ubuf = io.StringIO(); cli.write_rows(ubuf, merged_units, header=cli.UNITS_HEADER)
            assert ubuf.getvalue() == uone.getvalue()
        else:
            assert merged_units is None
    else:
        assert merged is None and merged_units is None and merged_conf is None
if rank == 0:
    print("CONF_GATHER_OK")
dist.barrier(); dist.destroy_process_group()
''' % (ROOT, ROOT)


def test_two_rank_gather_carries_the_confidence(tmp_path):
    """`count --confidence` under torchrun: the three values ride in the byte pool of the one gather (behind the modification string
    and the unit positions), bit for bit, and rank 0's rows equal the single-process ones (which the flag leaves byte-identical)."""
    script = tmp_path / "conf_worker.py"
    script.write_text(CONF_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "CONF_GATHER_OK" in outs[0]


def test_confidence_with_scan_is_rejected_by_the_parser(capsys):
    from strique_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["count", "reads.fofn", "model", "repeats.tsv", "--scan", "--scan-min-score", "5", "--confidence", "conf.tsv"])
    assert ei.value.code == 2
    assert "--confidence cannot be combined with --scan" in capsys.readouterr().err


def test_bake_keeps_the_summed_mass_of_parallel_edges(pm, cfg):
    """Two spliced paths between one pair of states (profile -> e1 / e2 -> end) become one baked edge: in_logp holds the larger
    probability, as the decode needs it, in_logp_sum their sum, as the forward pass needs it; every other edge has both equal."""
    from strique_amd import hmm
    chrom, b, e, repeat, prefix, suffix = cfg["repeat"]["c9orf72"]
    bk = hmm.FlankedRepeatModel(repeat, prefix[-20:], suffix[:20], pm, cfg["HMM"]).baked
    differ = np.nonzero(bk.in_logp_sum != bk.in_logp)[0]
    ends = set(range(int(bk.in_ptr[bk.end]), int(bk.in_ptr[bk.end + 1])))
    assert len(differ) == 3 and set(differ) <= ends
    assert np.all(bk.in_logp_sum >= bk.in_logp)
    got = sorted(np.exp(bk.in_logp_sum[differ]) - np.exp(bk.in_logp[differ]))
    assert np.allclose(got, [0.005, 0.01, 0.05], rtol=1e-9)          # delete_delete, match_delete, insert_delete behind the last column
