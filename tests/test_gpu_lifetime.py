"""Who owns the memory: everything a context allocates on the device and in pinned host memory -- its workspace, the images of its
models (lane layout, register-resident, forward, per-unit scores), the buffers of the optional passes, of a scan and of the upload's
staging ring -- is given back by strq_ctx_destroy.  strq_debug_live_allocations counts the blocks the library holds in the process."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 5.0          # anchored score threshold: between the present flank of the cut read (6.7) and its absent one (3.1)
MIN_SCORE = 5.0  # scan: the smallest flank score a candidate needs


def _read(rng, table, target, n_repeat, strand, keep=1.0):
    """A read of a few thousand samples: 200 nt of background on either side of prefix + repeats + suffix; keep < 1 cuts it there."""
    from strique_amd import synth
    from strique_amd.counter import reverse_complement
    repeat, prefix, suffix = target
    back = lambda: "".join(rng.choice(list("ACGT"), 200))
    seq = back() + (prefix + repeat * n_repeat + suffix).upper() + back()
    sig = synth.make_signal(rng, table, (seq if strand == "+" else reverse_complement(seq)).encode())
    return np.ascontiguousarray(sig[:int(len(sig) * keep)])


@pytest.fixture(scope="module")
def reads(pm, pm_mod, targets):
    """Four reads on C9orf72: two from the base table, one from the mCpG one, and one cut inside its repeat."""
    from strique_amd import synth
    target = targets["c9orf72"]
    base, mod = synth.KmerTable(pm), synth.KmerTable(pm_mod)
    rng = np.random.default_rng(53)
    sig = [_read(rng, base, target, 12, "+"), _read(rng, base, target, 21, "-"), _read(rng, mod, target, 17, "+"), _read(rng, base, target, 40, "+", keep=0.5)]
    assert all(s.dtype == np.int16 and 2000 < len(s) < 8000 for s in sig)
    return [("c9orf72", s, st) for s, st in zip(sig, "+-++")]


def _one_context(pm, pm_mod, cfg, targets, reads, baseline):
    """A context of its own: models, every optional pass, one detect batch, one scan over two candidates, close.  Returns what the
    calls returned and the counters before the close; asserts that the close brings them back to `baseline`."""
    from strique_amd import ffi
    from strique_amd.counter import repeatCounter
    rc = repeatCounter(pm, mod_model_file=pm_mod, align_config=cfg["align"], HMM_config=cfg["HMM"], device=0)
    try:
        rc.add_target("c9orf72", *targets["c9orf72"])          # flanked models with positions, modification models
        got = rc.detect_batch(reads, units=True, confidence=True, mod_llr=True, anchored=M, records=True)      # registers the anchored models
        assert set(rc.anchored_models) == {rc._classifier_for("c9orf72", st).target_id for st in "+-"}
        assert rc.ctx.last_viterbi_launches()["register_resident"] >= 1          # the flanked models run on their register-resident image
        ran = (rc.ctx.last_units(), rc.ctx.last_confidence(), rc.ctx.last_mod_llr(), rc.ctx.last_anchored())
        assert len(rc.candidates()) == 2
        scan = rc.scan_batch([s for _, s, _ in reads], min_score=MIN_SCORE, scores=True)
        live = ffi.live_allocations()
    finally:
        rc.ctx.close()
    assert ffi.live_allocations() == baseline
    return got, ran, scan, live


def test_close_gives_back_every_block(pm, pm_mod, cfg, targets, reads):
    from strique_amd import ffi
    baseline = ffi.live_allocations()          # other contexts of the process stay open
    got, ran, scan, live = _one_context(pm, pm_mod, cfg, targets, reads, baseline)
    print("live allocations (device, pinned): before", baseline, "with the context", live, "passes:", ran)
    assert live[0] > baseline[0] and live[1] > baseline[1]
    # the inputs reached what they were chosen for: decoded reads, a pattern with units, a read of kind 2 or 3, a scan with a winner
    assert sum(d.units is not None for d in got) >= 3 and sum(d.conf is not None for d in got) >= 3
    assert any(d.llr is not None for d in got) and any(d.anchored[0] in (2, 3) for d in got)
    assert any(w is not None for w in scan[0])


def test_two_contexts_in_a_row_same_rows_same_counters(pm, pm_mod, cfg, targets, reads):
    from strique_amd import ffi
    baseline = ffi.live_allocations()
    first = _one_context(pm, pm_mod, cfg, targets, reads, baseline)
    second = _one_context(pm, pm_mod, cfg, targets, reads, baseline)
    for a, b in zip(first[0], second[0]):
        assert a.row == b.row and a.anchored == b.anchored
        assert (a.units is None) == (b.units is None) and (a.units is None or np.array_equal(a.units, b.units))
        assert (a.conf is None) == (b.conf is None) and (a.conf is None or np.array(a.conf).tobytes() == np.array(b.conf).tobytes())
        assert (a.llr is None) == (b.llr is None) and (a.llr is None or np.array(a.llr).tobytes() == np.array(b.llr).tobytes())
    assert first[2][0] == second[2][0] and first[2][1].tobytes() == second[2][1].tobytes()
    assert first[3] == second[3]          # the same blocks held at the same point
