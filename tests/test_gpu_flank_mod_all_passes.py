"""The flank methylation calls beside every other optional pass, in the manner of tests/test_gpu_all_passes.py and on its reads and
counter (units, confidence, mod-llr, variants, anchored, anchored-mod, tracts; three sub-batches of at most two reads): with all of
them on, the rows and every other pass's fetch and counters are byte-equal with the flank switch on and off, and the flank records
are equal with the other switches on and off.  Renorm is left off: it changes the rows."""
import pytest

from test_gpu_all_passes import SWITCHES, _run, counter, items  # noqa: F401  (counter, items: its fixtures)

pytestmark = pytest.mark.gpu


def _with_flank(counter, items, on, flank):
    counter.set_flank_mod(flank)
    try:
        out, last = _run(counter, items, on)
    finally:
        counter.set_flank_mod(False)
    recs = [None if r is None else r.tobytes() for r in counter.ctx.batch_fetch_flank_mod()] if flank else None
    fl = counter.ctx.last_flank_mod()
    return out, last, recs, {k: v for k, v in fl.items() if k != "ms"}


def test_every_other_pass_is_untouched_and_so_are_the_flank_records(counter, items):
    on_all = _with_flank(counter, items, SWITCHES, True)
    off_all = _with_flank(counter, items, SWITCHES, False)
    alone = _with_flank(counter, items, (), True)
    assert set(on_all[0]) == {"rows", "mod"} | set(SWITCHES)
    for name in on_all[0]:
        assert on_all[0][name] == off_all[0][name], name
    assert on_all[1] == off_all[1]          # the counters of every other pass
    assert off_all[3] == {"flanks": 0, "groups": 0, "launches": 0}
    assert on_all[2] == alone[2] and on_all[3] == alone[3]
    recs = on_all[2]
    # the two spanning reads are called; the read whose flanks stand in the wrong order fails the gate
    assert recs[0] is not None and recs[2] is not None and recs[4] is None and on_all[3]["flanks"] >= 4 and on_all[3]["groups"] > 20
    assert alone[0]["rows"] == on_all[0]["rows"] and alone[0]["mod"] == on_all[0]["mod"]
