"""The stretches of the flank methylation calls from the detect pipeline (strq_batch_fetch_flank_ranges): where the alignments of the
whole configured flanks begin and end, before the trim that moves the row's prefix_begin / suffix_end to the inner 50 nt.  Against
tests/flank_mod_ref.flank_ranges (the oracle's __detect_range__ without a trim) on the reads of tests/test_gpu_flank_mod_models.py,
exactly; the rows themselves are what they were."""
import numpy as np
import pytest

import flank_mod_ref as fr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("names,as_int16", [(("c9orf72", "htt"), True), (("c9orf72",), False)])
def test_ranges_equal_the_reference(gpu_counter, tables, cfg, targets, orc, names, as_int16):
    cases, opm, _ = fr.cases(tables, cfg, targets, names, as_int16)
    params = orc.align_params(cfg["align"])
    items = [(c["target"], c["sig"], c["strand"]) for c in cases]
    rows = gpu_counter.detect_batch(items)
    got = gpu_counter.ctx.batch_fetch_flank_ranges()
    res = gpu_counter.ctx.batch_fetch()
    assert got.shape == (len(cases), 4) and got.dtype == np.int64
    for c, row, g, r in zip(cases, rows, got, res):
        what = (c["target"], c["strand"], c["table"])
        (_, _, pb, pe, _), (_, _, sb, se, _) = c["flanks"]
        assert tuple(int(v) for v in g) == (pb, pe, sb, se), (what, g, c["flanks"][0][2:4], c["flanks"][1][2:4])
        # the row keeps the trimmed positions: the inner 50 nt of a 150-nt flank
        assert (int(r["prefix_end"]), int(r["suffix_begin"])) == (pe, sb) and pb < int(r["prefix_begin"]) < pe and sb < int(r["suffix_end"]) < se, (what, r)
        tc = orc.classifier(*targets[c["target"]], c["strand"], opm, None, cfg["HMM"])
        want, info = orc.detect(c["sig"], tc, opm, params)
        assert tuple(row[:6]) == tuple(want[:6]) and (int(r["prefix_begin"]), int(r["suffix_end"])) == (info["prefix_begin"], info["suffix_end"]), what
    from strique_amd import ffi
    with pytest.raises(ffi.StriqueHipError) as e:
        gpu_counter.ctx._check(gpu_counter.ctx._lib.strq_batch_fetch_flank_ranges(gpu_counter.ctx._h, None, __import__("ctypes").c_int64(3)))
    assert e.value.code == ffi.STRQ_ERR_ARG
