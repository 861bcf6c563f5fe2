"""The cases of tests/vit_mode_cases.py, checked without a GPU: which kernel shape every model lands on (strq_debug_viterbi_plan), that
the case list covers the table of (shape, mode) pairs in strique_amd/csrc/vit_model.h, that the two references agree, and that the
cases exercise what they are there for.  tests/test_gpu_viterbi_modes.py then holds the kernels against the same references.
The same for the sourced windows (samples and a per-window map, as the detect pipeline gives them), which
tests/test_gpu_viterbi_sources.py launches."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import vit_mode_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def all_cases(pm, pm_mod, cfg):
    from strique_amd import build
    build.build_lib()
    return vc.cases(pm, pm_mod, cfg)


@pytest.fixture(scope="module")
def plans(all_cases):
    from strique_amd import ffi
    return {name: ffi.debug_viterbi_plan(c.baked) for name, c in all_cases.items()}


def test_abi_is_additive():
    import ctypes
    from strique_amd import build
    lib = ctypes.CDLL(build.build_lib())
    assert lib.strq_abi_version() == 13
    assert lib.strq_debug_viterbi_plan and lib.strq_debug_viterbi_mode and lib.strq_debug_viterbi_sourced


def test_every_model_lands_on_its_row(all_cases, plans):
    assert list(all_cases) == list(vc.CASE_NAMES)
    for name, c in all_cases.items():
        p = plans[name]
        if c.row is not None:
            assert p["row"] == c.row, (name, p)
        if c.ss is not None:
            assert p["ss"] == c.ss and p["single_stage"] == int(c.ss), (name, p)
        if c.g2:          # STRique's flanked models: the lane row they run on with STRQ_VIT_NO_G2
            assert p["row"] in (0, 5, 7), (name, p)
        assert p["csr"] == int(p["row"] == vc.SHAPE_CSR)
        assert set(c.modes) <= set(p["modes"]), (name, c.modes, p["modes"])
        assert p["shapes"] == [p["shape"]] * 5
        if vc.VIT_HUB in c.modes:
            assert p["rec_state"] == vc.rec_state(c.baked) >= 0
        if vc.VIT_UNIT in c.modes:
            assert p["unit_state"] == vc.unit_states(c.baked) and p["unit_state"][0] >= 0 and not p["silent_counted"]
    # the rows the packed shapes take for granted
    assert plans["row7_ss"]["e_flat"][2:] == [1, 1] and plans["row5_ss"]["e_flat"][2:] != [1, 1]
    assert max(plans["row0_ss"]["s_deg"]) == 3 and plans["general"]["csr"] == 1
    assert plans["row1_ss"]["silent_counted"] == 1 and plans["row6_multi"]["silent_counted"] == 1          # mark counts with counted silent states


def test_plan_hook_refuses_a_broken_edge_list(all_cases):
    """Arrays strq_model_create would refuse are a bad argument here too, with the same reason."""
    from strique_amd import ffi
    bk = all_cases["row6_ss"].baked
    src = np.array(bk.in_src).copy(); src[0] = bk.n_states + 5
    with pytest.raises(ffi.StriqueHipError, match="edge source out of range") as ei:
        ffi.debug_viterbi_plan(bk._replace(in_src=src))
    assert ei.value.code == ffi.STRQ_ERR_ARG


def _mode_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "vit_shapes_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "vit_shapes_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "--modes"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0, out.stdout.decode(errors="replace")
    return {tuple(int(v) for v in line.split()) for line in out.stdout.decode().splitlines()}


def test_cases_cover_the_mode_table(all_cases, plans, tmp_path):
    """Every (row, mode) vit_mode_ok has, single-stage and multi-stage, has a case; so have the general kernel and the
    register-resident one.  A new row or mode fails here until cases exist for it."""
    table = _mode_table(tmp_path)
    assert (0, 0) in table and (vc.SHAPE_G2, vc.VIT_UNIT) in table and (6, vc.VIT_HUB) in table and (6, vc.VIT_UNIT) not in table
    assert table == {(shape, mode) for shape, modes in vc.ROW_MODES.items() for mode in modes}          # the tests' copy of the table
    want = set()
    for shape, mode in table:
        if shape < vc.SHAPE_CSR:
            want |= {(shape, True, mode), (shape, False, mode)}
        else:
            want.add((shape, False, mode))
    assert {(s, m) for s, ss, m in want if s == vc.SHAPE_CSR} >= {(vc.SHAPE_CSR, vc.VIT_COUNT), (vc.SHAPE_CSR, vc.VIT_MARK)}
    assert {(s, m) for s, ss, m in want if s == vc.SHAPE_G2} == {(vc.SHAPE_G2, vc.VIT_COUNT), (vc.SHAPE_G2, vc.VIT_MARK), (vc.SHAPE_G2, vc.VIT_UNIT)}
    have = set()
    for name, c in all_cases.items():
        p = plans[name]
        for mode in c.modes:
            have.add((p["row"], p["ss"], mode))
            if c.g2 and mode != vc.VIT_BACKPTR:
                have.add((vc.SHAPE_G2, False, mode))
    assert not (want - have), sorted(want - have)


def _windows(all_cases):
    for name, c in all_cases.items():
        for label, x in c.windows:
            yield c, label, x


def test_references_agree(all_cases, orc):
    """A (the oracle's path) and B (the DP that carries the payloads) on every window: log-probability bits, count, both marks, the
    hub chain and the unit chain."""
    for c, label, x in _windows(all_cases):
        a = vc.reference_a(orc, c, label, x)
        b = vc.reference_b(c, label, x)
        what = (c.name, label)
        if label.startswith("nopath"):
            assert a["path"] is None and b["logp"] == -np.inf, what
            continue
        assert a["path"] is not None, what          # every other window has a path
        assert np.float64(a["logp"]).tobytes() == np.float64(b["logp"]).tobytes(), what
        assert (a["counted"], a["enter"], a["leave"]) == (b["counted"], b["enter"], b["leave"]), what
        assert vc.hub_chain(b["hub_last"], b["hub_rec"]) == a["hub"], what
        assert vc.unit_chain(b["unit_last"], b["unit_rec"]) == a["unit"], what
        for t, _ in a["hub"]:
            assert b["hub_live"][t], what
        for t, k in a["unit"]:
            assert b["unit_live"][t, k], what


def test_the_cases_test_something(all_cases, orc):
    for name, c in all_cases.items():
        refs = [(label, vc.reference_a(orc, c, label, x)) for label, x in c.windows if not label.startswith("nopath")]
        if vc.VIT_MARK in c.modes:
            assert any(a["enter"] and a["leave"] for _, a in refs), name
        if vc.VIT_HUB in c.modes:
            assert any(len(a["hub"]) >= 3 and len({br for _, br in a["hub"]}) >= 2 for _, a in refs), name
        # (the tie-prone variants leave the repeat after one round whatever the signal -- every round costs the same integer --
        # so their unit chain has one hop: they are here for the ties, checked below)
        if vc.VIT_UNIT in c.modes and not c.tie_prone:
            assert any(len(a["unit"]) >= 3 and {k for _, k in a["unit"]} == {0, 1} for _, a in refs), name
        if c.tie_prone:
            tied = 0
            for label, x in c.windows:
                a = vc.reference_a(orc, c, label, x); b = vc.reference_b(c, label, x)
                tied += sum(bool(b["tied"][t, s]) for t, s in enumerate(a["path"]))
            assert tied > 0, name
    # the boundary windows put both marks where the packed payload splits its fields
    got = {(a["enter"], a["leave"]) for label, x in all_cases["boundary_ss"].windows for a in [vc.reference_a(orc, all_cases["boundary_ss"], label, x)]}
    assert got == set(vc.BOUNDARY_TIMES)
    for v in ("ss", "multi", "csr"):
        c = all_cases["boundary_" + v]
        for (label, x), (enter, leave) in zip(c.windows, vc.BOUNDARY_TIMES):
            a = vc.reference_a(orc, c, label, x)
            assert (a["enter"], a["leave"], a["counted"]) == (enter, leave, leave - enter) and len(x) <= 8300


# ---- sourced windows ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def src_cases(all_cases, pm, pm_mod, cfg):
    return vc.sourced_cases(pm, pm_mod, cfg)


def _sourced(src_cases):
    for c in src_cases.values():
        for sw in vc.sourced_windows(c):
            yield c, sw


def test_uniform_support_parameter_moves_no_draw():
    """generated_model with the default support is what it was before the parameter existed (a digest of one model's arrays, taken
    from the code without it; floats to six decimals), and the wide twin differs in the Uniform emission parameters only."""
    def digest(bk):
        h = hashlib.sha256()
        for f in ("in_ptr", "in_src", "emis_kind", "count_inc", "tag"):
            h.update(np.ascontiguousarray(getattr(bk, f)).tobytes())
        for f in ("in_logp", "emis_a", "emis_b", "emis_c"):
            h.update(np.round(np.ascontiguousarray(getattr(bk, f), dtype=np.float64), 6).tobytes())
        return h.hexdigest()
    narrow = vc.generated_model(3, False)
    assert digest(narrow) == "e10a0107039599c91c4431c6e45d68f1327161a1d6ea622b5b205f2ae8d8024f"
    for row, multi, fan in ((3, False, 0), (7, True, 0), (1, True, 14)):
        a = vc.generated_model(row, multi, fan=fan); b = vc.generated_model(row, multi, fan=fan, support=vc.UNI_WIDE)
        for f in a._fields:
            if f not in ("emis_a", "emis_b", "emis_c"):
                va, vb = getattr(a, f), getattr(b, f)
                assert (va == vb) if isinstance(va, (int, list)) else np.array_equal(va, vb), (row, multi, fan, f)
        uni = np.asarray(a.emis_kind) == 2
        for f in ("emis_a", "emis_b", "emis_c"):
            assert np.array_equal(np.asarray(getattr(a, f))[~uni], np.asarray(getattr(b, f))[~uni]), (row, f)
        assert set(np.asarray(b.emis_a)[uni]) == {vc.UNI_WIDE[0]} and set(np.asarray(b.emis_b)[uni]) == {vc.UNI_WIDE[1]}
        assert vc.uniform_bounds(a) == (vc.UNI_LO, vc.UNI_HI) and vc.uniform_bounds(b) == vc.UNI_WIDE


def test_wide_cases_land_on_the_rows_of_their_twins(all_cases, plans, src_cases):
    from strique_amd import ffi
    assert list(src_cases) == list(vc.SOURCED_NAMES)
    for name in vc.WIDE_NAMES:
        c, twin = src_cases[name], all_cases[vc.narrow_name(name)]
        p, q = ffi.debug_viterbi_plan(c.baked), plans[twin.name]
        assert (p["shape"], p["row"], p["ss"], p["modes"]) == (q["shape"], q["row"], q["ss"], q["modes"]), (name, p, q)
        assert (c.row, c.ss, c.modes) == (twin.row, twin.ss, twin.modes) and p["row"] == c.row and p["ss"] == c.ss
        assert p["e_flat"] == q["e_flat"] and p["rec_state"] == q["rec_state"] and p["unit_state"] == q["unit_state"]


def test_sourced_windows_are_what_they_claim(src_cases, pm):
    """Labels, the window set of every case, the predicate, the clipped samples, the map, odd offsets."""
    seen_odd = False
    for name, c in src_cases.items():
        sws = vc.sourced_windows(c)
        labels = [sw.label for sw in sws]
        assert len(set(labels)) == len(labels), name
        ulo, uhi = vc.uniform_bounds(c.baked)
        if name not in vc.BOUNDARY_NAMES:
            i16 = {len(sw.samples) for sw in sws if sw.kind == vc.VIT_SRC_I16_AFFINE and not sw.label.startswith(("edge", "nopath"))}
            short = {len(sw.samples) for sw in sws if sw.label.startswith("nopath")}
            assert i16 | short >= set(vc.T_LIST) and short <= {1, 2}, (name, i16)
            assert {len(sw.samples) for sw in sws if sw.kind == vc.VIT_SRC_F64_AFFINE and sw.label.startswith("f64_T")} == {65, 333}, name
        else:
            assert not np.isfinite([ulo, uhi]).any()          # no Uniform emission: the predicate holds for any range
            assert [len(sw.samples) for sw in sws] == [len(x) for _, x in c.windows] and max(len(x) for _, x in c.windows) <= 8300
        if name.startswith("flanked_") or name.startswith("tie_"):          # the pipeline's range
            assert all(sw.consts[4:] == (pm.model_min + 0.5, pm.model_max - 0.5) for sw in sws if not sw.label.startswith("edge")), name
            assert (ulo, uhi) == ((0.0, 200.0) if c.tie_prone else (pm.model_min, pm.model_max)), name
        if name in vc.STRIQUE_NAMES:          # their own windows ride along, all that samples can hold
            own = [l for l, x in c.windows if not l.startswith("nopath") and np.isfinite(x).all() and not (l.startswith("T") and l[1:].isdigit() and int(l[1:]) in vc.T_LIST)]
            assert own and all(("i16_" + l in labels) or ("i16_own_" + l in labels) for l in own), (name, own, labels)
        off = 0
        for sw in sws:
            what = (name, sw.label)
            c1, h1, h2, c2, lo, hi = sw.consts
            assert h1 != 0 and lo <= hi, what
            assert sw.samples.dtype == (np.int16 if sw.kind == vc.VIT_SRC_I16_AFFINE else np.float64), what
            assert vc.predicate(c.baked, sw.consts) == sw.fast, what
            assert sw.fast == (not sw.label.startswith(("edge_lo_ulp", "edge_hi_ulp", "edge_nan"))), what
            if sw.label.startswith("edge_nan"):
                assert np.isnan(sw.x_prime).all() and len(sw.x_prime) == len(sw.samples), what
                continue
            # the map once more, by scalar arithmetic
            for t in (0, len(sw.samples) // 2, len(sw.samples) - 1):
                v = (float(sw.samples[t]) - c1) / h1
                v = v * h2 + c2
                assert min(max(v, lo), hi) == sw.x_prime[t], what
            assert np.isfinite(sw.x_prime).all() and sw.x_prime.min() >= lo and sw.x_prime.max() <= hi, what
            if len(sw.samples) >= 63:
                raw = (sw.samples.astype(np.float64) - c1) / h1 * h2 + c2
                assert ((raw < lo) & (sw.x_prime == lo)).any() and ((raw > hi) & (sw.x_prime == hi)).any(), what
                assert sw.samples.min() == -32768 and sw.samples.max() == 32767, what
            if sw.kind == vc.VIT_SRC_I16_AFFINE:
                seen_odd |= off % 2 == 1
                off += len(sw.samples)
        if name in vc.EDGE_NAMES:
            eq = [sw for sw in sws if sw.label.startswith("edge_eq")]
            assert eq and all((sw.consts[4], sw.consts[5]) == (ulo, uhi) for sw in eq), name
            lo_ulp = [sw for sw in sws if sw.label.startswith("edge_lo_ulp")]; hi_ulp = [sw for sw in sws if sw.label.startswith("edge_hi_ulp")]
            assert lo_ulp and all(sw.consts[4] < ulo and np.nextafter(sw.consts[4], np.inf) == ulo and sw.consts[5] == uhi for sw in lo_ulp), name
            assert hi_ulp and all(sw.consts[5] > uhi and np.nextafter(sw.consts[5], -np.inf) == uhi and sw.consts[4] == ulo for sw in hi_ulp), name
            assert any(np.isnan(sw.consts[0]) for sw in sws) and any(np.isnan(sw.consts[1]) for sw in sws), name
            # either source kind meets both values of the predicate in its launch
            for kind in (vc.VIT_SRC_I16_AFFINE, vc.VIT_SRC_F64_AFFINE):
                assert {sw.fast for sw in sws if sw.kind == kind} == {True, False}, (name, kind)
    assert seen_odd
    assert {n for n in vc.EDGE_NAMES} <= set(src_cases)


def test_references_agree_on_the_sourced_windows(src_cases, orc):
    for c, sw in _sourced(src_cases):
        label = vc.ref_label(sw)
        a = vc.reference_a(orc, c, label, sw.x_prime)
        b = vc.reference_b(c, label, sw.x_prime)
        what = (c.name, sw.label)
        if sw.label.startswith("nopath"):
            assert a["path"] is None and b["logp"] == -np.inf, what
            continue
        assert a["path"] is not None, what
        assert np.float64(a["logp"]).tobytes() == np.float64(b["logp"]).tobytes(), what
        assert (a["counted"], a["enter"], a["leave"]) == (b["counted"], b["enter"], b["leave"]), what
        assert vc.hub_chain(b["hub_last"], b["hub_rec"]) == a["hub"], what
        assert vc.unit_chain(b["unit_last"], b["unit_rec"]) == a["unit"], what
        for t, _ in a["hub"]:
            assert b["hub_live"][t], what
        for t, k in a["unit"]:
            assert b["unit_live"][t, k], what
        if sw.label.startswith("edge_nan"):          # the oracle on an all-NaN window of that length
            lp, path, counted = orc.viterbi(c.baked, np.full(len(sw.samples), np.nan))
            assert np.float64(lp).tobytes() == np.float64(a["logp"]).tobytes() and np.array_equal(path, a["path"]) and counted == a["counted"], what


def test_the_sourced_windows_test_something(src_cases, orc):
    """The criteria of test_the_cases_test_something, on the windows whose predicate is true."""
    for name, c in src_cases.items():
        sws = [sw for sw in vc.sourced_windows(c) if sw.fast and not sw.label.startswith("nopath")]
        refs = [vc.reference_a(orc, c, vc.ref_label(sw), sw.x_prime) for sw in sws]
        if vc.VIT_MARK in c.modes:
            assert any(a["enter"] and a["leave"] for a in refs), name
        if vc.VIT_HUB in c.modes:
            assert any(len(a["hub"]) >= 3 and len({br for _, br in a["hub"]}) >= 2 for a in refs), name
        if vc.VIT_UNIT in c.modes and not c.tie_prone:
            assert any(len(a["unit"]) >= 3 and {k for _, k in a["unit"]} == {0, 1} for a in refs), name
        if c.tie_prone:
            tied = 0
            for sw, a in zip(sws, refs):
                b = vc.reference_b(c, vc.ref_label(sw), sw.x_prime)
                tied += sum(bool(b["tied"][t, s]) for t, s in enumerate(a["path"]))
            assert tied > 0, name
    for v in ("ss", "multi", "csr"):
        c = src_cases["boundary_" + v]
        sws = vc.sourced_windows(c)
        assert len(sws) == len(vc.BOUNDARY_TIMES)
        for sw, (enter, leave) in zip(sws, vc.BOUNDARY_TIMES):
            a = vc.reference_a(orc, c, vc.ref_label(sw), sw.x_prime)
            assert (a["enter"], a["leave"], a["counted"]) == (enter, leave, leave - enter), (v, sw.label, a["enter"], a["leave"])


def test_sourced_cases_cover_the_mode_table(src_cases, tmp_path):
    """Every (row, single-stage, mode) of the table, the general kernel and the register-resident one have a sourced window whose
    predicate is true."""
    from strique_amd import ffi
    table = _mode_table(tmp_path)
    want = set()
    for shape, mode in table:
        if mode != vc.VIT_BACKPTR:
            want |= {(shape, True, mode), (shape, False, mode)} if shape < vc.SHAPE_CSR else {(shape, False, mode)}
    have = set()
    for name, c in src_cases.items():
        if not any(sw.fast and not sw.label.startswith("nopath") for sw in vc.sourced_windows(c)):
            continue
        p = ffi.debug_viterbi_plan(c.baked)
        for mode in c.modes:
            have.add((p["row"], p["ss"], mode))
            if c.g2:
                have.add((vc.SHAPE_G2, False, mode))
    assert not (want - have), sorted(want - have)
