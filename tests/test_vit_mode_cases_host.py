"""The cases of tests/vit_mode_cases.py, checked without a GPU: which kernel shape every model lands on (strq_debug_viterbi_plan), that
the case list covers the table of (shape, mode) pairs in strique_amd/csrc/vit_model.h, that the two references agree, and that the
cases exercise what they are there for.  tests/test_gpu_viterbi_modes.py then holds the kernels against the same references."""
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
    assert lib.strq_debug_viterbi_plan and lib.strq_debug_viterbi_mode


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
