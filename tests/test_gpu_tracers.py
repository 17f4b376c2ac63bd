"""Passive tracers on an MI355X: the checks of tests/tracer_checks.py with the product library against tests/tracer_expect.py, bit for
bit -- the LDS slabs, lane shifts and the UM forms (k_advt2_col<1, true>, <2, true>) that the host emulation does not have."""
import os
import subprocess
import sys

import pytest

import tracer_checks as chk

pytestmark = pytest.mark.gpu
LIB = None                                                    # the product library (extpom_amd.lib.LIBPATH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", chk.CASES)
def test_twins_from_a_started_state(case):
    chk.twins_started(LIB, case)


@pytest.mark.parametrize("case", chk.CASES)
def test_twins_from_a_cold_start(case):
    chk.twins_cold(LIB, case)


@pytest.mark.parametrize("nbc", [1, 3])
@pytest.mark.parametrize("adv", chk.ADV, ids=str)
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_independent_tracer_against_the_expectation(case, size, adv, nbc):
    chk.against_expectation(LIB, case, size, adv, nbc, need_branches=size == chk.SIZES[0])


@pytest.mark.parametrize("switch", [None, "TR_NOPAIR", "ADVT2_SINGLE", "UVMEAN_PASS"])
@pytest.mark.parametrize("ntr", [2, 3, 8])
def test_pairs_and_an_odd_tracer_against_the_expectation(ntr, switch):
    chk.against_expectation(LIB, "archipelago", (20, 17, 6) if ntr == 8 else (65, 49, 21), ntr=ntr, switch=switch, steps=3, need_branches=False)


@pytest.mark.parametrize("case", chk.CASES)
def test_mode_4_moves_the_tracer_alone(case):
    chk.mode4(LIB, case)


@pytest.mark.parametrize("adv", [(1, 1), (2, 2)], ids=str)
def test_mode_4_with_the_other_advections(adv):
    chk.against_expectation(LIB, "archipelago", (20, 17, 6), adv, nml=dict(mode=4), need_branches=False)


def test_tracers_do_not_touch_the_flow():
    chk.no_interference(LIB)


def test_step_forms_agree():
    chk.step_forms(LIB)


def test_refusals():
    chk.refusals(LIB)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    from extpom_amd import lib as L
    chk.fp32_builds_refuse({"f32": L.LIBPATH_F32, "f32a": L.LIBPATH_F32A}[variant])


@pytest.mark.parametrize("split", [(1, 2), (2, 2)], ids=str)
def test_tiles_match_the_single_tile(split):
    """thread tiles in a child process (tests/gpu_tracer_tiles.py): tracer arrays on owned cells equal the single tile's, the added message
    rounds are the derived number and none with tracers off"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_tracer_tiles.py"), str(split[0]), str(split[1])],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "TRACER TILES OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
