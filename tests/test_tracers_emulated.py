"""Passive tracers on the host build of the unmodified kernel sources (tests/emu): the checks of tests/tracer_checks.py against
tests/tracer_expect.py, bit for bit.  The emulation runs one lane at a time: the LDS slabs and lane shifts of the device kernels are
covered by tests/test_gpu_tracers.py.  The tests named pin_* hold the expectation itself and pass without the feature, by design."""
import os
import subprocess

import pytest

import tracer_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


# ---- pins of the expectation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adv", chk.ADV, ids=str)
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_pin_hooked_run_equals_plain_run(case, size, adv):
    chk.pin_hooked_run_equals_plain_run(case, size, adv)


@pytest.mark.parametrize("adv", [(2, 1), (1, 1)], ids=str)   # (not nitera > 1: tests/tracer_expect.py says why)
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_pin_stage_reproduces_t_and_s(case, size, adv):
    chk.pin_stage_reproduces_t_and_s(case, size, adv)


@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_pin_bcond4_one_equals_the_oracles_bcond4(case, size):
    chk.pin_bcond4_one(case, size)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", chk.CASES)
def test_twins_from_a_started_state(case):
    chk.twins_started(EMU, case)


@pytest.mark.parametrize("case", chk.CASES)
def test_twins_from_a_cold_start(case):
    chk.twins_cold(EMU, case)


@pytest.mark.parametrize("nbc", [1, 3])
@pytest.mark.parametrize("adv", chk.ADV, ids=str)
@pytest.mark.parametrize("size", chk.SIZES, ids=str)
@pytest.mark.parametrize("case", chk.CASES)
def test_independent_tracer_against_the_expectation(case, size, adv, nbc):
    chk.against_expectation(EMU, case, size, adv, nbc, need_branches=size == chk.SIZES[0])


@pytest.mark.parametrize("switch", [None, "TR_NOPAIR", "ADVT2_SINGLE", "UVMEAN_PASS"])
@pytest.mark.parametrize("ntr", [2, 3, 8])
def test_pairs_and_an_odd_tracer_against_the_expectation(ntr, switch):
    chk.against_expectation(EMU, "archipelago", (20, 17, 6) if ntr == 8 else (65, 49, 21), ntr=ntr, switch=switch, steps=3, need_branches=False)


@pytest.mark.parametrize("case", chk.CASES)
def test_mode_4_moves_the_tracer_alone(case):
    chk.mode4(EMU, case)


@pytest.mark.parametrize("adv", [(1, 1), (2, 2)], ids=str)
def test_mode_4_with_the_other_advections(adv):
    chk.against_expectation(EMU, "archipelago", (20, 17, 6), adv, nml=dict(mode=4), need_branches=False)


def test_tracers_do_not_touch_the_flow():
    chk.no_interference(EMU)


def test_step_forms_agree():
    chk.step_forms(EMU)


def test_refusals():
    chk.refusals(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fp32_builds_refuse(VARIANTS[variant])


@pytest.mark.parametrize("split,adv", [((1, 2), (2, 1)), ((2, 2), (2, 1)), ((2, 2), (2, 2)), ((2, 2), (1, 1))], ids=str)
def test_tiles_match_the_single_tile(split, adv):
    """1x2 and 2x2 emulated tiles: owned cells equal the single tile, the added rounds are the derived number, none with tracers off"""
    chk.tiles(EMU, split[0], split[1], adv=adv)
