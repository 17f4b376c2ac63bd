"""Tides on the host build of the unmodified kernel sources (tests/emu): the checks of tests/tide_checks.py against tests/tide_expect.py.
The emulation runs one lane at a time; the two-substep pass (k_ext_march2) and the one-launch loop (k_ext_loop) do not exist in it and are
shown excluded here -- tests/test_gpu_tides.py reaches them on the device."""
import os
import subprocess

import pytest

import tide_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


# ---- 1: the forcing against the oracle ---------------------------------------------------------------------------------------------------------
def test_tide_phasors_equal_the_c_librarys():
    chk.phasors(EMU)


@pytest.mark.parametrize("with_un", [True, False], ids=["un", "el_only"])
@pytest.mark.parametrize("nc", chk.NCS)
@pytest.mark.parametrize("case,size", chk.CASES, ids=[c for c, _ in chk.CASES])
def test_run_with_a_tide_equals_the_oracle(case, size, nc, with_un):
    chk.forcing(EMU, case, size, nc, with_un)


@pytest.mark.parametrize("kw", [dict(lramp=True), dict(time0=0.75), dict(nml=dict(mode=2), path="mode2"), dict(nml=dict(mode=4)), dict(sides=("west", "north")),
                                dict(lramp=True, time0=0.75, nml=dict(mode=4), sides=("east",))],
                         ids=["lramp", "time0", "mode2", "mode4", "two_sides", "all_at_once"])
def test_run_with_a_tide_ramp_time0_modes(kw):
    chk.forcing(EMU, "island", (20, 17, 6), 2, True, **kw)


@pytest.mark.parametrize("case,size", [chk.CASES[0], chk.CASES[2]], ids=["island", "seamount"])
@pytest.mark.parametrize("path", list(chk.PATHS))
def test_every_external_path_carries_the_tide(path, case, size):
    if path == "mode2":
        chk.forcing(EMU, case, size, 2, True, nml=dict(mode=2), path=path)
    else:
        chk.forcing(EMU, case, size, 2, True, path=path, excluded=path in chk.DEVICE_ONLY)


def test_the_tide_changes_the_flow():
    chk.tide_matters(EMU)


def test_routine_by_routine_host_gets_the_tide():
    chk.stand_alone(EMU)


# ---- 2: tiles ---------------------------------------------------------------------------------------------------------------------------------
def test_four_tiles_equal_one_with_the_tide():
    chk.tiles(EMU)


# ---- 3: off means off ----------------------------------------------------------------------------------------------------------------------------
def test_no_table_is_a_context_that_never_heard_of_tides():
    chk.off_means_off(EMU)


def test_zero_coefficients_are_no_tide_and_one_launch_a_step():
    chk.zero_tide_is_no_tide(EMU)


# ---- 4: the analysis ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("steps", [1, 2, 7])
def test_harmonic_sums_and_matrix_bit_for_bit(steps, every):
    chk.harmonic_sums(EMU, steps, every)


def test_harmonic_sums_eight_constituents():
    chk.harmonic_sums(EMU, 3, 1, nc=8, case="archipelago", size=(8, 8, 6))


def test_harmonic_solve_against_numpy():
    chk.harmonic_solve(EMU)


def test_closed_form_signal_comes_back_with_its_phase():
    chk.closed_form(EMU)


def test_harmonic_launch_counts():
    chk.harmonic_launches(EMU)


# ---- 5: hosts ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    chk.refusals(EMU)


# ---- 6: files ------------------------------------------------------------------------------------------------------------------------------------
def test_harmonics_file_matches_its_schema_and_the_solve(tmp_path):
    chk.harmonics_file(EMU, tmp_path)


def test_tide_file_equals_set_tides(tmp_path):
    chk.tide_file(EMU, tmp_path)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_refuse(variant):
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fp32_builds_refuse(VARIANTS[variant])
