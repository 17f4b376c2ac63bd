"""aam and aam2d formed inside advct's march, on the host build of the unmodified kernel sources (tests/emu): the checks of
tests/aam_fused_checks.py against the CPU oracle, bit for bit, and the launch counts from the library's own event profile."""
import os
import subprocess

import pytest

import aam_fused_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    """run(2), run(1), run(3), one download: every array that is not scratch, aam and aam2d included; per step one k_advct_col that
    formed aam, no k_aam_pair, k_aam or k_vint.  The default namelist makes no canonical copy in its steps; nadv = 1 (advt1 reads the
    slot) makes them in front of mode_internal's 3-D part"""
    chk.unobserved_steps(EMU, case, chk.NAMELISTS[nml], (65, 49, 21), copies=0 if nml in ("default", "mode4", "npg2") else None)


def test_inputs_exercise_the_fused_march():
    """archipelago: the new aam differs from aam_init in the interior, the rim keeps aam_init (off zero), aam2d is not constant and
    there is land inside the rim"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), need=("aam_new", "rim_keeps_init", "aam2d_varies", "land_inside"))


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(EMU, "archipelago", None, size, copies=0)


def test_aam_nofuse_keeps_the_pair():
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), switch="AAM_NOFUSE")


@pytest.mark.parametrize("switch", chk.STILL_FUSED)
def test_single_field_marches_read_the_current_buffer(switch):
    """POMGPU_ADVT2_SINGLE, POMGPU_ADVQ_SINGLE: k_advt2_col<1>, k_advq_col<1> read aam where it lives, no copy"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), switch=switch, copies=0)


def test_nadv1_copies_in_front_of_advt1():
    """three steps: the first skips the 3-D part, the second finds aam back in its slot, the third copies"""
    chk.unobserved_steps(EMU, "seamount", dict(nadv=1), (20, 17, 6), calls=(3,), copies=1)


def test_both_parities_observed_and_an_upload_at_the_odd_one():
    chk.both_parities(EMU)


def test_both_parities_with_the_time_mean_on():
    chk.both_parities(EMU, mean=True)


def test_restart_written_and_read_at_the_odd_parity(tmp_path):
    chk.restart_at_the_odd_parity(EMU, tmp_path)


def test_address_handed_out_ends_the_fusion():
    chk.address_handed_out(EMU)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(EMU)


def test_stand_alone_entry_points_after_fused_steps():
    chk.stand_alone_entry_points(EMU)


def test_routine_by_routine_host_keeps_the_pair_without_a_copy_per_step():
    chk.routine_by_routine(EMU)


def test_fp64_fused_equals_pair():
    chk.fused_equals_pair(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_fused_equals_pair(variant):
    """k_vint reads aam back rounded to the storage type: the fused march must sum what it stores.  The fp32-arithmetic variant keeps
    the pair (no fp64 arithmetic in its stencil kernels): k_aam and k_vint show on both sides there"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fused_equals_pair(VARIANTS[variant], fuses=variant != "f32a")
