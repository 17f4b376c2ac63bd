"""The depth-mean correction of u, v applied on load, on the host build of the unmodified kernel sources (tests/emu): the checks of
tests/uvmean_onload_checks.py against the CPU oracle, bit for bit, and the launch counts from the library's own event profile.  The
emulation runs one lane at a time and reads neighbour rows and lanes from memory through the same helper (uvm_ld): the LDS slabs and
lane shifts of the device kernels are covered by tests/test_gpu_uvmean_onload.py."""
import os
import subprocess

import pytest

import uvmean_onload_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    """run(2), run(1), run(3), one download: every array that is not scratch; no k_int_uvmean* per body step (nadv = 1: one)"""
    chk.unobserved_steps(EMU, case, chk.NAMELISTS[nml], (65, 49, 21), onload=nml not in chk.FALLBACK_NML)


def test_inputs_exercise_the_correction():
    """archipelago: the correction changes u and v, in the interior and on the frame of the rim filter; land inside; cu != cv"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), need=chk.ALL_NEEDS)


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(EMU, "archipelago", None, size)


def test_kb_beyond_the_register_kernels_keeps_the_pass():
    chk.unobserved_steps(EMU, "archipelago", None, chk.SIZE_FALLBACK, onload=False)


@pytest.mark.parametrize("switch", chk.KEEP)
def test_paths_that_keep_the_pass(switch):
    """POMGPU_UVMEAN_PASS, POMGPU_W_NOFUSE, POMGPU_UV_NOFUSE, POMGPU_ADVT2_SINGLE: k_int_uvmean* once per body step, the same bits"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), switch=switch)


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(EMU)


def test_routine_by_routine_host_corrects_on_load():
    chk.routine_by_routine(EMU)


def test_upload_of_u_before_mode_internal_falls_back():
    chk.routine_by_routine(EMU, upload_u=True)


def test_upload_of_another_u_before_mode_internal():
    chk.upload_changes_u(EMU)


def test_stand_alone_entry_points_keep_their_kernels():
    chk.stand_alone_entry_points(EMU)


def test_fp64_onload_equals_pass():
    chk.onload_equals_pass(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_onload_equals_pass(variant):
    """the pass stored u, v rounded to the storage type: the on-load correction must round what it hands on.  The fp32-arithmetic
    variant keeps the pass (no fp64 arithmetic in its stencil kernels): it shows on both sides there"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.onload_equals_pass(VARIANTS[variant], onload=variant != "f32a")
