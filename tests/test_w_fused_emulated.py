"""w formed inside the q2 / q2l advection march, on the host build of the unmodified kernel sources (tests/emu): the checks of
tests/w_fused_checks.py against the CPU oracle, bit for bit, and the launch counts from the library's own event profile."""
import os
import subprocess

import pytest

import w_fused_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("nml", list(chk.NAMELISTS))
@pytest.mark.parametrize("case", chk.CASES)
def test_unobserved_steps_every_case_and_namelist(case, nml):
    """run(2), run(1), run(3), one download: every array that is not scratch, w included; one k_advq2_col and no k_vertvl per body step"""
    chk.unobserved_steps(EMU, case, chk.NAMELISTS[nml], (65, 49, 21))


def test_inputs_exercise_the_fused_march():
    """archipelago: w is not zero, not at the surface (a surface volume flux) nor at the bottom, and there is land inside the rim"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), need=("w", "w_surface", "w_bottom", "vfluxf", "land_inside", "q2"))


@pytest.mark.parametrize("size", chk.SIZES[1:], ids=str)
def test_unobserved_steps_every_shape(size):
    chk.unobserved_steps(EMU, "archipelago", None, size)


@pytest.mark.parametrize("switch", list(chk.KEEP))
def test_paths_that_keep_the_pair(switch):
    """POMGPU_W_NOFUSE, POMGPU_ADVQ_SINGLE, POMGPU_ADVQ_EXCHANGE: k_vertvl once per body step, the same bits"""
    chk.unobserved_steps(EMU, "archipelago", None, (65, 49, 21), switch=switch)


def test_unmasked_surface_flux_on_land():
    chk.land_forced(EMU)


def test_unmasked_surface_flux_on_land_pair():
    chk.land_forced(EMU, switch="W_NOFUSE")


def test_switch_flipped_on_a_live_context():
    chk.switch_flipped_live(EMU)


def test_routine_by_routine_host_is_fused():
    chk.routine_by_routine(EMU)


def test_stand_alone_vertvl_keeps_its_kernel():
    chk.stand_alone_entry_points(EMU)


def test_fp64_fused_equals_pair():
    chk.fused_equals_pair(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_fused_equals_pair(variant):
    """the unfused kernel reads w back rounded to the storage type: the fused one must round what it multiplies with q.  The
    fp32-arithmetic variant keeps the pair (no fp64 arithmetic in its stencil kernels): vertvl shows on both sides there"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.fused_equals_pair(VARIANTS[variant], fuses=variant != "f32a")
