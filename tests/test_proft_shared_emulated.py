"""proft of T and S in one lane, on the host build of the unmodified kernel sources (tests/emu): the checks of tests/proft_shared_checks.py
against the CPU oracle, bit for bit, and the path from the library's own event profile.  The emulation runs one lane at a time: what
the device adds (registers, the order of loads) is covered by tests/test_gpu_proft_shared.py."""
import os
import subprocess

import pytest

import proft_shared_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("nbct,nbcs", chk.PAIRS)
@pytest.mark.parametrize("case", chk.CASES)
def test_every_pair_of_surface_conditions(case, nbct, nbcs):
    """(1,1) and (3,3) in one lane; the mixed classes (1,3), (3,1), (2,4), (4,2) and the short-wave pairs the twin; the rest two launches"""
    chk.whole_steps(EMU, case, (65, 49, 21), nbct, nbcs)


@pytest.mark.parametrize("nbc", [1, 3])
@pytest.mark.parametrize("size", chk.SHAPES, ids=str)
def test_every_shape(size, nbc):
    """kb below the template's bound (levels computed on clamped operands and discarded), at it, and past the one-lane kernel's last"""
    chk.whole_steps(EMU, "archipelago", size, nbc, nbc)


@pytest.mark.parametrize("nbc", [1, 3])
def test_switch_keeps_the_twin(nbc):
    chk.whole_steps(EMU, "archipelago", (65, 49, 21), nbc, nbc, switch=True)


@pytest.mark.parametrize("nbc", [1, 3])
def test_switch_flipped_on_a_live_context(nbc):
    chk.switch_flipped_live(EMU, nbc)


def test_fp64_lane_equals_twin():
    chk.lane_equals_twin(EMU)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_study_builds_lane_equals_twin(variant):
    """f and kh come through the storage type and the result is rounded to it on store; the solve is fp64 in both variants"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.lane_equals_twin(VARIANTS[variant])


def test_tiles_2x2_equal_the_single_tile():
    chk.tiles_2x2(EMU)
