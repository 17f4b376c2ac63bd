"""Round trips through tclim, sclim, rmean read only where bits change, on the host builds of the unmodified kernel sources (tests/emu):
the checks of tests/rt_flags_checks.py -- flags, POMGPU_RT_LOAD and n x run(1) against the CPU oracle, bit for bit, and the host's
decisions from the event profile's counts ts_rt_flags and profq_rm_flags.  (The host build forms a word bit by bit, one lane at a time;
the lane mask and its store run on the device, tests/test_gpu_rt_flags.py.)"""
import os
import subprocess

import pytest

import rt_flags_checks as chk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "_emu", "libpomgpu_emu.so")
VARIANTS = {"f32": os.path.join(ROOT, "tests", "_emu_f32", "libpomgpu_emu_f32.so"), "f32a": os.path.join(ROOT, "tests", "_emu_f32a", "libpomgpu_emu_f32a.so")}


@pytest.fixture(scope="module", autouse=True)
def emu_lib():
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("clim", chk.CLIMS)
@pytest.mark.parametrize("case,size", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_inputs_are_what_they_claim(case, size, clim):
    chk.inputs_are_what_they_claim(case, size, clim)


@pytest.mark.parametrize("clim", chk.CLIMS)
@pytest.mark.parametrize("case,size", chk.SHAPES, ids=chk.SHAPE_IDS)
def test_same_bits_every_way(case, size, clim):
    chk.same_bits_every_way(EMU, case, size, clim)


@pytest.mark.parametrize("variant", ["f32", "f32a"])
def test_fp32_builds_same_bits_every_way(variant):
    """the fp32 study builds take the flag path (the flags are formed and used in their own compute type); no oracle for them: flags
    against POMGPU_RT_LOAD against 4 x run(1)"""
    subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu_variant.sh"), variant], stdout=subprocess.DEVNULL)
    chk.same_bits_every_way(VARIANTS[variant], "archipelago", (65, 49, 21), "part", oracle=False)


def test_switch_on_a_live_context():
    chk.switch_on_a_live_context(EMU)


def test_decision_address_handed_out():
    chk.decision_address_handed_out(EMU)


def test_decision_advt2_single():
    chk.decision_advt2_single(EMU)


def test_decision_stand_alone_pair():
    chk.decision_stand_alone_pair(EMU)


@pytest.mark.parametrize("how", ["download", "upload"])
def test_observer_between_routines(how):
    chk.observer_between_routines(EMU, how)


def test_upload_changes_rho():
    chk.upload_changes_rho(EMU)
